#!/usr/bin/env python3
"""Guided UCT (ddz_guided_step, csrc/ddz_guided.h: k_guided) against its yardstick, the one-launch UCT search (ddz_search:
k_search), in ONE process on the same tables, at 65,536 tables x 1 tree and at 64 tables x 64 trees, budget --budget:

  the device time of one ddz_guided_step (one iteration of every (table, tree)): median [min-max] over the steps of a
  search, the first --skip steps left out, with constant leaf values so that nothing but the step is between the events,
  search()'s device time / budget at the same shape: what one iteration costs inside the one-launch kernel.  The phased form
  re-enters the table and, hidden, re-deals on every launch; the ratio of the two is what that costs per iteration,
  the device time of one call of engine.PlayoutLeaf(--playouts) and of dqn_glue.QLeaf (face variant 3, one untrained
  network for the three roles) on the leaves of step --skip of such a search.

Device time = HIP events on the current stream after a warm-up; medians [min-max] of --reps calls (of the steps, for the
step).  The tables are --plies random plies into their games.  Writes the table to --notes (profiles/r21_notes.md).

  python tools/guided_probe.py [--reps 5] [--plies 12] [--budget 64] [--playouts 8] [--notes profiles/r21_notes.md]
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from search_probe import make_env  # noqa: E402  (the same directory)

SHAPES = ((65536, 1), (64, 64))


def timed(fn, reps):
    """(median, min, max) ms of fn() by events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def step_times(env, budget, trees, hidden, skip):
    """ms of every step behind the first `skip` of one search with constant values, and the search left open at step `skip`
    of a second one (its leaves are what the evaluators are timed on)"""
    kw = dict(trees=trees, hidden=hidden, roles=0b111)
    s = env.guided(budget, **kw)
    s.values.fill_(512)
    out = []
    for i in range(budget):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.step()
        b.record()
        b.synchronize()
        if i >= skip:
            out.append(a.elapsed_time(b))
    s.close()
    s = env.guided(budget, **kw)
    s.values.fill_(512)
    for _ in range(skip + 1):
        s.step()
    return out, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--playouts", type=int, default=8)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--notes", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    torch.manual_seed(0)
    net = pkg.dqn_glue.QNet(pkg.FACE_PLANES[3]).to("cuda:0").eval()
    lines = ["| tables x trees | form | guided step, ms | search() / budget, ms | step / search | PlayoutLeaf(%d), ms | QLeaf v3, ms | leaves |"
             % a.playouts, "|---|---|---|---|---|---|---|---|"]
    fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}-{t[2]:.3f}]"   # noqa: E731
    for T, trees in SHAPES:
        env = make_env(pkg, T, a.plies)
        visits = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        wins = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        for hidden in (False, True):
            steps, s = step_times(env, a.budget, trees, hidden, a.skip)
            st = (statistics.median(steps), min(steps), max(steps))
            need = int(s.need.sum().item())
            playout = pkg.PlayoutLeaf(a.playouts)
            qleaf = pkg.QLeaf({"lord": net, "down": net, "up": net}, 3)
            tp = timed(lambda: playout(s), a.reps)
            tq = timed(lambda: qleaf(s), a.reps)
            s.close()
            ts = timed(lambda: env.search(a.budget, trees=trees, hidden=hidden, visits=visits, wins=wins), a.reps)
            per = tuple(x / a.budget for x in ts)
            row = (f"| {T} x {trees} | {'hidden' if hidden else 'open'} | {fmt(st)} | {fmt(per)} | {st[0] / per[0]:.2f} | {fmt(tp)} | "
                   f"{fmt(tq)} | {need} of {T * trees} |")
            print(row)
            lines.append(row)
            del playout, qleaf, s
        assert env.status() == 0
        del env
        torch.cuda.empty_cache()
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("# Guided UCT (search spec v3): one iteration per launch against the one-launch search\n\n"
                    f"`python tools/guided_probe.py --reps {a.reps} --plies {a.plies} --budget {a.budget} --playouts {a.playouts}`: "
                    "HIP events, medians [min-max]; the step over the steps of one search with constant leaf values, the "
                    "evaluators on the leaves of one step, `search()` at the same shape divided by its budget.\n\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
