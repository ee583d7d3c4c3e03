#!/usr/bin/env python3
"""Guided ISMCTS (ddz_gismcts_step, csrc/ddz_gismcts.h: k_gismcts) against the two kernels it composes, in ONE process on the
same tables, at 65,536 tables x 1 tree and at 64 tables x 64 trees, budget --budget:

  the device time of one ddz_gismcts_step (one iteration of every (table, tree) on that iteration's world): median [min-max]
  over the steps of a search, the first --skip steps left out, with constant leaf values so that nothing but the step is
  between the events,
  the same for one ddz_guided_step of the hidden form (k_guided<true>: the tree re-applies stored moves and enumerates a list
  only where it expands; k_gismcts enumerates one at every level of its descent),
  ismcts()'s device time / budget at the same shape: what one iteration costs inside the one-launch kernel, its random
  playout included,
  the mean depth of the guided-ISMCTS descents (moves applied / iterations run, from the totals).

Device time = HIP events on the current stream after a warm-up; the one-launch kernel as the median [min-max] of --reps
calls.  The tables are --plies random plies into their games.  Writes the table to --notes if given.

  python tools/gismcts_probe.py [--reps 5] [--plies 12] [--budget 64] [--notes FILE]
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from guided_probe import timed  # noqa: E402  (the same directory)
from search_probe import make_env  # noqa: E402

SHAPES = ((65536, 1), (64, 64))


def step_times(open_search, budget, skip):
    """(ms of every step behind the first `skip` of one search with constant values, its totals int64 [4])"""
    s = open_search()
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
    totals = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    s.close(totals)
    return out, totals.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--notes", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    lines = ["| tables x trees | guided-ISMCTS step, ms | guided step (hidden), ms | ismcts() / budget, ms | v4 / guided step | "
             "v4 step / ismcts | mean depth, v4 | mean depth, guided |", "|---|---|---|---|---|---|---|---|"]
    fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}-{t[2]:.3f}]"   # noqa: E731
    for T, trees in SHAPES:
        env = make_env(pkg, T, a.plies)
        visits = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        wins = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        rows = {}
        for name, make in (("v4", lambda: env.guided_ismcts(a.budget, trees=trees)),
                           ("v3", lambda: env.guided(a.budget, trees=trees, hidden=True))):
            make().close()                              # (the workspace allocated, the kernel loaded)
            steps, totals = step_times(make, a.budget, a.skip)
            rows[name] = ((statistics.median(steps), min(steps), max(steps)), totals[0].item() / max(1, totals[1].item()))
        ts = timed(lambda: env.ismcts(a.budget, trees=trees, visits=visits, wins=wins), a.reps)
        per = tuple(x / a.budget for x in ts)
        v4, v3 = rows["v4"], rows["v3"]
        row = (f"| {T} x {trees} | {fmt(v4[0])} | {fmt(v3[0])} | {fmt(per)} | {v4[0][0] / v3[0][0]:.2f} | {v4[0][0] / per[0]:.2f} | "
               f"{v4[1]:.2f} | {v3[1]:.2f} |")
        print(row, flush=True)
        lines.append(row)
        assert env.status() == 0
        del env
        torch.cuda.empty_cache()
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("# Guided ISMCTS (search spec v4): its step against guided UCT's and the one-launch ISMCTS\n\n"
                    f"`python tools/gismcts_probe.py --reps {a.reps} --plies {a.plies} --budget {a.budget}`: HIP events, medians "
                    "[min-max]; the steps over the steps of one search with constant leaf values, `ismcts()` at the same shape "
                    "divided by its budget; mean depth = moves applied / iterations run.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
