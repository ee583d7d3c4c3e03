#!/usr/bin/env python3
"""Guided PUCT (ddz_puct_step, csrc/ddz_puct.h: k_puct) against its yardstick, guided UCT (ddz_guided_step: k_guided), in ONE
process on the same tables:

  the device time of one step (one iteration of every (table, tree)) of both at 65,536 tables x 1 tree, open and hidden:
  median [min-max] over the steps of a search, the first --skip left out, with leaf values (and, PUCT, prior weights) drawn
  once per item so that nothing but the step is between the events; their ratio and the workspace bytes per tree,
  the lord's win rate against the RULE farmers (env.auto_choose(0b101)) with engine.PlayoutLeaf(--playouts) as the leaf
  evaluator at --trees x --budget iterations on sampled hands, by guided_puct_choose (most visits) and by guided_choose
  (mode "sides", the best win ratio), one run each of --tables x --iterations steps, with the binomial standard error, c and
  the share of PUCT nodes that fell back to uniform priors.

Device time = HIP events on the current stream.  The step tables are --plies random plies into their games.  Writes the
tables to --notes.

  python tools/puct_probe.py [--budget 64] [--trees 4] [--playouts 4] [--tables 1024] [--iterations 200] [--c 1.25] [--notes FILE]
"""
import argparse
import importlib
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from search_probe import make_env  # noqa: E402  (the same directory)


def step_times(env, puct, budget, hidden, skip, c):
    """ms of every step behind the first `skip` of one search whose values / priors were drawn once, and its bytes per tree"""
    kw = dict(trees=1, hidden=hidden, roles=0b111)
    s = env.guided_puct(budget, c=c, **kw) if puct else env.guided(budget, mode="sides", **kw)
    g = torch.Generator(device="cuda:0").manual_seed(5)
    s.values.copy_(torch.randint(0, 1025, s.values.shape, generator=g, device="cuda:0", dtype=torch.int32))
    if puct:
        s.priors.copy_(torch.randint(0, 256, s.priors.shape, generator=g, device="cuda:0", dtype=torch.int32).to(torch.uint8))
    out = []
    for i in range(budget):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.step()
        b.record()
        b.synchronize()
        if i >= skip:
            out.append(a.elapsed_time(b))
    totals = torch.zeros(5, dtype=torch.int64, device="cuda:0")
    s.close(totals)
    per = (env.lib.ddz_puct_work_bytes(1, budget, 1, s.pool) if puct else env.lib.ddz_guided_work_bytes(1, budget, 1))
    return (statistics.median(out), min(out), max(out)), per, totals.tolist()


def match(pkg, a, puct):
    """the lord by guided PUCT or by guided UCT on sampled hands, the farmers by the rule agent -> (stats, totals)"""
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device="cuda:0")
    env.reset()
    lord = torch.empty(a.tables, dtype=torch.int32, device="cuda:0")
    leaf = pkg.PlayoutLeaf(a.playouts)
    totals = torch.zeros(5, dtype=torch.int64, device="cuda:0")
    for it in range(a.iterations):
        leaf.salt = it
        if puct:
            visits, _ = env.guided_puct(a.budget, trees=a.trees, c=a.c, salt=it, hidden=True, roles=0b010).run(leaf, totals=totals)
            env._choose_wins(visits, lord)
        else:
            env.guided_choose(leaf, a.budget, trees=a.trees, mode="sides", salt=it, hidden=True, roles=0b010, out=lord)
        env.step_slab(torch.where(env.role == 1, lord, env.auto_choose(0b101)), pkg.STEP_IDS, auto_reset=True)
    assert env.status() == 0
    return env.stats(), totals.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--trees", type=int, default=4)
    ap.add_argument("--playouts", type=int, default=4)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=200, help="0: no match")
    ap.add_argument("--step-tables", type=int, default=65536, help="0: no step timing")
    ap.add_argument("--c", type=float, default=1.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--notes", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}-{t[2]:.3f}]"   # noqa: E731
    steps = ["| tables x trees | form | guided step, ms | guided_puct step, ms | puct / guided | bytes per tree, guided | puct | "
             "moves per iteration, guided | puct |", "|---|---|---|---|---|---|---|---|---|"]
    if a.step_tables:
        env = make_env(pkg, a.step_tables, a.plies)
        for hidden in (False, True):
            for _ in range(2):                                 # (the first pass warms both up)
                tg, bg, totg = step_times(env, False, a.budget, hidden, a.skip, a.c)
                tp, bp, totp = step_times(env, True, a.budget, hidden, a.skip, a.c)
            row = (f"| {a.step_tables} x 1 | {'hidden' if hidden else 'open'} | {fmt(tg)} | {fmt(tp)} | {tp[0] / tg[0]:.2f} | {bg} | {bp} | "
                   f"{totg[0] / max(1, totg[1]):.2f} | {totp[0] / max(1, totp[1]):.2f} |")
            print(row, flush=True)
            steps.append(row)
        assert env.status() == 0
        del env
        torch.cuda.empty_cache()
    games = ["| lord | games | lord wins | rate | standard error | uniform-fallback nodes |", "|---|---|---|---|---|---|"]
    rates = {}
    if a.iterations:
        for puct in (True, False):
            st, totals = match(pkg, a, puct)
            n, w = st["episodes"], st["lord_wins"]
            p = w / max(1, n)
            se = math.sqrt(p * (1 - p) / max(1, n))
            rates[puct] = (p, se)
            name = f"guided_puct, c = {a.c}, most visits" if puct else "guided, mode sides, c = 0.7, best ratio"
            share = f"{totals[4]} of {totals[3] + totals[1] // a.budget} ({totals[4] / max(1, totals[3]):.2%})" if puct else "-"
            row = f"| {name} | {n} | {w} | {p:.2%} | {se:.2%} | {share} |"
            print(row, flush=True)
            games.append(row)
        d = rates[True][0] - rates[False][0]
        se = math.hypot(rates[True][1], rates[False][1])
        verdict = (f"PUCT - guided = {d:+.2%}, {abs(d) / se:.1f} standard errors of the difference ({se:.2%}): "
                   + ("PUCT is ahead by more than two." if d > 2 * se else "PUCT is NOT ahead by more than two standard errors."))
        print(verdict)
        games.append("")
        games.append(verdict)
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("# Guided PUCT (search spec v5) against guided UCT (spec v3): step time and playing strength\n\n"
                    f"`python tools/puct_probe.py --budget {a.budget} --trees {a.trees} --playouts {a.playouts} --tables {a.tables} "
                    f"--iterations {a.iterations} --c {a.c} --plies {a.plies}`: one process.  Step: HIP events, medians [min-max] over "
                    f"the steps {a.skip} .. {a.budget - 1} of one search, values and weights drawn once per item.  Match: the lord at "
                    f"{a.trees} x {a.budget} iterations, PlayoutLeaf({a.playouts}), hands sampled, against the rule farmers.\n\n"
                    + "\n".join(steps) + "\n\n" + "\n".join(games) + "\n")


if __name__ == "__main__":
    main()
