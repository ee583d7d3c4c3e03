#!/usr/bin/env python3
"""The UCT tree search (ddz_search, csrc/ddz_search.h: k_search) against its yardstick, the flat playout evaluator
(ddz_playout: k_playout), in ONE process, the two alternated call by call:

  search iterations per second (totals[1] / device time) at 1, 64 and 4,096 tables with --budget 1000 iterations per tree,
  a sweep of `trees` at every table count,
  beside each row BatchedEnv.playout at an EQUAL number of playouts: K = round(budget * trees / mean list size), so that
  n * K ~ budget * trees per table; playouts per second of both and their ratio,
  the workspace bytes per tree at budgets 64 / 1000 / 4096.

An iteration is one playout plus the descent to it: re-applied moves, the selection's table probes and node reads (global
memory latency that a flat playout does not pay) and the backup.  Device time = HIP events around the call on the current
stream (the memsets included), after a warm-up call of each; every figure is the median [min-max] of --reps calls.  The
tables are --plies random plies into their games, as in tools/playout_probe.py.

  python tools/search_probe.py [--reps 5] [--plies 12] [--budget 1000] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_alternating(fns, reps):
    """ms per call of every fn of `fns`, by events, after one warm-up call each, the fns taking turns: [(median, min, max)]"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b))
    return [(statistics.median(x), min(x), max(x)) for x in out]


def make_env(pkg, T, plies, seed=3):
    env = pkg.BatchedEnv(T, seed=seed, device="cuda:0")
    env.reset()
    if plies:
        env.rollout_random(plies)
    env.legal_slab()
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--budget", type=int, default=1000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    res = {"rows": [], "workspace": [], "reps": a.reps, "plies": a.plies, "budget": a.budget}
    totals = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    for T, sweep in ((1, (1, 16, 64, 256, 1024, 6144)), (64, (1, 4, 16, 96)), (4096, (1, 2, 4))):
        env = make_env(pkg, T, a.plies)
        n = env.counts.float()
        running = n > 0
        mean_n = n[running].mean().item()
        visits = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        wins = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        for trees in sweep:
            K = max(1, round(a.budget * trees / mean_n))
            totals.zero_()
            env.search(a.budget, trees=trees, visits=visits, wins=wins, totals=totals)
            s_tot = totals.tolist()
            totals.zero_()
            env.playout(K, wins=wins, totals=totals)
            p_tot = totals.tolist()
            (sm, slo, shi), (pm, plo, phi) = timed_alternating(
                [lambda: env.search(a.budget, trees=trees, visits=visits, wins=wins), lambda: env.playout(K, wins=wins)], a.reps)
            row = {"tables": T, "trees": trees, "mean_list": mean_n, "K": K,
                   "search": {"moves": s_tot[0], "iterations": s_tot[1], "unfinished": s_tot[2], "nodes": s_tot[3], "ms": sm,
                              "ms_min": slo, "ms_max": shi, "iterations_per_s": s_tot[1] / sm * 1e3},
                   "playout": {"moves": p_tot[0], "playouts": p_tot[1], "ms": pm, "ms_min": plo, "ms_max": phi,
                               "playouts_per_s": p_tot[1] / pm * 1e3}}
            row["rate_ratio"] = row["search"]["iterations_per_s"] / row["playout"]["playouts_per_s"]
            res["rows"].append(row)
            print(f"T={T:5d} trees={trees:5d}  search {s_tot[1]:10d} it {s_tot[0]:12d} moves {sm:10.3f} ms [{slo:.3f}-{shi:.3f}] "
                  f"{row['search']['iterations_per_s'] / 1e6:8.3f} M it/s | playout K={K:5d} {p_tot[1]:10d} playouts "
                  f"{pm:10.3f} ms [{plo:.3f}-{phi:.3f}] {row['playout']['playouts_per_s'] / 1e6:8.3f} M playouts/s | "
                  f"search / playout {row['rate_ratio']:.3f}")
        assert env.status() == 0
        del env
    env = make_env(pkg, 1, 0)
    for budget in (64, 1000, 4096):
        b = int(env.lib.ddz_search_work_bytes(1, budget, 1))
        res["workspace"].append({"budget": budget, "bytes_per_tree": b})
        print(f"workspace: budget {budget:5d}: {b} bytes per tree")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
