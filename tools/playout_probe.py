#!/usr/bin/env python3
"""Playout evaluator (ddz_playout, csrc/ddz_playout.h) against its yardstick, ddz_rollout_random, in ONE process:

  playout moves per second (totals[0] / device time) at 1, 64, 4,096 and 65,536 tables for K = 8 and 64 playouts per move,
  rollout_random env steps per second at 4,096 and 65,536 tables (the same list work per ply, plus the list stores),
  the time of one call on ONE table as `chunks` grows.

Device time = HIP events around the call on the current stream (the memset of `wins` included), after a warm-up call of the
same shape; every figure is the median [min-max] of --reps calls.  The tables are --plies random plies into their games
(mid-game lists; the fresh 20-card lead of every table at once is the costliest root there is), idle tables re-dealt.

  python tools/playout_probe.py [--reps 5] [--plies 12] [--budget-ms 1500] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """ms per call of fn(), by events, after one warm-up call: (median, min, max)"""
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
    ap.add_argument("--budget-ms", type=float, default=1500.0, help="skip a (tables, K) whose predicted call is longer")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    res = {"playout": [], "rollout": [], "chunks": [], "reps": a.reps, "plies": a.plies}
    totals = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    rate = None                                   # moves per ms of the last measured shape: predicts the next one
    for T in (1, 64, 4096, 65536):
        env = make_env(pkg, T, a.plies)
        moves_per_k = None
        for K in (8, 64):
            if rate and moves_per_k and moves_per_k * K / rate > a.budget_ms:
                print(f"playout  T={T:6d} K={K:3d}  skipped: predicted {moves_per_k * K / rate:.0f} ms > --budget-ms")
                continue
            totals.zero_()
            env.playout(K, totals=totals)
            moves, runs, unfinished, _ = totals.tolist()
            moves_per_k = moves / K
            med, lo, hi = timed(lambda: env.playout(K), a.reps)
            rate = moves / med
            row = {"tables": T, "K": K, "moves": moves, "playouts": runs, "unfinished": unfinished, "ms": med, "ms_min": lo,
                   "ms_max": hi, "moves_per_s": moves / med * 1e3}
            res["playout"].append(row)
            print(f"playout  T={T:6d} K={K:3d}  {moves:12d} moves {runs:10d} playouts  {med:9.3f} ms [{lo:.3f}-{hi:.3f}]  "
                  f"{row['moves_per_s'] / 1e9:.3f} G moves/s")
        if T >= 4096:
            iters = 256
            med, lo, hi = timed(lambda: env.rollout_random(iters), a.reps)
            row = {"tables": T, "iters": iters, "ms": med, "ms_min": lo, "ms_max": hi, "steps_per_s": T * iters / med * 1e3}
            res["rollout"].append(row)
            print(f"rollout  T={T:6d} {iters} iterations  {med:9.3f} ms [{lo:.3f}-{hi:.3f}]  {row['steps_per_s'] / 1e9:.3f} G steps/s")
        del env
    env = make_env(pkg, 1, 0)                      # one table, the lord's first lead: the longest list there is
    K = 64
    for chunks in (1, 8, 64, 512, 4096, 8192):
        totals.zero_()
        env.playout(K, chunks=chunks, totals=totals)
        moves = totals.tolist()[0]
        med, lo, hi = timed(lambda: env.playout(K, chunks=chunks), a.reps)
        row = {"tables": 1, "K": K, "chunks": chunks, "moves": moves, "ms": med, "ms_min": lo, "ms_max": hi,
               "moves_per_s": moves / med * 1e3}
        res["chunks"].append(row)
        print(f"chunks   T=1 K={K} list={int(env.counts[0])} chunks={chunks:5d}  {med:9.3f} ms [{lo:.3f}-{hi:.3f}]  "
              f"{row['moves_per_s'] / 1e6:.1f} M moves/s")
    assert env.status() == 0
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
