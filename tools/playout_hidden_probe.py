#!/usr/bin/env python3
"""Hidden-hand playouts (ddz_playout_hidden, csrc/ddz_playout.h: k_playout<true>) against their yardstick, the open form
(ddz_playout: k_playout<false>), in ONE process, the two forms alternated call by call:

  playout moves per second (totals[0] / device time) at 4,096 and 65,536 tables for K = 8 and 64 playouts per move,
  the single-table call (the lord's first lead, K = 64),
  ddz_playout_worlds alone (K worlds per table), for what the redeal costs on its own.

Device time = HIP events around the call on the current stream (the memset of `wins` included), after a warm-up call of
each form; every figure is the median [min-max] of --reps calls.  The tables are --plies random plies into their games, as
in tools/playout_probe.py.  Both forms run the same number of playouts (the lists are the same); the moves differ, because
the hidden form plays on other hands.

  python tools/playout_hidden_probe.py [--reps 5] [--plies 12] [--json out.json]
  python tools/playout_hidden_probe.py --parent-lib PATH   # the OPEN form alone on another build of the library (one of
      the parent commit: its sample spread is the yardstick of the open form here; the hidden entry points are not looked up)
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    forms = ("open", "hidden")
    if a.parent_lib:
        lib = importlib.import_module("doudizhu-rl_amd._lib")
        for name in ("ddz_playout_hidden", "ddz_playout_worlds"):
            lib.SYMBOLS.pop(name)
        lib.use_library(os.path.abspath(a.parent_lib))
        forms = ("open",)
    pkg = importlib.import_module("doudizhu-rl_amd")
    res = {"rows": [], "worlds": [], "reps": a.reps, "plies": a.plies, "lib": a.parent_lib or "this build"}
    totals = torch.zeros(4, dtype=torch.int64, device="cuda:0")

    def measure(env, T, K, chunks=None, label=""):
        wins = torch.empty(env.T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        moves = {}
        for f in forms:
            totals.zero_()
            env.playout(K, totals=totals, chunks=chunks, wins=wins, **({"hidden": True} if f == "hidden" else {}))
            moves[f] = totals.tolist()
        fns = [(lambda f=f: env.playout(K, chunks=chunks, wins=wins, **({"hidden": True} if f == "hidden" else {}))) for f in forms]
        times = timed_alternating(fns, a.reps)
        row = {"tables": T, "K": K, "label": label}
        for f, (med, lo, hi) in zip(forms, times):
            row[f] = {"moves": moves[f][0], "playouts": moves[f][1], "unfinished": moves[f][2], "ms": med, "ms_min": lo,
                      "ms_max": hi, "moves_per_s": moves[f][0] / med * 1e3}
            print(f"{f:6s} T={T:6d} K={K:3d} {label} {moves[f][0]:12d} moves {moves[f][1]:10d} playouts  {med:9.3f} ms "
                  f"[{lo:.3f}-{hi:.3f}]  {row[f]['moves_per_s'] / 1e9:.3f} G moves/s")
        if len(forms) == 2:
            row["ms_ratio"] = row["hidden"]["ms"] / row["open"]["ms"]
            row["rate_ratio"] = row["hidden"]["moves_per_s"] / row["open"]["moves_per_s"]
            print(f"       hidden / open: time {row['ms_ratio']:.3f}, moves per second {row['rate_ratio']:.3f}")
        res["rows"].append(row)

    for T in (4096, 65536):
        env = make_env(pkg, T, a.plies)
        for K in (8, 64):
            measure(env, T, K)
        if len(forms) == 2:
            for K in (8, 64):
                (med, lo, hi), = timed_alternating([lambda: env.playout_worlds(K)], a.reps)
                res["worlds"].append({"tables": T, "K": K, "ms": med, "ms_min": lo, "ms_max": hi, "worlds_per_s": T * K / med * 1e3})
                print(f"worlds T={T:6d} K={K:3d}  {med:9.3f} ms [{lo:.3f}-{hi:.3f}]  {T * K / med / 1e6:.3f} G worlds/s")
        assert env.status() == 0
        del env
    env = make_env(pkg, 1, 0)                      # one table, the lord's first lead
    measure(env, 1, 64, label=f"list={int(env.counts[0])}")
    env = make_env(pkg, 1, a.plies)
    measure(env, 1, 64, label=f"list={int(env.counts[0])}")
    assert env.status() == 0
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
