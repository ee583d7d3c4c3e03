#!/usr/bin/env python3
"""The CFR endgame solver (ddz_cfr, csrc/ddz_cfr.h: k_cfr) timed: milliseconds per launch of BatchedEnv.cfr(8) for

  1, 64 and 4,096 copies of the worst case the capacity sweep found (tools/cfr_sweep.py: 4 5 6 7 and both jokers dealt 2/2/2,
  the lord facing a single 3: 90 deals, 10,512 nodes, 2,835 information sets), and
  up to 4,096 endgames reached by random play: --tables games are played with uniformly random moves and a table is taken
  the first time its three hands hold 6 cards or fewer.

Device time = HIP events around the call on the current stream (the head's zeroing included), after a warm-up call; every figure is
the median [min-max] of --reps calls.  Also printed: the forest sizes (totals) and the workspace per slot.

  python tools/cfr_probe.py [--reps 5] [--iterations 8] [--tables 65536] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def worst_case():
    """uint8 [11, 16]: the lord (role 1) holds 4 and the black joker; 5 6 7 and the red joker are out; up (role 0) led a 3"""
    s = np.zeros((11, 16), np.uint8)
    s[1, [1, 13]] = 1                          # the lord's hand: 4, BJ
    s[0, 15] = s[1, 15] = s[2, 15] = 2         # cards left
    taken = np.array([4] * 13 + [1, 1], np.uint8)
    taken[[1, 2, 3, 4, 13, 14]] -= 1
    s[9, :15] = taken
    s[3, :15] = taken                          # (histories: not read)
    s[6, 0], s[6, 15] = 1, 1                   # up's recent row: a single 3
    s[10, 0], s[10, 2], s[10, 6] = 1, 0xFF, 1
    return s


def timed(fn, reps):
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


def random_endgames(pkg, tables, want, seed=3):
    """up to `want` states uint8 [n, 11, 16] of games under random play, each at the first ply with 6 cards or fewer"""
    env = pkg.BatchedEnv(tables, seed=seed, device="cuda:0")
    env.reset()
    env.legal_slab()
    taken = torch.zeros(tables, dtype=torch.bool, device="cuda:0")
    out, n = [], 0
    for _ in range(170):
        st = env.state.view(tables, 11, 16)
        left = st[:, 0:3, 15].to(torch.int32)
        hit = (st[:, 10, 1] == 0) & (left.sum(1) <= 6) & (left.min(1).values >= 1) & ~taken
        if hit.any():
            out.append(st[hit].clone())
            taken |= hit
            n += int(hit.sum())
            if n >= want:
                break
        env.step_slab(mode=pkg.STEP_RANDOM, auto_reset=False)
    return torch.cat(out)[:want].cpu().numpy() if out else np.zeros((0, 11, 16), np.uint8)


def measure(pkg, states, iterations, reps, label, res):
    T = len(states)
    env = pkg.BatchedEnv(T, seed=1, device="cuda:0")
    env.state_import(torch.from_numpy(np.ascontiguousarray(states).reshape(-1)))
    totals = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    out = env.cfr(iterations, slots=T, totals=totals)
    torch.cuda.synchronize()
    n = out[0].cpu().numpy()
    tot = totals.tolist()
    assert env.status() == 0 and (n > 0).all(), (env.status(), np.unique(n))
    med, lo, hi = timed(lambda: env.cfr(iterations, slots=T, out=out), reps)
    row = {"case": label, "tables": T, "iterations": iterations, "deals": tot[0], "nodes": tot[1], "infosets": tot[2],
           "pairs": tot[3], "ms": med, "ms_min": lo, "ms_max": hi, "nodes_per_table": tot[1] / T}
    res["rows"].append(row)
    print(f"{label:28s} T={T:5d}  {med:9.3f} ms [{lo:.3f}-{hi:.3f}]  {tot[1] / T:9.1f} nodes/table  {tot[2] / T:8.1f} sets/table  "
          f"{tot[1] * iterations / med / 1e6:8.2f} G node-iterations/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--tables", type=int, default=65536)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    res = {"rows": [], "reps": a.reps}
    for T in (1, 64, 4096):
        measure(pkg, np.repeat(worst_case()[None], T, 0), a.iterations, a.reps, "worst case", res)
    st = random_endgames(pkg, a.tables, 4096)
    if len(st):
        measure(pkg, st, a.iterations, a.reps, f"random play ({a.tables} games)", res)
    lib = importlib.import_module("doudizhu-rl_amd._lib").lib()
    res["slot_bytes"] = int(lib.ddz_cfr_work_bytes(2) - lib.ddz_cfr_work_bytes(1))
    print(f"workspace: {res['slot_bytes']} bytes per slot")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
