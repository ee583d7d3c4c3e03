#!/usr/bin/env python3
"""The exact endgame solver (ddz_solve, csrc/ddz_solve.h: k_solve) timed on endings reached by random play.

For every card threshold N of --cards (default 9 12 15) and every table count of --tables (default 4096 65536): games are
played with uniformly random moves and a table is taken the first time its three hands together hold N cards or fewer; then
BatchedEnv.solve(max_cards=N) is timed at the default budget and table size.  Printed per row: milliseconds per launch,
positions / s, nodes / s, nodes per position, the share of root moves and of positions left unknown; then, at the first table
count, the effect of tt_entries (--tt) and of chunks, and for scale BatchedEnv.search(1000) on the same positions.

Device time = HIP events around the call on the current stream (the two memsets included), after a call with budget 1 that
allocates the workspace; the median [min-max] of --reps calls (one call where a single launch takes seconds).

  python tools/solve_probe.py [--reps 3] [--cards 9 12 15] [--tables 4096 65536] [--tt 64 1024 4096 16384] [--json out.json]
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
DEV = "cuda:0"


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
        if out[-1] > 2000.0:
            break                       # seconds per launch: one call says enough
    return statistics.median(out), min(out), max(out)


def endings(pkg, want, max_cards, seed=7):
    """`want` states uint8 [want, 11, 16] of games under random play, each at the first ply with max_cards cards or fewer"""
    out, n, rnd = [], 0, 0
    games = min(max(want, 4096), 65536)
    while n < want and rnd < 8:
        env = pkg.BatchedEnv(games, seed=seed + rnd, device=DEV)
        env.reset()
        env.legal_slab()
        taken = torch.zeros(games, dtype=torch.bool, device=DEV)
        for _ in range(170):
            st = env.state.view(games, 11, 16)
            cards = st[:, 0:3, :15].to(torch.int32).sum((1, 2))
            hit = (st[:, 10, 1] == 0) & (st[:, 10, 6] != 0) & (cards <= max_cards) & ~taken
            if hit.any():
                out.append(st[hit].clone())
                taken |= hit
                n += int(hit.sum())
            env.step_slab(mode=pkg.STEP_RANDOM, auto_reset=False)
        rnd += 1
        env.close()
    return torch.cat(out)[:want].contiguous()


def solve_row(env, label, reps, res, **kw):
    T = env.T
    totals = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = env.solve(budget=1, **kw)                       # allocates the workspace and the outputs
    out = tuple(x.view(-1) for x in out)
    torch.cuda.synchronize()
    env.solve(totals=totals, out=out, **kw)
    torch.cuda.synchronize()
    n = out[0].cpu().numpy()
    nodes, hits, solved, unknown = totals.tolist()
    assert env.status() == 0 and (n > 0).all(), (env.status(), np.unique(n))
    unk_tables = int((out[2].view(T, -1).sum(1) > 0).sum())
    med, lo, hi = timed(lambda: env.solve(out=out, **kw), reps)
    row = {"case": label, "tables": T, "ms": med, "ms_min": lo, "ms_max": hi, "nodes": nodes, "hits": hits, "moves": solved + unknown,
           "moves_unknown": unknown, "tables_unknown": unk_tables, **{k: v for k, v in kw.items()}}
    res["rows"].append(row)
    print(f"{label:34s} T={T:6d} {med:10.3f} ms [{lo:.3f}-{hi:.3f}] {T / med * 1e3:12.0f} positions/s {nodes / med / 1e3:9.2f} M nodes/s "
          f"{nodes / T:10.1f} nodes/position  hits {hits / max(nodes, 1):.3f}  unknown {unknown / max(solved + unknown, 1):.5f} of moves, "
          f"{unk_tables / T:.5f} of positions", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cards", type=int, nargs="+", default=[9, 12, 15])
    ap.add_argument("--tables", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--tt", type=int, nargs="+", default=[64, 1024, 4096, 16384])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    res = {"rows": [], "reps": a.reps}
    for N in a.cards:
        st = endings(pkg, max(a.tables), N)
        for T in a.tables:
            if len(st) < T:
                print(f"only {len(st)} endings of {N} cards or fewer: T={T} skipped")
                continue
            env = pkg.BatchedEnv(T, seed=1, device=DEV)
            env.state_import(st[:T].reshape(-1))
            solve_row(env, f"<= {N} cards, defaults", a.reps, res, max_cards=N)
            if T == a.tables[0]:
                for tt in a.tt:
                    if tt != 4096:
                        solve_row(env, f"<= {N} cards, tt_entries={tt}", a.reps, res, max_cards=N, tt_entries=tt)
                solve_row(env, f"<= {N} cards, chunks=4", a.reps, res, max_cards=N, chunks=4)
            env._solve_work = None                        # (the next row's workspace is another size)
            env.search(1000)
            torch.cuda.synchronize()
            med, lo, hi = timed(lambda: env.search(1000), a.reps)
            res["rows"].append({"case": f"search(1000), <= {N} cards", "tables": T, "ms": med, "ms_min": lo, "ms_max": hi})
            print(f"{'search(1000) on the same positions':34s} T={T:6d} {med:10.3f} ms [{lo:.3f}-{hi:.3f}] {T / med * 1e3:12.0f} positions/s",
                  flush=True)
            env.close()
            del env
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
