#!/usr/bin/env python3
"""Information-set MCTS (ddz_ismcts, csrc/ddz_ismcts.h: k_ismcts) against its yardstick, the determinized UCT search
(ddz_search, hidden form: k_search<true>), in ONE process, the two alternated call by call on the same tables with the same
budget and trees:

  device time per iteration (ms / totals[1]) of both and their ratio, at 1, 64 and 4,096 tables, for one deep tree
  (--budget iterations) and for --trees trees of budget / trees,
  the mean descent depth of both: nodes below the root on an iteration's path, the created one included.  Every iteration
  adds 1 to V of every node of its path, so depth = (sum of V over the node records - iterations) / iterations, read from
  the workspace cached on the env (zeroed before the call so that records never written count nothing).  k_ismcts enumerates
  one list per level of that depth where k_search enumerates one per iteration: the ratio is expected to grow with it,
  the workspace bytes per tree of both at budgets 64 / 1000 / 4096.

Device time = HIP events around the call on the current stream (the memsets included), after a warm-up call of each; every
figure is the median [min-max] of --reps calls.  The tables are --plies random plies into their games.

  python tools/ismcts_probe.py [--reps 3] [--plies 12] [--budget 1024] [--trees 16] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from search_probe import make_env, timed_alternating  # noqa: E402  (the same directory)

RECORD = {"_ismcts_work": 32, "_search_work": 24}      # bytes of a node record; V is the u32 at offset 8 of both


def depth(env, attr, call, budget, trees, totals):
    """mean nodes below the root on a path, of the trees `call` builds in the workspace `attr`"""
    call()                                               # (the workspace exists)
    getattr(env, attr).zero_()
    totals.zero_()
    call()
    torch.cuda.synchronize()
    iterations = int(totals[1].item())
    rec = RECORD[attr]
    table_log = 1
    while (1 << table_log) < 2 * (budget + 1):
        table_log += 1
    nodes_bytes = (budget + 1) * rec
    if rec == 24:
        nodes_bytes = (nodes_bytes + 15) & ~15
    tree_bytes = nodes_bytes + (8 << table_log)
    work = getattr(env, attr)[:env.T * trees * tree_bytes].view(env.T * trees, tree_bytes)
    nodes = work[:, :(budget + 1) * rec].contiguous().view(torch.int32).view(env.T * trees, budget + 1, rec // 4)
    v = int(nodes[:, :, 2].to(torch.int64).sum().item())
    return (v - iterations) / max(1, iterations), totals.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--budget", type=int, default=1024)
    ap.add_argument("--trees", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    res = {"rows": [], "workspace": [], "reps": a.reps, "plies": a.plies}
    totals = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    for T in (1, 64, 4096):
        env = make_env(pkg, T, a.plies)
        visits = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        wins = torch.empty(T * env.slab_stride, dtype=torch.int32, device="cuda:0")
        for budget, trees in ((a.budget, 1), (max(1, a.budget // a.trees), a.trees)):
            kw = dict(trees=trees, visits=visits, wins=wins, totals=totals)

            def ism():
                env.ismcts(budget, **kw)

            def uct():
                env.search(budget, hidden=True, **kw)

            d_i, t_i = depth(env, "_ismcts_work", ism, budget, trees, totals)
            d_u, t_u = depth(env, "_search_work", uct, budget, trees, totals)
            (im, ilo, ihi), (um, ulo, uhi) = timed_alternating([ism, uct], a.reps)
            row = {"tables": T, "budget": budget, "trees": trees,
                   "ismcts": {"moves": t_i[0], "iterations": t_i[1], "unfinished": t_i[2], "nodes": t_i[3], "depth": d_i,
                              "ms": im, "ms_min": ilo, "ms_max": ihi, "us_per_iteration": im * 1e3 / max(1, t_i[1])},
                   "uct": {"moves": t_u[0], "iterations": t_u[1], "unfinished": t_u[2], "nodes": t_u[3], "depth": d_u,
                           "ms": um, "ms_min": ulo, "ms_max": uhi, "us_per_iteration": um * 1e3 / max(1, t_u[1])}}
            row["time_ratio"] = im / um
            res["rows"].append(row)
            print(f"T={T:5d} {trees:3d} x {budget:5d}  ismcts {t_i[1]:9d} it depth {d_i:6.2f} nodes {t_i[3]:9d} {im:10.3f} ms "
                  f"[{ilo:.3f}-{ihi:.3f}] | uct(hidden) depth {d_u:6.2f} nodes {t_u[3]:9d} {um:10.3f} ms [{ulo:.3f}-{uhi:.3f}] | "
                  f"ismcts / uct {row['time_ratio']:.3f}")
        assert env.status() == 0
        del env
    env = make_env(pkg, 1, 0)
    for budget in (64, 1000, 4096):
        bi, bu = int(env.lib.ddz_ismcts_work_bytes(1, budget, 1)), int(env.lib.ddz_search_work_bytes(1, budget, 1))
        res["workspace"].append({"budget": budget, "ismcts_bytes_per_tree": bi, "uct_bytes_per_tree": bu})
        print(f"workspace: budget {budget:5d}: ismcts {bi} bytes per tree, uct {bu}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
