#!/usr/bin/env python3
"""Flat Monte Carlo on the batched engine: a lord that plays the move with the most playout wins (BatchedEnv.playout_choose:
every legal move followed by --playouts uniformly random playouts over the three known hands, the reference's Monte-Carlo
player of server/mcts/interface.py:15-45 without its tree) against random farmers -- beside a lord that plays at random like
them.  Prints both win rates from env.stats().

  python examples/flat_mc.py [--tables 1024] [--playouts 16] [--iterations 400] [--seed 0] [--hidden] [--match]
  python examples/flat_mc.py --search BUDGET [--trees 1] [--mode reference] [--tables 256] [--iterations 200]
  python examples/flat_mc.py --ismcts BUDGET [--trees 1] [--uct-trees 16] [--mode reference] [--tables 256] [--iterations 200]
  python examples/flat_mc.py --guided BUDGET [--leaf playout|q] [--leaf-playouts 4] [--trees 4] [--tables 256] [--iterations 200]
  python examples/flat_mc.py --guided-ismcts BUDGET [--leaf playout|q] [--leaf-playouts 4] [--trees 1] [--uct-trees 4] [--tables 256]
  python examples/flat_mc.py --guided-puct BUDGET [--leaf playout|q] [--leaf-playouts 4] [--trees 4] [--c 1.25] [--tables 256]

--hidden: the playouts do not read the farmers' hands; they run on hands dealt anew, per playout number, from the cards the
lord has not seen (playout spec v2, BatchedEnv.playout_choose(hidden=True, roles=0b010): only the lord's tables are
evaluated).  This is the evaluation a seat may use: the open form looks at the opponents' cards.
--match: the hidden-playout lord against the RULE farmers (env.auto_choose(0b101)) instead of random ones: the two id vectors
are merged with torch.where and stepped with step_slab(STEP_IDS); the win counts come from env.stats().  The win rate this
prints has not been measured anywhere in this repository's notes: quote it only with that said.

--search BUDGET: a UCT lord (BatchedEnv.search_choose: --trees trees of BUDGET iterations, search spec v1) against flat
Monte-Carlo farmers at an EQUAL number of playouts per decision -- the farmers' playouts per move are BUDGET * trees divided by
the mean size of their lists on that iteration -- and, as the yardstick, the same match with a flat Monte-Carlo lord given the
same number.  Both seats see all three hands.  Printed as the lord's win rate in both matches.

--ismcts BUDGET: an information-set MCTS lord (BatchedEnv.ismcts_choose: --trees trees of BUDGET iterations, every iteration
on a fresh deal of the cards the lord has not seen, search spec v2) against the RULE farmers (env.auto_choose(0b101)) -- beside
a determinized-UCT lord (search_choose(hidden=True)) with the same total iterations per move split over --uct-trees worlds, for
example 1 x 1024 against 16 x 64.  Neither lord reads the farmers' hands; only the lord's tables are searched (roles=0b010).

--guided BUDGET: a guided-UCT lord (BatchedEnv.guided_choose, search spec v3: --trees trees of BUDGET iterations on sampled
hands, one launch per iteration, every new leaf judged by --leaf: `playout` = engine.PlayoutLeaf(--leaf-playouts), `q` =
dqn_glue.QLeaf on an UNTRAINED network of face variant 3 for every role, which is not expected to win) against the RULE farmers
-- beside the determinized-UCT lord of search_choose(hidden=True) at the same budget and trees against the same farmers.  The
win rates are printed with their game counts; nothing in this repository's notes has measured them.

--guided-ismcts BUDGET: a guided-ISMCTS lord (BatchedEnv.guided_ismcts_choose, search spec v4: --trees trees of BUDGET
iterations, every iteration on a fresh deal of the cards the lord has not seen, one launch per iteration, every new leaf judged
by --leaf as above) against the RULE farmers -- beside a guided-UCT lord with the same evaluator and the same total iterations
per move split over --uct-trees worlds, and an ISMCTS lord (random playouts) at the same trees and budget, for example 1 x 256
against 4 x 64 and 1 x 256.  Printed with their game counts; one run is an observation, not a measurement.

--guided-puct BUDGET: a guided-PUCT lord (BatchedEnv.guided_puct_choose, search spec v5: --trees trees of BUDGET iterations on
sampled hands, one launch per iteration, every new node judged by --leaf, which also hands back a prior weight for each of
the node's moves; selection over all moves by mean + c * prior * sqrt(N) / (1 + visits), the move with the most visits is
played) against the RULE farmers -- beside a guided-UCT lord (mode "sides") with the same evaluator, budget and trees.  Printed
with their game counts; one run is an observation, not a measurement (tools/puct_probe.py measures).

The playouts are computed for every table on every iteration and used where the lord is to move (the other tables take -1 =
the engine's random move): simple, and three times the work a loop that asks only for the lord's tables would do.
"""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rates(s):
    e = max(1, s["episodes"])
    return f"{s['episodes']} episodes: lord {s['lord_wins'] / e:.1%}, farmers {(s['up_wins'] + s['down_wins']) / e:.1%}"


def seat_match(pkg, a, dev, uct):
    """the lord by UCT (uct=True) or by flat Monte Carlo, the farmers by flat Monte Carlo, at budget * trees playouts a move"""
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    lord = torch.empty(a.tables, dtype=torch.int32, device=dev)
    farm = torch.empty(a.tables, dtype=torch.int32, device=dev)
    per_move = a.search * a.trees
    for it in range(a.iterations):
        counts = env.legal_slab()[0]
        is_lord = env.role == 1
        n_farm = counts[~is_lord].float().mean().item() if (~is_lord).any().item() else 1.0
        n_lord = counts[is_lord].float().mean().item() if is_lord.any().item() else 1.0
        if uct:
            env.search_choose(a.search, trees=a.trees, mode=a.mode, salt=it, out=lord)
        else:
            env.playout_choose(max(1, round(per_move / max(n_lord, 1.0))), salt=it, out=lord)
        env.playout_choose(max(1, round(per_move / max(n_farm, 1.0))), salt=it + (1 << 20), out=farm)
        env.step_slab(torch.where(is_lord, lord, farm), pkg.STEP_IDS, auto_reset=True)
    assert env.status() == 0
    return env.stats()


def hidden_match(pkg, a, dev, ismcts):
    """the lord by ISMCTS (ismcts=True: trees x budget) or by determinized UCT (uct_trees x the same total / uct_trees), both
    on sampled hands; the farmers by the rule agent"""
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    lord = torch.empty(a.tables, dtype=torch.int32, device=dev)
    uct_budget = max(1, a.ismcts * a.trees // a.uct_trees)
    for it in range(a.iterations):
        if ismcts:
            env.ismcts_choose(a.ismcts, trees=a.trees, mode=a.mode, salt=it, roles=0b010, out=lord)
        else:
            env.search_choose(uct_budget, trees=a.uct_trees, mode=a.mode, salt=it, hidden=True, roles=0b010, out=lord)
        env.step_slab(torch.where(env.role == 1, lord, env.auto_choose(0b101)), pkg.STEP_IDS, auto_reset=True)
    assert env.status() == 0
    return env.stats()


def make_leaf(pkg, a, dev):
    """--leaf: engine.PlayoutLeaf(--leaf-playouts), or dqn_glue.QLeaf on one untrained network for the three roles"""
    if a.leaf == "q":
        torch.manual_seed(a.seed)
        net = pkg.dqn_glue.QNet(pkg.FACE_PLANES[3]).to(dev).eval()
        return pkg.QLeaf({"lord": net, "down": net, "up": net}, 3)
    return pkg.PlayoutLeaf(a.leaf_playouts)


def guided_ismcts_match(pkg, a, dev, lord_kind):
    """the lord by guided ISMCTS ("v4": trees x budget), by guided UCT ("v3": uct_trees x the same total / uct_trees, the same
    evaluator) or by ISMCTS with its random playout ("v2": trees x budget), all on sampled hands; the farmers by the rule agent"""
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    lord = torch.empty(a.tables, dtype=torch.int32, device=dev)
    leaf = make_leaf(pkg, a, dev)
    uct_budget = max(1, a.guided_ismcts * a.trees // a.uct_trees)
    for it in range(a.iterations):
        leaf.salt = it
        if lord_kind == "v4":
            env.guided_ismcts_choose(leaf, a.guided_ismcts, trees=a.trees, mode=a.mode, salt=it, roles=0b010, out=lord)
        elif lord_kind == "v3":
            env.guided_choose(leaf, uct_budget, trees=a.uct_trees, mode=a.mode, salt=it, hidden=True, roles=0b010, out=lord)
        else:
            env.ismcts_choose(a.guided_ismcts, trees=a.trees, mode=a.mode, salt=it, roles=0b010, out=lord)
        env.step_slab(torch.where(env.role == 1, lord, env.auto_choose(0b101)), pkg.STEP_IDS, auto_reset=True)
    assert env.status() == 0
    return env.stats()


def guided_puct_match(pkg, a, dev, puct):
    """the lord by guided PUCT (puct=True) or by guided UCT with the "sides" rule at the same budget and trees, the same
    evaluator, both on sampled hands; the farmers by the rule agent"""
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    lord = torch.empty(a.tables, dtype=torch.int32, device=dev)
    leaf = make_leaf(pkg, a, dev)
    for it in range(a.iterations):
        leaf.salt = it
        if puct:
            env.guided_puct_choose(leaf, a.guided_puct, trees=a.trees, c=a.c, salt=it, hidden=True, roles=0b010, out=lord)
        else:
            env.guided_choose(leaf, a.guided_puct, trees=a.trees, mode="sides", salt=it, hidden=True, roles=0b010, out=lord)
        env.step_slab(torch.where(env.role == 1, lord, env.auto_choose(0b101)), pkg.STEP_IDS, auto_reset=True)
    assert env.status() == 0
    return env.stats()


def guided_match(pkg, a, dev, guided):
    """the lord by guided UCT (guided=True) or by determinized UCT at the same budget and trees, both on sampled hands; the
    farmers by the rule agent"""
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    lord = torch.empty(a.tables, dtype=torch.int32, device=dev)
    leaf = make_leaf(pkg, a, dev)
    for it in range(a.iterations):
        if guided:
            leaf.salt = it
            env.guided_choose(leaf, a.guided, trees=a.trees, mode=a.mode, salt=it, hidden=True, roles=0b010, out=lord)
        else:
            env.search_choose(a.guided, trees=a.trees, mode=a.mode, salt=it, hidden=True, roles=0b010, out=lord)
        env.step_slab(torch.where(env.role == 1, lord, env.auto_choose(0b101)), pkg.STEP_IDS, auto_reset=True)
    assert env.status() == 0
    return env.stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hidden", action="store_true", help="sample the farmers' hands per playout instead of reading them")
    ap.add_argument("--match", action="store_true", help="a hidden-playout lord against the rule farmers")
    ap.add_argument("--search", type=int, default=0, metavar="BUDGET", help="a UCT lord against flat Monte-Carlo farmers")
    ap.add_argument("--ismcts", type=int, default=0, metavar="BUDGET", help="an ISMCTS lord against the rule farmers")
    ap.add_argument("--guided", type=int, default=0, metavar="BUDGET", help="a guided-UCT lord against the rule farmers")
    ap.add_argument("--guided-ismcts", type=int, default=0, metavar="BUDGET", help="a guided-ISMCTS lord against the rule farmers")
    ap.add_argument("--guided-puct", type=int, default=0, metavar="BUDGET", help="a guided-PUCT lord against the rule farmers")
    ap.add_argument("--c", type=float, default=1.25, help="--guided-puct: the exploration constant")
    ap.add_argument("--leaf", default="playout", choices=("playout", "q"), help="--guided / --guided-ismcts / --guided-puct: the leaf evaluator")
    ap.add_argument("--leaf-playouts", type=int, default=4, help="--guided --leaf playout: playouts per move of a leaf")
    ap.add_argument("--trees", type=int, default=1, help="--search / --ismcts / --guided: trees per table")
    ap.add_argument("--uct-trees", type=int, default=None,
                    help="--ismcts / --guided-ismcts: worlds of the UCT lord beside it (default 16 / 4)")
    ap.add_argument("--mode", default="reference", choices=("reference", "sides"), help="--search / --ismcts: the selection rule")
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    dev = torch.device("cuda:0")
    if a.uct_trees is None:
        a.uct_trees = 4 if a.guided_ismcts else 16
    if a.guided_puct:
        for puct, name in ((True, f"guided-PUCT lord ({a.trees} x {a.guided_puct} iterations, leaf {a.leaf}, c {a.c})"),
                           (False, f"guided-UCT lord ({a.trees} x {a.guided_puct} iterations, leaf {a.leaf}, mode sides)")):
            t0 = time.perf_counter()
            st = guided_puct_match(pkg, a, dev, puct)
            dt = time.perf_counter() - t0
            print(f"{name} vs rule farmers: {rates(st)}  [{dt / a.iterations * 1e3:.2f} ms per iteration at {a.tables} tables]")
        return
    if a.guided_ismcts:
        uct_budget = max(1, a.guided_ismcts * a.trees // a.uct_trees)
        for kind, name in (("v4", f"guided-ISMCTS lord ({a.trees} x {a.guided_ismcts} iterations, leaf {a.leaf}, mode {a.mode})"),
                           ("v3", f"guided-UCT lord ({a.uct_trees} x {uct_budget} iterations, leaf {a.leaf})"),
                           ("v2", f"ISMCTS lord ({a.trees} x {a.guided_ismcts} iterations, random playouts)")):
            t0 = time.perf_counter()
            st = guided_ismcts_match(pkg, a, dev, kind)
            dt = time.perf_counter() - t0
            print(f"{name} vs rule farmers: {rates(st)}  [{dt / a.iterations * 1e3:.2f} ms per iteration at {a.tables} tables]")
        return
    if a.guided:
        t0 = time.perf_counter()
        gd = guided_match(pkg, a, dev, True)
        t1 = time.perf_counter()
        uct = guided_match(pkg, a, dev, False)
        t2 = time.perf_counter()
        print(f"guided-UCT lord ({a.trees} x {a.guided} iterations, leaf {a.leaf}, mode {a.mode}) vs rule farmers: {rates(gd)}  "
              f"[{(t1 - t0) / a.iterations * 1e3:.2f} ms per iteration at {a.tables} tables]")
        print(f"determinized-UCT lord ({a.trees} x {a.guided} iterations) vs the same farmers: {rates(uct)}  "
              f"[{(t2 - t1) / a.iterations * 1e3:.2f} ms per iteration]")
        return
    if a.ismcts:
        t0 = time.perf_counter()
        ism = hidden_match(pkg, a, dev, True)
        t1 = time.perf_counter()
        uct = hidden_match(pkg, a, dev, False)
        t2 = time.perf_counter()
        print(f"ISMCTS lord ({a.trees} x {a.ismcts} iterations, mode {a.mode}) vs rule farmers: {rates(ism)}  "
              f"[{(t1 - t0) / a.iterations * 1e3:.2f} ms per iteration at {a.tables} tables]")
        print(f"determinized-UCT lord ({a.uct_trees} x {max(1, a.ismcts * a.trees // a.uct_trees)} iterations) vs the same "
              f"farmers: {rates(uct)}  [{(t2 - t1) / a.iterations * 1e3:.2f} ms per iteration]")
        return
    if a.search:
        t0 = time.perf_counter()
        uct = seat_match(pkg, a, dev, True)
        dt = time.perf_counter() - t0
        flat = seat_match(pkg, a, dev, False)
        print(f"UCT lord ({a.trees} x {a.search} iterations, mode {a.mode}) vs flat Monte-Carlo farmers at "
              f"{a.search * a.trees} playouts per move: {rates(uct)}  [{dt / a.iterations * 1e3:.2f} ms per iteration at "
              f"{a.tables} tables]")
        print(f"flat Monte-Carlo lord vs the same farmers, {a.search * a.trees} playouts per move: {rates(flat)}")
        return
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    env.legal_slab()
    rng_move = torch.full((a.tables,), -1, dtype=torch.int32, device=dev)
    ids = torch.empty(a.tables, dtype=torch.int32, device=dev)
    hidden = a.hidden or a.match
    kw = {"hidden": True, "roles": 0b010} if hidden else {}
    t0 = time.perf_counter()
    for it in range(a.iterations):
        env.playout_choose(a.playouts, salt=it, out=ids, **kw)
        # the lord by playouts; the farmers by the rule agent (--match) or by the engine RNG
        others = env.auto_choose(0b101) if a.match else rng_move
        sel = torch.where(env.role == 1, ids, others)
        env.step_slab(sel, pkg.STEP_IDS, auto_reset=True)
    mc = env.stats()
    dt = time.perf_counter() - t0
    print(f"flat Monte-Carlo lord ({a.playouts} {'hidden-hand' if hidden else 'open'} playouts per move) vs "
          f"{'rule' if a.match else 'random'} farmers: {rates(mc)}  "
          f"[{dt / a.iterations * 1e3:.2f} ms per iteration at {a.tables} tables]")
    base = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    base.reset()
    base.rollout_random(a.iterations)
    print(f"random lord vs random farmers: {rates(base.stats())}")
    assert env.status() == 0 and base.status() == 0


if __name__ == "__main__":
    main()
