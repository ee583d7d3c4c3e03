#!/usr/bin/env python3
"""The exact endgame solver as a yardstick for the Monte-Carlo players: --tables games are played with uniformly random moves
until their three hands together hold --cards cards or fewer (a table is taken the first time it does), every ending is
solved exactly (BatchedEnv.solve: open-hand minimax per root move, solve spec v1), and the moves that flat Monte Carlo
(playout_choose(--playouts)) and UCT (search_choose(--budget)) pick on the same endings are held against the proven values.

Prints how many endings have a proven-winning move for the side to move, how many are proven lost and how many are left
unknown at the budget, and -- over the endings where a winning move exists -- how often each Monte-Carlo player picks one.

  python examples/endgame_solve.py [--tables 4096] [--cards 12] [--playouts 64] [--budget 1000] [--seed 7]
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def endings(pkg, tables, cards, seed, dev):
    """uint8 [n, 176]: the first state of every random rollout whose three hands hold `cards` cards or fewer"""
    env = pkg.BatchedEnv(tables, seed=seed, device=dev)
    env.reset()
    env.legal_slab()
    taken = torch.zeros(tables, dtype=torch.bool, device=dev)
    out = []
    for _ in range(170):
        st = env.state.view(tables, 11, 16)
        held = st[:, 0:3, :15].to(torch.int32).sum((1, 2))
        hit = (st[:, 10, 1] == 0) & (st[:, 10, 6] != 0) & (held <= cards) & ~taken
        if hit.any():
            out.append(st[hit].clone())
            taken |= hit
        env.step_slab(mode=pkg.STEP_RANDOM, auto_reset=False)
    return torch.cat(out).reshape(-1, 176)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=4096)
    ap.add_argument("--cards", type=int, default=12)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--budget", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    dev = torch.device("cuda:0")
    st = endings(pkg, a.tables, a.cards, a.seed, dev)
    T = len(st)
    env = pkg.BatchedEnv(T, seed=a.seed, device=dev)
    env.state_import(st.reshape(-1))
    n, wins, unknown = env.solve(max_cards=a.cards)
    _, value = env.solve_choose(solved=(n, wins, unknown))
    assert env.status() == 0 and bool((n > 0).all())
    ids = env.slab_ids()                                   # [T, stride]: the canonical ids of the lists solve() read
    winning, lost, open_ = value == 1, value == 0, value == -1
    print(f"{T} endings of {a.cards} cards or fewer from {a.tables} random rollouts: a proven-winning move in {int(winning.sum())} "
          f"({winning.float().mean().item():.1%}), proven lost {int(lost.sum())}, unknown at the default budget {int(open_.sum())}; "
          f"{int(unknown.sum())} of {int(n.sum())} root moves unknown")

    def proven_share(choice):
        """over the endings with a proven-winning move: the share where `choice` (canonical ids) is one"""
        at = (ids == choice[:, None].to(ids.dtype)) & (torch.arange(ids.shape[1], device=dev)[None] < n[:, None])
        good = ((wins > 0) & at).any(1)
        return good[winning].float().mean().item()

    if winning.any():
        flat = env.playout_choose(a.playouts)
        uct = env.search_choose(a.budget)
        print(f"playout_choose({a.playouts}) picks a proven-winning move in {proven_share(flat):.1%} of the endings that have one, "
              f"search_choose({a.budget}) in {proven_share(uct):.1%}")


if __name__ == "__main__":
    main()
