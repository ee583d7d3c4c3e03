#!/usr/bin/env python3
"""The reference's serving policy as a seat on the batched engine: a lord that plays server/core.py's three-way switch
(Predictor.act, :74-118) against the rule farmers, every table in lock step, nothing per table on the host --

  the lord holds 12 cards or more          the rule agent                          (env.auto_choose)
  the three hands hold 6 cards or fewer    CFR, 8 iterations, a sampled move       (env.cfr_choose: CFR spec v1)
  otherwise                                the Q-network's greedy move             (dqn_glue.ragged_q + env.select)

-- in the manner of the reference's ensemble_compete (ensemble.py), which asks a remote predictor for every move.  The three
id vectors are merged with torch.where and stepped with step_slab(STEP_IDS); the farmers' moves are env.auto_choose(0b101).
Prints the lord's win rate from env.stats() and how many of its decisions each engine took.  The Q-network is --net PATH.pt
(a state dict of the reference's Net for EnvCooperationSimplify) or, without it, randomly initialised: the win rate printed
is a property of that network and has not been measured anywhere in this repository's notes.

  python examples/predictor_match.py [--tables 1024] [--iterations 300] [--seed 0] [--net PATH.pt] [--greedy]
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--net", default=None, help="state dict of the lord's Q-network (default: random weights)")
    ap.add_argument("--greedy", action="store_true", help="CFR plays the first maximum of sigma instead of sampling")
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    net = glue.QNet(engine.FACE_PLANES[3]).to(dev).eval()
    if a.net:
        net.load_state_dict(torch.load(a.net, map_location=dev))
    env = pkg.BatchedEnv(a.tables, seed=a.seed, device=dev)
    env.reset()
    rule = torch.empty(a.tables, dtype=torch.int32, device=dev)
    cfr = torch.empty(a.tables, dtype=torch.int32, device=dev)
    used = torch.zeros(3, dtype=torch.int64, device=dev)            # the lord's decisions by Rule / CFR / RL1
    for it in range(a.iterations):
        off, rows, ids = env.legal()
        with torch.no_grad():
            q = glue.ragged_q(net, env.observe(3), rows, off)
        choice = env.select(q)
        rl = ids[(off[:-1].long() + choice.clamp(min=0).long()).clamp(max=ids.numel() - 1)]
        env.auto_choose(0b111, out=rule)
        env.cfr_choose(8, roles=0b010, salt=it, greedy=a.greedy, out=cfr)
        left = env.hands()[:, :, 15].to(torch.int32)
        is_lord = (env.role == 1) & (choice >= 0)
        by_rule = left[:, 1] >= 12
        by_cfr = ~by_rule & (left.sum(1) <= 6) & (cfr >= 0)
        lord = torch.where(by_rule, rule, torch.where(by_cfr, cfr, rl))
        used += torch.stack([(is_lord & by_rule).sum(), (is_lord & by_cfr).sum(), (is_lord & ~by_rule & ~by_cfr).sum()])
        env.step_slab(torch.where(env.role == 1, lord, rule), pkg.STEP_IDS, auto_reset=True)
    status = env.status()
    assert status & ~pkg.STATUS_CFR_CAPACITY == 0, status   # (more endgames in one iteration than workspace slots)
    s = env.stats()
    e = max(1, s["episodes"])
    u = used.tolist()
    print(f"{s['episodes']} episodes: lord (Rule {u[0]} / CFR {u[1]} / RL1 {u[2]} decisions) {s['lord_wins'] / e:.1%}, "
          f"rule farmers {(s['up_wins'] + s['down_wins']) / e:.1%}")


if __name__ == "__main__":
    main()
