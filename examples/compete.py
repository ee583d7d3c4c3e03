#!/usr/bin/env python3
"""Game.compete (game.py:240-290) on the batched engine: a network (greedy), a reference checkpoint or the rule agent per role,
lock-step iterations over --tables tables until at least --total episodes have finished (dqn_glue.compete: SeatLoop, one
role-keyed shared-rows Q pass per iteration; csrc/ddz_qnet.h section 7).  Prints the reference's progress and total-wins lines
and the ms per iteration.

  python examples/compete.py [--lord net|rule|PATH.pt] [--down ...] [--up ...] [--face-variant 2] [--tables 4096] [--total 10000]

`net` is a randomly initialised QNet of the variant's planes (seeded per role); PATH.pt a state dict saved by the reference's
Net.save or metrics.save_state_dict (loaded weights_only).
"""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    for role, default in (("lord", "net"), ("down", "rule"), ("up", "rule")):
        ap.add_argument(f"--{role}", default=default)
    ap.add_argument("--face-variant", type=int, default=2, choices=(1, 2, 3))
    ap.add_argument("--tables", type=int, default=4096)
    ap.add_argument("--total", type=int, default=10000)
    a = ap.parse_args()
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    metrics = importlib.import_module("doudizhu-rl_amd.metrics")
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    dev = torch.device("cuda:0")
    nets = {}
    for k, role in enumerate(("lord", "down", "up")):
        spec = getattr(a, role)
        if spec == "rule":
            nets[role] = None
        elif spec == "net":
            torch.manual_seed(k)
            nets[role] = glue.QNet(engine.FACE_PLANES[a.face_variant]).to(dev).eval()
        else:
            nets[role] = spec
    book = metrics.WinRateBook()
    t0 = time.perf_counter()
    res = glue.compete(a.face_variant, nets, a.total, tables=a.tables, book=book, device=dev)
    dt = time.perf_counter() - t0
    print(book.log_message(res["episodes"], dt), end="")
    eps = max(1, res["episodes"])
    print("Total wins: lord {} ({:.2%}), down {} ({:.2%}), up {} ({:.2%}) over {} episodes".format(
        res["lord"], res["lord"] / eps, res["down"], res["down"] / eps, res["up"], res["up"] / eps, res["episodes"]))
    print(f"tables={a.tables} iterations={res['iterations']}: {dt / max(1, res['iterations']) * 1e3:.2f} ms/iteration "
          f"(wall clock, first-call allocation included)")


if __name__ == "__main__":
    main()
