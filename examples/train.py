#!/usr/bin/env python3
"""Game.train (game.py:183-238; the set-up of the reference's train.py:8-31) on the batched engine: EnvCooperation faces, a
NetCooperation-shaped QNet per trained role, the rule agent for the others; dqn_glue.train -- TrainLoop (SeatLoop's acting, the
device-side transition recorder and packed replay rings of csrc/ddz_replay.h; nothing on the host inside an iteration) + one
autograd td_step per trained role per iteration.  Hyper-parameters are the reference's (config.py:8-14).  Prints the
reference's progress lines, the total wins and the checkpoints written.

  python examples/train.py [--lord-vs-rule] [--tables 4096] [--episodes 20000] [--log-every 5000] [--model-every 10000]
                           [--model-dir models] [--win-dir outs/win_rates] [--fused | --packed] [--batch-size 256]
                           [--mc [--gamma 1.0]]
                           [--teacher KIND[:N] [--teacher-hidden] [--label-every N] [--act-teacher]]

Default: lord, down and up all train (three networks).  --lord-vs-rule: the reference's train.py as it stands -- the lord trains
against the rule-based farmers (reward_dict {'lord': 100}).  --fused: td_step through QNet.forward_fused (the first layer by the
engine's forward / backward kernels, csrc/ddz_qtrain.h); --packed: batches stay packed replay rows and both passes of td_step run
QNet.forward_packed (two stage launches per pass, no face, no library convolution); --batch-size: transitions per td_step (the reference's 256).
--mc: Monte-Carlo return targets instead of one-step TD targets -- the device-side return recorder of csrc/ddz_returns.h, one mc_step
per trained role per iteration, no target network; --gamma: the discount of the returns (default 1.0: Deep Monte Carlo).
--teacher: search-supervised targets (teacher spec v1, csrc/ddz_teach.h) -- every --label-every-th iteration the evaluator KIND
runs on the trained roles' tables and every legal move gets reward * (2 wins / visits - 1) as its target; playout:8 = 8 playouts
per move, search:64 / ismcts:64 = a budget of 64 iterations, solve = the exact endgame solver (endgames only).  --teacher-hidden:
the teacher does not read the opponents' hands (open-hand labels are legitimate for training, not for serving; ismcts is always
hidden).  --act-teacher: the labelled tables also play the teacher's move (expert iteration).
"""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FACE_VARIANT = 2   # EnvCooperation (envi.py:182-198), 9 planes: NetCooperation's input (net.py)


def make_teacher(engine, ap, spec, hidden):
    """KIND[:N] -> engine.Teacher: N is n_playouts of playout, the budget of search / ismcts"""
    kind, _, n = spec.partition(":")
    size = {"playout": "n_playouts", "search": "budget", "ismcts": "budget", "solve": None}
    if kind not in size or bool(n) != (size[kind] is not None) or (n and not n.isdigit()):
        ap.error("--teacher: playout:N, search:N, ismcts:N or solve")
    kw = {size[kind]: int(n)} if n else {}
    if kind != "ismcts":
        kw["hidden"] = hidden
    return engine.Teacher(kind, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lord-vs-rule", action="store_true")
    ap.add_argument("--tables", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=20000)
    ap.add_argument("--log-every", type=int, default=5000)
    ap.add_argument("--model-every", type=int, default=10000)
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--win-dir", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--mc", action="store_true")
    ap.add_argument("--gamma", type=float, default=None)
    ap.add_argument("--teacher", default=None, metavar="KIND[:N]")
    ap.add_argument("--teacher-hidden", action="store_true")
    ap.add_argument("--label-every", type=int, default=1)
    ap.add_argument("--act-teacher", action="store_true")
    a = ap.parse_args()
    if a.gamma is not None and not a.mc:
        ap.error("--gamma is the discount of --mc's returns")
    if a.teacher and a.mc:
        ap.error("--teacher and --mc are two kinds of targets: pick one")
    if not a.teacher and (a.teacher_hidden or a.act_teacher or a.label_every != 1):
        ap.error("--teacher-hidden, --label-every and --act-teacher go with --teacher")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    metrics = importlib.import_module("doudizhu-rl_amd.metrics")
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    roles = ("lord",) if a.lord_vs_rule else ("lord", "down", "up")
    nets, train_dict, reward_dict = {}, {}, dict(glue.REWARD_DICT)
    for k, role in enumerate(("lord", "down", "up")):
        torch.manual_seed(a.seed * 3 + k)
        nets[role] = glue.QNet(engine.FACE_PLANES[FACE_VARIANT]) if role in roles else None
        train_dict[role] = role in roles
        print("{}: {} based model.{}".format(role, "AI" if role in roles else "Rule",
                                             " Without pretrained model. Continue training." if role in roles else ""))
    teacher = make_teacher(engine, ap, a.teacher, a.teacher_hidden) if a.teacher else None
    targets = "teacher" if teacher else "mc" if a.mc else "td"
    book = metrics.WinRateBook()
    t0 = time.perf_counter()
    res = glue.train(FACE_VARIANT, nets, a.episodes, train_dict=train_dict, reward_dict=reward_dict, tables=a.tables,
                     seed=a.seed, log_every=a.log_every, model_every=a.model_every, book=book, model_dir=a.model_dir,
                     win_dir=a.win_dir, log=lambda m: print(m, end=""), fused="packed" if a.packed else a.fused,
                     batch_size=glue.BATCH_SIZE if a.batch_size is None else a.batch_size,
                     targets=targets, gamma=a.gamma, teacher=teacher, label_every=a.label_every,
                     act="teacher" if a.act_teacher else "net")
    dt = time.perf_counter() - t0
    eps = max(1, res["episodes"])
    print("Total wins: lord {} ({:.2%}), down {} ({:.2%}), up {} ({:.2%}) over {} episodes".format(
        res["lord"], res["lord"] / eps, res["down"], res["down"] / eps, res["up"], res["up"] / eps, res["episodes"]))
    print("last loss: " + ", ".join(f"{r} {v:.3f}" if v is not None else f"{r} -" for r, v in res["loss"].items()))
    for p in res["checkpoints"]:
        print("saved", p)
    print(f"tables={a.tables} iterations={res['iterations']}: {dt / max(1, res['iterations']) * 1e3:.2f} ms/iteration "
          f"(wall clock, {'td_step' if targets == 'td' else 'mc_step'} and first-call allocation included)")


if __name__ == "__main__":
    main()
