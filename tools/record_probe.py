#!/usr/bin/env python3
"""What recording transitions costs per lock-step iteration (variant 2 = EnvCooperation faces, three trained networks, epsilon 0),
device + host time between HIP events, the forms alternated in one process, medians over the repeats:
  (a) SeatLoop.step alone (acting, no recording; auto-reset inside the step);
  (b) TrainLoop.step: the same acting + the device recorder (ddz_tr_before / ddz_tr_after, packed rings), eager and as a captured
      graph;
  (c) the same iteration recorded by the host-paced classes: TransitionAssembler (nonzero / argsort, f32 faces) + one
      Replay.push per role.
and the bytes of pending state per table of both recorders.  Prints one JSON line per table count.
  python tools/record_probe.py [--tables 65536 4096] [--iters 10] [--repeats 7] [--warmup 30]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def probe(pkg, glue, T, n, R, warm, nets, variant=2, capacity=20000):
    dev = torch.device("cuda:0")
    P = pkg.FACE_PLANES[variant]

    def env():
        e = pkg.BatchedEnv(T, seed=5, device=dev)
        e.reset()
        e.legal_slab()
        return e

    ea, eb, ec, ed = env(), env(), env(), env()
    seat = glue.SeatLoop(ea, nets, variant)
    tl = glue.TrainLoop(eb, nets, variant, capacity=capacity)
    tg = glue.TrainLoop(ec, nets, variant, capacity=capacity)
    # (c): SeatLoop's acting, the host classes' recording
    hs = glue.SeatLoop(ed, nets, variant, auto_reset=False)
    asm = glue.TransitionAssembler(T, P, dev)
    reps = [glue.Replay(capacity, P, dev) for _ in range(3)]
    ar = torch.arange(T, device=dev)

    def push(tr):
        for k in range(3):
            m = tr["role"] == k
            reps[k].push({key: v[m] for key, v in tr.items()})

    def host_iteration():
        hs.act()
        rows = ed.slab_rows()
        role = ed.role.clone()
        chosen = pkg.rows_to_onehot(rows[ar, hs.choice.clamp(min=0).long()])
        greedy = pkg.rows_to_onehot(rows[ar, hs.greedy.clamp(min=0).long()])
        push(asm.before_step(role, hs.face, chosen, greedy, active=hs.slot >= 0))
        done, r, _ = ed.step_slab(hs.ids, pkg.STEP_IDS, auto_reset=False)
        ed.observe(variant, out=hs.face)
        push(asm.after_step(role, done, r, hs.face))
        ed.reset(mask=done)
        ed.legal_slab()
        ed.observe(variant, out=hs.face)

    for f in (seat.step, tl.step, tg.step, host_iteration):
        for _ in range(warm):
            f()
    graph = tg.capture(1)
    ta, tb, tgc, tc = [], [], [], []
    for _ in range(R):
        ta.append(timed(seat.step, n))
        tb.append(timed(tl.step, n))
        tgc.append(timed(graph.replay, n))
        tc.append(timed(host_iteration, n))
    counts = tl.rec.note_counts()
    out = {"tables": T, "variant": variant, "iters": n, "repeats": R, "warmup": warm,
           "a_seat_loop_step": spread(ta), "b_train_loop_eager": spread(tb), "b_train_loop_captured": spread(tgc),
           "c_assembler_replay_push": spread(tc),
           "recorder_ws_bytes": int(tl.rec.ws.numel()), "recorder_ws_bytes_per_table": round(tl.rec.ws.numel() / T, 1),
           "assembler_ws_bytes_per_table": 3 * P * 240 + 3 * 240, "ring_entry_bytes": 369, "replay_entry_bytes": 2 * P * 240 + 2 * 240 + 5,
           "ring_counts": counts, "status": [e.status() for e in (ea, eb, ec, ed)]}
    for e in (ea, eb, ec, ed):
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    nets = {}
    for seed, role in enumerate(("lord", "down", "up")):
        torch.manual_seed(seed)
        nets[role] = glue.QNet(9).cuda().eval()
    for T in a.tables:
        print(json.dumps(probe(pkg, glue, T, a.iters, a.repeats, a.warmup, nets)), flush=True)


if __name__ == "__main__":
    main()
