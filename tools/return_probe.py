#!/usr/bin/env python3
"""What Monte-Carlo return targets cost beside one-step TD targets (variant 2 = EnvCooperation faces, three trained networks,
epsilon 0.1), device + host time between HIP events, the two targets alternated in one process, medians over the repeats:
  (1) TrainLoop.step with targets="td" and targets="mc", and inside each the recorder's own calls (before + after) between
      events of their own;
  (2) bytes the recorder writes per iteration (from the ring counts' movement over the timed iterations) and per ring entry;
  (3) td_step against mc_step on packed batches of 256 and 4,096 drawn from the rings the loops filled.
Prints one JSON line per table count.
  python tools/return_probe.py [--tables 4096 65536] [--iters 10] [--repeats 7] [--warmup 150]"""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TR_ENTRY, TR_SLOT = 369, 176 + 4          # a transition; what ddz_tr_before writes per recorded decision (row + action id)
MC_ENTRY, MC_LOG = 189, 182               # a return entry; a log entry


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


class Stopwatch:
    """HIP events around every call of fn; total() after a synchronisation"""

    def __init__(self, fn):
        self.fn, self.pairs = fn, []

    def __call__(self, *a, **kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = self.fn(*a, **kw)
        e.record()
        self.pairs.append((s, e))
        return out

    def total(self):
        t = sum(s.elapsed_time(e) for s, e in self.pairs)
        self.pairs = []
        return t


def timed(loop, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        loop.step()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n, (loop.rec.before.total() + loop.rec.after.total()) / n


def learner(glue, rec, nets, step, n, R, warm, variant=2):
    out = {}
    for batch in (256, 4096):
        policy = copy.deepcopy(nets["lord"]).train()
        target = copy.deepcopy(nets["lord"]).eval()
        opt = torch.optim.Adam(policy.parameters(), 1e-4)
        b = rec.sample_packed("lord", batch, variant, at_least=1)
        fn = (lambda: glue.td_step(policy, target, opt, b)) if step == "td" else (lambda: glue.mc_step(policy, opt, b))
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(R):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                fn()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e) / n)
        out[str(batch)] = spread(ts)
    return out


def probe(pkg, glue, T, n, R, warm, nets, variant=2, capacity=20000):
    loops = {}
    for targets in ("td", "mc"):
        env = pkg.BatchedEnv(T, seed=5, device="cuda:0")
        env.reset()
        env.legal_slab()
        loop = glue.TrainLoop(env, nets, variant, capacity=capacity, epsilon=0.1, targets=targets)
        loop.rec.before, loop.rec.after = Stopwatch(loop.rec.before), Stopwatch(loop.rec.after)
        loop.run(warm)
        torch.cuda.synchronize()
        loop.rec.before.total(), loop.rec.after.total()
        loops[targets] = loop
    start = {k: v.rec.note_counts() for k, v in loops.items()}
    times = {k: ([], []) for k in loops}
    for _ in range(R):
        for k, loop in loops.items():                      # alternated
            it, rec = timed(loop, n)
            times[k][0].append(it)
            times[k][1].append(rec)
    moved = {k: sum(v.rec.note_counts()) - sum(start[k]) for k, v in loops.items()}
    its = n * R
    out = {"tables": T, "variant": variant, "iters": n, "repeats": R, "warmup": warm}
    for k, loop in loops.items():
        entry, opened = (TR_ENTRY, TR_SLOT) if k == "td" else (MC_ENTRY, MC_LOG)
        out[k] = {"iteration": spread(times[k][0]), "recorder_calls": spread(times[k][1]),
                  "ring_entries_per_iteration": round(moved[k] / its, 1), "ring_entry_bytes": entry,
                  "bytes_written_per_iteration": round(moved[k] / its * entry + T * opened),
                  "ws_bytes": int(loop.rec.ws.numel()), "ring_bytes": int(loop.rec.rings[1].numel())}
        out[k]["step_packed"] = learner(glue, loop.rec, nets, k, n, R, 10, variant)
        out[k]["status"] = loop.env.status()
        loop.env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=150)
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
