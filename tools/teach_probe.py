#!/usr/bin/env python3
"""What teacher targets cost (variant 2 = EnvCooperation faces, three trained networks, epsilon 0.1), device + host time between
HIP events, medians over the repeats with their range, everything in one process on the states a warmed-up TrainLoop(targets="mc")
left:
  (1) TeacherRecorder.label() alone -- on playout statistics (a total per table: no list is read to count) and on the same
      statistics with a visits array -- alternated with real iterations of that loop, in which the "mc" recorder's own calls
      (before + after) sit between events of their own (tools/return_probe.py's measurement);
  (2) ring entries per label() call (emits, dropped ones included: hdr[k] movement is capped by the ring, so they are counted
      from the statistics) and the bytes they take;
  (3) every Teacher kind's evaluate() at one modest setting (--kinds-tables tables only: the searches are the expensive part).
Prints one JSON line per table count.
  python tools/teach_probe.py [--tables 4096 65536] [--iters 10] [--repeats 7] [--warmup 150] [--kinds-tables 4096]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MC_ENTRY = 189                            # a return ring entry
SETTINGS = {"playout": dict(n_playouts=8, hidden=True), "search": dict(budget=16, trees=1, hidden=True),
            "ismcts": dict(budget=16, trees=1), "guided": dict(budget=8, trees=1, hidden=True), "solve": dict(max_cards=12)}


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


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n


def probe(pkg, glue, T, n, R, warm, nets, kinds, variant=2, capacity=20000):
    env = pkg.BatchedEnv(T, seed=5, device="cuda:0")
    env.reset()
    env.legal_slab()
    loop = glue.TrainLoop(env, nets, variant, capacity=capacity, epsilon=0.1, targets="mc")
    loop.run(warm)
    active = torch.ones(T, dtype=torch.uint8, device="cuda:0")      # (three trained networks: every table is a network table)
    before, after = Stopwatch(loop.rec.before), Stopwatch(loop.rec.after)
    loop.rec.before, loop.rec.after = before, after

    def mc_calls(n):
        """n real iterations of the "mc" loop; the time of the recorder's own calls inside them"""
        before.total(), after.total()
        loop.run(n)
        torch.cuda.synchronize()
        return (before.total() + after.total()) / n

    rec = glue.TeacherRecorder(env, capacity)
    stats = pkg.Teacher("playout", n_playouts=2, hidden=True).evaluate(env)     # (counts is the env's own: it moves with the loop)
    visits = torch.full_like(stats.num, 2)
    visits[::3] = 0                       # a third of the moves unvisited
    forms = {"label_den_const": stats, "label_den_array": stats._replace(den=visits, den_const=None)}
    calls = {k: (lambda n, s=s: timed(lambda: rec.label(s, active), n)) for k, s in forms.items()}
    calls["mc_before_after"] = mc_calls
    for fn in calls.values():
        fn(10)
    times = {k: [] for k in calls}
    entries = {k: [] for k in forms}
    for _ in range(R):
        for k, fn in calls.items():       # alternated
            times[k].append(fn(n))
        live = torch.arange(env.slab_stride, device="cuda:0")[None, :] < env.counts[:, None]
        entries["label_den_const"].append(int(live.sum()))
        entries["label_den_array"].append(int((live & (visits.view(T, -1) > 0)).sum()))
    entries = {k: int(statistics.median(v)) for k, v in entries.items()}
    out = {"tables": T, "variant": variant, "iters": n, "repeats": R, "warmup": warm, "capacity": capacity,
           "ws_bytes": int(rec.ws.numel()), "ring_bytes": int(rec.rings[1].numel())}
    for k in calls:
        out[k] = spread(times[k])
        if k in entries:
            out[k].update(ring_entries_per_call=entries[k], entry_bytes=MC_ENTRY, bytes_per_call_uncapped=entries[k] * MC_ENTRY)
    if T in kinds:
        out["evaluate"] = {}
        for kind, kw in SETTINGS.items():
            teacher = pkg.Teacher(kind, evaluator=pkg.PlayoutLeaf(1) if kind == "guided" else None, **kw)
            for _ in range(2):
                teacher.evaluate(env)
            out["evaluate"][kind] = dict(spread([timed(lambda: teacher.evaluate(env), 2) for _ in range(max(3, R // 2))]), **kw)
    out["status"] = env.status()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=150)
    ap.add_argument("--kinds-tables", type=int, nargs="*", default=[4096])
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    nets = {}
    for seed, role in enumerate(("lord", "down", "up")):
        torch.manual_seed(seed)
        nets[role] = glue.QNet(9).cuda().eval()
    for T in a.tables:
        print(json.dumps(probe(pkg, glue, T, a.iters, a.repeats, a.warmup, nets, a.kinds_tables)), flush=True)


if __name__ == "__main__":
    main()
