#!/usr/bin/env python3
"""CPU only: what the host side of a call costs, per verb, with no device behind it -- the recorder verbs, teach, the *_choose
verbs and Teacher.evaluate / choose of a BatchedEnv built by tests/test_engine_arguments_cpu.py's make_env on a stand-in library
whose launches return at once.  Best of `--repeats` x `--calls` calls, microseconds per call, one JSON line.  Run it on two
checkouts to compare their host layers:
  python tools/host_call_probe.py [--tree PATH] [--calls 2000] [--repeats 7]"""
import argparse
import importlib
import json
import os
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    sys.path[:0] = [a.tree, os.path.join(a.tree, "tests")]
    torch.set_num_threads(1)
    A = importlib.import_module("test_engine_arguments_cpu")
    M = importlib.import_module("doudizhu-rl_amd.engine")

    class Quiet:
        def __getattr__(self, name):
            if name.endswith("_bytes") or name in A.SIZE_QUERIES:
                return lambda *args: A.SIZE_QUERIES.get(name, 64)
            return lambda *args: 0

    lib = Quiet()
    M._lib.lib = lambda jk=False: lib
    M._stream = lambda device: None
    M._require_gpu = lambda device: torch.device(device)
    T, z, u8, i8, i32 = A.T, A.z, A.u8, A.i8, A.i32
    env, out = A.make_env(M), z(T, dt=i32)
    ws, rings, ids, active, done, r = z(64, dt=u8), A.rings(), z(T, dt=i32), z(T, dt=u8), z(T, dt=u8), z(T, dt=i8)
    num, reward = z(A.CAP, dt=i32), (50.0, 100.0, 50.0)
    calls = {
        "tr_before": lambda: env.tr_before(ws, rings, 8, ids, ids, active, 0b110),
        "tr_after": lambda: env.tr_after(ws, rings, 8, done, r, reward),
        "mc_before": lambda: env.mc_before(ws, 54, ids, active, 0b110),
        "mc_after": lambda: env.mc_after(ws, 54, rings, 8, done, r, reward),
        "teach": lambda: env.teach(ws, rings, 8, num, den_const=4, active=active, trained_roles=0b110),
        "playout_choose": lambda: env.playout_choose(4, out=out),
        "search_choose": lambda: env.search_choose(8, trees=2, out=out),
        "ismcts_choose": lambda: env.ismcts_choose(8, trees=2, out=out),
        "solve_choose": lambda: env.solve_choose(out=out),
        "cfr_choose": lambda: env.cfr_choose(out=out),
    }
    for kind, kw in (("playout", dict(n_playouts=4)), ("search", dict(budget=8, trees=2)), ("ismcts", dict(budget=8, trees=2)),
                     ("solve", {})):
        t = M.Teacher(kind, **kw)
        calls[f"Teacher({kind}).evaluate"] = lambda t=t: t.evaluate(env)
        calls[f"Teacher({kind}).evaluate+choose"] = lambda t=t: t.choose(env, t.evaluate(env), out=out)
    res = {}
    for name, f in calls.items():
        f()
        best = float("inf")
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            best = min(best, (time.perf_counter() - t0) / a.calls)
        res[name] = round(best * 1e6, 2)
    print(json.dumps({"tree": a.tree, "us_per_call": res}))


if __name__ == "__main__":
    main()
