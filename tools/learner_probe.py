#!/usr/bin/env python3
"""What one td_step costs with the literal QNet.forward and with QNet.forward_fused (the first layer by the engine's kernels,
csrc/ddz_qtrain.h), on random faces: device + host time between HIP events, the two forms alternated in one process, medians
over the repeats.  Per face variant and batch size:
  td_step eager, literal / fused;  td_step as a captured graph (Adam capturable=True), literal / fused, where the capture works;
  the first layer alone: forward and forward + backward, literal chain (cat, conv1..4, cat, max-pool) / FirstLayer.
Prints one JSON line per (variant, batch).
  python tools/learner_probe.py [--variants 2 3] [--batches 256 4096 16384] [--iters 10] [--repeats 7] [--warmup 30]"""
import argparse
import copy
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


def capture(step, warm):
    """the step as one graph (None with the reason when this torch / runtime cannot capture it)"""
    dev = torch.device("cuda:0")
    try:
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(warm):
                step()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        g.replay()
        torch.cuda.synchronize(dev)
        return g, None
    except Exception as exc:     # noqa: BLE001  (reported, not hidden: the line says which form was not captured and why)
        torch.cuda.synchronize(dev)
        return None, f"{type(exc).__name__}: {str(exc)[:200]}"


def alternate(forms, n, R):
    """{name: spread} of the callables, alternated R times"""
    out = {k: [] for k in forms}
    for _ in range(R):
        for k, fn in forms.items():
            out[k].append(timed(fn, n))
    return {k: spread(v) for k, v in out.items()}


def probe(pkg, glue, variant, B, n, R, warm):
    dev = torch.device("cuda:0")
    P = pkg.FACE_PLANES[variant]
    C = P + 1
    g = torch.Generator(device=dev).manual_seed(B + variant)
    rnd = lambda *s: torch.rand(s, generator=g, device=dev)   # noqa: E731
    batch = {"s0": rnd(B, P, 15, 4), "a0": (rnd(B, 15, 4) < 0.2).float(), "s1": rnd(B, P, 15, 4),
             "a1": (rnd(B, 15, 4) < 0.2).float(), "reward": rnd(B) * 100 - 50, "done": rnd(B) < 0.05}
    torch.manual_seed(variant)
    base = glue.QNet(P).to(dev)

    def learner(fused, capturable):
        net = copy.deepcopy(base).train()
        target = copy.deepcopy(base).eval()
        opt = torch.optim.Adam(net.parameters(), glue.LEARNING_RATE, capturable=capturable)
        return lambda: glue.td_step(net, target, opt, batch, glue.GAMMA, fused=fused)

    res = {"variant": variant, "planes": P, "batch": B, "iters": n, "repeats": R, "warmup": warm}
    eager = {"literal": learner(False, False), "fused": learner(True, False)}
    for fn in eager.values():
        for _ in range(warm):
            fn()
    res["td_step_eager"] = alternate(eager, n, R)
    graphs, why = {}, {}
    for name, fused in (("literal", False), ("fused", True)):
        gr, err = capture(learner(fused, True), 3)
        if gr is None:
            why[name] = err
        else:
            graphs[name] = gr.replay
    if graphs:
        for fn in graphs.values():
            for _ in range(warm):
                fn()
        res["td_step_graph"] = alternate(graphs, n, R)
    if why:
        res["not_captured"] = why
    # the first layer alone
    net = copy.deepcopy(base)
    params = [p for cv in (net.conv1, net.conv2, net.conv3, net.conv4) for p in (cv.weight, cv.bias)]
    face, act, gy = batch["s0"], batch["a0"], torch.randn((B, 3840), generator=g, device=dev)

    def literal():
        x = torch.cat((face, act.unsqueeze(1)), dim=1)
        y = torch.cat([f(x) for f in (net.conv1, net.conv2, net.conv3, net.conv4)], -1)
        return net.pool(y).view(B, -1)

    def both(fwd):
        def run():
            net.zero_grad(set_to_none=True)
            fwd().backward(gy)
        return run

    def no_grad(fwd):
        def run():
            with torch.no_grad():
                fwd()
        return run

    fused = lambda: glue.FirstLayer.apply(face, act, *params)   # noqa: E731
    forms = {"fwd_literal": no_grad(literal), "fwd_fused": no_grad(fused), "fwd_bwd_literal": both(literal), "fwd_bwd_fused": both(fused)}
    for fn in forms.values():
        for _ in range(warm):
            fn()
    res["first_layer"] = alternate(forms, n, R)
    # bytes each form moves through global memory, from the layouts (f32; x = face + action, pre = [B,256,15,4], y = [B,3840])
    x, pre, y = B * C * 240, B * 256 * 15 * 4 * 4, B * 3840 * 4
    wts = sum(256 * C * k * 4 + 1024 for k in range(1, 5))
    parts = min((B + 7) // 8, 512) * (10 * C + 4) * 1024
    res["bytes"] = {
        # cat: read + write x; convs: read x four times, write pre/4 each; cat: read + write pre; pool: read pre, write y + indices
        "fwd_literal": 2 * x + 4 * x + pre + 2 * pre + pre + y + 2 * y,
        "fwd_fused": x + wts + y + B * 3840,
        # pool backward: read gy + indices, write pre; cat backward: read pre, write pre; four weight- and four bias-gradient kernels
        "bwd_literal": y + 2 * y + pre + 2 * pre + 4 * x + 2 * pre + wts,
        "bwd_fused": x + y + B * 3840 + 2 * parts + wts,
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 16384])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("learner_probe: no GPU visible (nothing is timed on a CPU)")
    pkg = importlib.import_module("doudizhu-rl_amd")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    for v in a.variants:
        for B in a.batches:
            print(json.dumps(probe(pkg, glue, v, B, a.iters, a.repeats, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
