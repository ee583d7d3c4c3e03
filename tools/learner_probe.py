#!/usr/bin/env python3
"""What one td_step costs with the literal QNet.forward, with QNet.forward_fused (the first layer by the engine's kernels,
csrc/ddz_qtrain.h), with QNet.forward_stage (everything in front of dropout by the engine's kernels) -- these three on the same
random faces -- and on a packed batch (QNet.forward_packed; the time INCLUDES TransitionRecorder.sample_packed, drawn from a ring
that a TrainLoop at 4,096 tables filled; "sample" is what the other forms would pay on top: the decode of such a draw into faces):
device + host time between HIP events, the forms alternated in one process, medians over the repeats.  Per face variant and batch size:
  td_step eager, literal / fused / stage / packed;  td_step as a captured graph (Adam capturable=True), where the capture works;
  the first layer alone: forward and forward + backward, literal chain (cat, conv1..4, cat, max-pool) / FirstLayer;
  the stage alone: forward and forward + backward, literal lines up to the dropout / Stage on faces / Stage on the ring.
Prints one JSON line per (variant, batch).  A library without the stage (an older commit) reports the forms it has.
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


_rings = {}


def filled_recorder(pkg, glue, variant):
    """a TrainLoop's recorder after 40 iterations at 4,096 tables (one per variant): every ring holds tens of thousands of entries"""
    if variant not in _rings:
        P = pkg.FACE_PLANES[variant]
        torch.manual_seed(100 + variant)
        nets = {r: glue.QNet(P).to("cuda:0").eval() for r in ("lord", "down", "up")}
        env = pkg.BatchedEnv(4096, seed=variant, device="cuda:0")
        env.reset()
        env.legal_slab()
        loop = glue.TrainLoop(env, nets, variant, capacity=glue.REPLAY_SIZE, epsilon=0.1)
        loop.run(40)
        loop.rec.note_counts()
        _rings[variant] = loop.rec
    return _rings[variant]


def probe(pkg, glue, variant, B, n, R, warm):
    dev = torch.device("cuda:0")
    has_stage = hasattr(glue, "Stage")
    rec = filled_recorder(pkg, glue, variant) if has_stage else None
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
        if fused == "packed":
            return lambda: glue.td_step(net, target, opt, rec.sample_packed("lord", B, variant), glue.GAMMA)
        return lambda: glue.td_step(net, target, opt, batch, glue.GAMMA, fused=fused)

    res = {"variant": variant, "planes": P, "batch": B, "iters": n, "repeats": R, "warmup": warm}
    forms = (("literal", False), ("fused", True)) + ((("stage", "stage"), ("packed", "packed")) if has_stage else ())
    eager = {name: learner(fused, False) for name, fused in forms}
    if has_stage:
        eager["sample"] = lambda: rec.sample("lord", B, variant)
    for fn in eager.values():
        for _ in range(warm):
            fn()
    res["td_step_eager"] = alternate(eager, n, R)
    # (the captured learners stay alive beside their graphs: a graph holds raw addresses of the networks and the Adam state, and the
    # next capture empties the allocator's cache -- memory of a learner dropped here would be unmapped under the earlier graph)
    graphs, why, kept = {}, {}, {}
    for name, fused in forms:
        kept[name] = learner(fused, True)
        gr, err = capture(kept[name], 3)
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
    if has_stage:
        sparams = params + [net.conv_shunzi.weight, net.conv_shunzi.bias]
        gh = torch.randn((B, 4864), generator=g, device=dev)
        pb = rec.sample_packed("lord", B, variant)
        rows = {"states": pb.s0, "ids": pb.a0, "index": pb.index, "table": pb.table, "variant": variant}

        def literal_stage():
            x = torch.cat((face, act.unsqueeze(1)), dim=1)
            y = torch.cat([f(x) for f in (net.conv1, net.conv2, net.conv3, net.conv4)], -1)
            return torch.cat([net.pool(y).view(B, -1), net.conv_shunzi(x).view(B, -1)], -1)

        def both_h(fwd):
            def run():
                net.zero_grad(set_to_none=True)
                fwd().backward(gh)
            return run

        on_faces = lambda: glue.Stage.apply({"face": face, "actions": act}, *sparams)   # noqa: E731
        on_rows = lambda: glue.Stage.apply(rows, *sparams)                              # noqa: E731
        forms = {"fwd_literal": no_grad(literal_stage), "fwd_faces": no_grad(on_faces), "fwd_rows": no_grad(on_rows),
                 "fwd_bwd_literal": both_h(literal_stage), "fwd_bwd_faces": both_h(on_faces), "fwd_bwd_rows": both_h(on_rows)}
        for fn in forms.values():
            for _ in range(warm):
                fn()
        res["stage"] = alternate(forms, n, R)
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
    # the whole stage: z = [B,1024] f32, h = [B,4864] f32; packed rows: a 176-byte state row + an action id per sample and side
    z, h, wts_s = B * 4096, B * 4864 * 4, 256 * C * 15 * 4 + 1024
    parts_s = min((B + 7) // 8, 512) * (15 * C + 1) * 1024
    res["bytes"].update({
        # fused=True behind its first layer: cat (read + write x), conv_shunzi (x -> z), cat (read y + z, write h)
        "fwd_fused_rest": 2 * x + x + z + wts_s + 2 * h,
        # ... backward: the cat's slices (read h, write y + z), conv_shunzi's weight and bias gradients (x + z, z)
        "bwd_fused_rest": 2 * h + x + 2 * z + wts_s,
        "fwd_stage": 2 * x + wts + wts_s + h + B * 3840,            # two launches, each reads x
        "bwd_stage": 2 * x + h + B * 3840 + 2 * (parts + parts_s) + wts + wts_s,
        "fwd_packed": 2 * B * (176 + 4 + 8) + wts + wts_s + h + B * 3840,
        "bwd_packed": 2 * B * (176 + 4 + 8) + h + B * 3840 + 2 * (parts + parts_s) + wts + wts_s,
        "decode_per_side": B * (176 + 4 + 8 + 16) + x + B * 240,   # what sample() writes (and td_step then reads) per side
    })
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
