#!/usr/bin/env python3
"""Per-role Q forward (dqn_glue.RoleQ / SeatLoop, csrc/ddz_qnet.h section 7) against the single-network compositions it replaces,
device time by HIP events, the compared forms alternated in one process, the spread over repeats:
  1. one-slot map vs FactorisedQ.needed(shared="all") + q_slab (PolicyLoop's Q pass), variants 2 and 3: ms per pass, q equal;
  2. lord net + rule farmers, variant 2: ms per lock-step iteration of (a) config4_rule_opponent.py --lord net's composition
     (the shared-rows pass over ALL tables, arg-max kept where the lord moves) and (b) SeatLoop.step;
  3. rule lord + two farmer networks, variant 2: ms per Q pass of one RoleQ pass and of two single-network passes.
Prints one JSON line.
  python tools/seat_loop_probe.py [--tables 65536] [--iters 10] [--repeats 5]"""
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


def ws_gb(ws):
    """device bytes of a workspace dict (tensors only), GB"""
    return round(sum(v.numel() * v.element_size() for v in ws.values() if torch.is_tensor(v)) / 1e9, 2)


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("doudizhu-rl_amd")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    dev = torch.device("cuda:0")
    T, n, R = a.tables, a.iters, a.repeats
    out = {"tables": T, "iters": n, "repeats": R}
    nets = {}
    for P in (6, 9):
        for seed in (0, 1, 2):
            torch.manual_seed(seed)
            nets[(P, seed)] = glue.QNet(P).to(dev).eval()

    # 1. one-slot map vs the single-network shared pass, same state
    for v, P in ((2, 9), (3, 6)):
        env = pkg.BatchedEnv(T, seed=5, device=dev)
        env.reset()
        env.rollout_random(20)
        env.legal_slab()
        face = env.observe(v)
        A = nets[(P, 0)]
        fq, rq = glue.FactorisedQ(A), glue.RoleQ({"lord": A, "down": A, "up": A}, v)
        q1 = torch.zeros((T, env.slab_stride), device=dev)
        q2 = torch.zeros_like(q1)
        single = lambda: fq.q_slab(env, fq.needed(env, face, shared="all"), out=q1)   # noqa: E731
        roles = lambda: rq.q_slab(env, rq.needed(env, face), q2)                      # noqa: E731
        single(); roles()
        ts, tr = [], []
        for _ in range(R):
            ts.append(timed(single, n))
            tr.append(timed(roles, n))
        valid = torch.arange(env.slab_stride, device=dev)[None, :] < env.counts.long()[:, None]
        w1 = fq._ws[("needed", face.device, T)]
        w2 = next(iter(rq._ws.values()))
        out[f"one_slot_v{v}"] = {"single_network": spread(ts), "role_q": spread(tr),
                                 "q_identical": bool(torch.equal(q1[valid], q2[valid])),
                                 "shared_rows": int(w1["sseg"][32]), "shared_rows_roles": int(w2["sseg"][0, 32]),
                                 "d_rows": int(w1["dseg"][32]), "d_rows_roles": int(w2["dseg"][0, 32]),
                                 "workspace_gb": ws_gb(w1), "workspace_gb_roles": ws_gb(w2)}
        env.close()

    # 2. lord net, rule farmers: the config4 composition vs SeatLoop, two environments on the same deal
    A = nets[(9, 0)]
    ea, eb = pkg.BatchedEnv(T, seed=7, device=dev), pkg.BatchedEnv(T, seed=7, device=dev)
    for e in (ea, eb):
        e.reset()
        e.legal_slab()
    fq = glue.FactorisedQ(A)
    face = torch.empty((T, 9, 15, 4), device=dev)
    qbuf = torch.zeros((T, ea.slab_stride), device=dev)

    def composition():
        sel = ea.auto_choose(0b101)
        ea.observe(2, out=face)
        q = fq.q_slab(ea, fq.needed(ea, face, shared="all"), out=qbuf)
        choice = ea.select_slab(q)
        lord = ea.slab_ids().gather(1, choice.clamp(min=0).long()[:, None])[:, 0].to(torch.int32)
        ea.step_slab(torch.where(sel >= 0, sel, lord), pkg.STEP_IDS, auto_reset=True)

    loop = glue.SeatLoop(eb, {"lord": A}, 2)
    composition(); loop.step()
    ta, tb = [], []
    for _ in range(R):
        ta.append(timed(composition, n))
        tb.append(timed(loop.step, n))
    wl = next(iter(loop.rq._ws.values()))
    wf = fq._ws[("needed", face.device, T)]
    out["lord_net_rule_farmers_v2"] = {"composition": spread(ta), "seat_loop": spread(tb),
                                       "shared_rows_all_tables": int(wf["sseg"][32]), "shared_rows_lord_tables": int(wl["sseg"][0, 32]),
                                       "d_rows_all_tables": int(wf["dseg"][32]), "d_rows_lord_tables": int(wl["dseg"][0, 32]),
                                       "states_equal": bool(torch.equal(ea.state, eb.state))}
    ea.close(); eb.close()

    # 3. rule lord, two farmer networks: one RoleQ pass vs two single-network passes over all tables
    B, C = nets[(9, 1)], nets[(9, 2)]
    env = pkg.BatchedEnv(T, seed=9, device=dev)
    env.reset()
    env.rollout_random(200)             # (past many re-deals: the actors' roles mixed, not the lock-step ply of one deal)
    env.legal_slab()
    face = env.observe(2)
    rq = glue.RoleQ({"down": B, "up": C}, 2)
    fb, fc = glue.FactorisedQ(B), glue.FactorisedQ(C)
    qb, qc, qr = (torch.zeros((T, env.slab_stride), device=dev) for _ in range(3))

    def two():
        fb.q_slab(env, fb.needed(env, face, shared="all"), out=qb)
        fc.q_slab(env, fc.needed(env, face, shared="all"), out=qc)

    one = lambda: rq.q_slab(env, rq.needed(env, face), qr)   # noqa: E731
    two(); one()
    t2, t1 = [], []
    for _ in range(R):
        t2.append(timed(two, n))
        t1.append(timed(one, n))
    w = next(iter(rq._ws.values()))
    wb, wc = fb._ws[("needed", face.device, T)], fc._ws[("needed", face.device, T)]
    out["rule_lord_two_farmer_nets_v2"] = {"two_single_passes": spread(t2), "role_q_pass": spread(t1),
                                           "shared_rows_per_slot": [int(x) for x in w["sseg"][:, 32].tolist()],
                                           "d_rows_per_slot": [int(x) for x in w["dseg"][:, 32].tolist()],
                                           "shared_rows_single_passes": [int(wb["sseg"][32]), int(wc["sseg"][32])],
                                           "d_rows_single_passes": [int(wb["dseg"][32]), int(wc["dseg"][32])],
                                           "workspace_gb_roles": ws_gb(w), "workspace_gb_single": ws_gb(wb) + ws_gb(wc)}
    out["status"] = env.status()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
