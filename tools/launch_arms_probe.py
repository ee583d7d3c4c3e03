#!/usr/bin/env python3
"""Walks every arm of the C entry points that choose a kernel instance by a run-time value (the table in profiles/r24_notes.md),
once each, at the smallest shape that selects it: 64 tables everywhere, 6,000 tables without ids for the dense rollout arms (their
threshold is 5,400 wavefronts), one to three iterations per arm.  One stream, a synchronisation behind every arm, no second try:
the first error ends the run.  Meant to run under `rocprofv3 --kernel-trace` on two builds of the library, whose ordered lists of
kernel names (with their template arguments) must then be equal:
  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_arms_probe.py [--library PATH]
  python tools/launch_arms_probe.py --names OUT_A/**/*kernel_trace.csv > a.txt      (the engine's kernels of a trace, in start order)"""
import argparse
import csv
import importlib
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_KERNEL = re.compile(r"^(void )?(\(anonymous namespace\)::|_ZN12_GLOBAL__N_1\d+)k_")


def names(paths):
    rows = []
    for p in paths:
        for r in csv.DictReader(open(p, newline="")):
            if ENGINE_KERNEL.match(r["Kernel_Name"]):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
    for _, n in sorted(rows):
        print(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None, help="another build of the default library (_lib.use_library)")
    ap.add_argument("--names", nargs="+", default=None, help="kernel-trace CSV files: print the engine's kernel names in start order")
    a = ap.parse_args()
    if a.names:
        return names(a.names)
    sys.path.insert(0, REPO)
    import torch
    pkg = importlib.import_module("doudizhu-rl_amd")
    L = importlib.import_module("doudizhu-rl_amd._lib")
    if a.library:
        L.use_library(os.path.abspath(a.library))
    E = importlib.import_module("doudizhu-rl_amd.engine")
    G = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    dev = torch.device("cuda:0")
    T, DENSE_T = 64, 6000
    count = [0]

    def arm(site, cond, fn):
        fn()
        torch.cuda.synchronize()
        count[0] += 1
        print(f"arm {count[0]:3d}  {site}: {cond}", flush=True)

    def env(ids, coop=None, tables=T):
        e = pkg.BatchedEnv(tables, seed=7, device=dev, want_ids=ids,
                           _debug_tables_per_wave=None if coop is None else 1, _debug_slab_coop=coop)
        e.reset()
        return e

    def traj(e, n=1):
        return torch.zeros((n, e.T, 32), dtype=torch.uint8, device=dev)

    # launch_moves, ddz_get_moves_slab: ids
    e = env(True)
    hands, lasts = e.hands()[:, 0].contiguous(), torch.zeros((T, 16), dtype=torch.int8, device=dev)
    for ids in (True, False):
        arm("launch_moves", f"ids={ids}", lambda: pkg.get_moves(hands, lasts, want_ids=ids))
        arm("ddz_get_moves_slab", f"ids={ids}", lambda: pkg.get_moves_slab(hands, lasts, want_ids=ids))
    # launch_table (ids), ddz_step (mode), ddz_slab_to_csr (ids_out), ddz_rollout_random_csr per iteration
    for ids in (True, False):
        e = env(ids)
        arm("launch_table", f"F_ENUM ids={ids}", e.legal)
        sel = {pkg.STEP_RANDOM: None, pkg.STEP_CHOICE: torch.zeros(T, dtype=torch.int32, device=dev),
               pkg.STEP_IDS: torch.full((T,), -1, dtype=torch.int32, device=dev)}
        for mode in (pkg.STEP_RANDOM, pkg.STEP_CHOICE, pkg.STEP_ROWS, pkg.STEP_IDS):
            if mode == pkg.STEP_ROWS:
                e.legal()
                sel[mode] = e.rows[e.offsets[:-1].long()].clone()       # the first legal move of the current states
            arm("ddz_step", f"mode={mode} ids={ids}", lambda: e.step(sel[mode], mode, traj=traj(e)[0]))
        arm("launch_table", f"F_SLAB ids={ids}", e.legal_slab)
        arm("ddz_slab_to_csr", f"ids_out={ids}", lambda: e.slab_to_csr(rows_per_table=512))
        arm("launch_table", f"F_ENUM|F_STEP ids={ids}", lambda: e.rollout_random_csr(2, batch=0))
    # ddz_step_slab: mode x ids x coop; ddz_policy_step_slab: ids x coop
    for coop in (1, 0):
        for ids in (True, False):
            e = env(ids, coop)
            e.legal_slab()
            for mode in (pkg.STEP_RANDOM, pkg.STEP_CHOICE, pkg.STEP_ROWS, pkg.STEP_IDS):
                sel = {pkg.STEP_RANDOM: None, pkg.STEP_CHOICE: torch.zeros(T, dtype=torch.int32, device=dev),
                       pkg.STEP_ROWS: e.slab_rows()[:, 0].contiguous(), pkg.STEP_IDS: torch.full((T,), -1, dtype=torch.int32, device=dev)}[mode]
                arm("ddz_step_slab", f"mode={mode} ids={ids} coop={coop}", lambda: e.step_slab(sel, mode, traj=traj(e)[0]))
            q = torch.zeros((T, e.slab_stride), dtype=torch.float32, device=dev)
            arm("ddz_policy_step_slab", f"ids={ids} coop={coop}", lambda: e.policy_step_slab(q, 0.0, face_variant=3, traj=traj(e)[0]))
    # launch_rollout: ids x records x staged below the dense threshold, records x staged above it
    for ids in (True, False):
        for rec in (False, True):
            e = env(ids)
            arm("launch_rollout", f"ids={ids} traj={rec} staged=False dense=False", lambda: e.rollout_random(3, traj=traj(e, 3) if rec else None))
            arm("launch_rollout", f"ids={ids} traj={rec} staged=True dense=False",
                lambda: e.rollout_random_csr(3, traj=traj(e, 3) if rec else None, batch=2))
    e = env(False, tables=DENSE_T)
    for rec in (False, True):
        arm("launch_rollout", f"ids=False traj={rec} staged=False dense=True", lambda: e.rollout_random(2, traj=traj(e, 2) if rec else None))
        arm("launch_rollout", f"ids=False traj={rec} staged=True dense=True",
            lambda: e.rollout_random_csr(2, traj=traj(e, 2) if rec else None, batch=2))
    del e
    # the faces and the Q forward: variant / planes
    on_stream = lambda name, fn: fn()                                    # noqa: E731  (FactorisedQ.needed: every stage on this stream)
    e = env(True)
    e.legal_slab()
    states = e.state.view(T, -1)
    table = E.action_table(dev)
    zero_ids = torch.zeros(T, dtype=torch.int32, device=dev)
    actions = torch.zeros((T, 15, 4), dtype=torch.float32, device=dev)
    torch.manual_seed(0)
    for v in range(4):
        P = E.FACE_PLANES[v]
        face = torch.empty((T, P, 15, 4), dtype=torch.float32, device=dev)
        arm("ddz_observe", f"variant={v}", lambda: e.observe(v, out=face))
        arm("ddz_observe_states", f"variant={v}", lambda: E.observe_states(states, None, v))
        net = G.QNet(P).to(dev)
        fq = G.FactorisedQ(net)
        arm("launch_q_features", f"planes={P}", lambda: fq.tables(face))
        arm("ddz_q_features_needed", f"planes={P}", lambda: fq.needed(e, face, gemm="mfma", hook=on_stream))
        if v:
            arm("ddz_q_shared_rows(_hashed) + ddz_q_features_rows + ddz_q_features_drows", f"variant={v} planes={P}",
                lambda: fq.needed(e, face, shared="all", hook=on_stream))
            rq = G.RoleQ({"lord": net, "down": G.QNet(P).to(dev)}, v)
            w = rq._workspace(e, face)
            arm("ddz_q_roles_rows", f"variant={v}",
                lambda: e.q_roles_rows(v, rq.net_of_role, rq.N, w["sws"], w["scap"], w["srows"], w["srep"], w["sseg"], w["slot"]))
        arm("ddz_q_first_fwd + ddz_q_first_bwd", f"planes={P}", lambda: net.forward_fused(face, actions).sum().backward())
        arm("ddz_q_stage_fwd + ddz_q_stage_bwd", f"faces planes={P}", lambda: net.forward_stage(face, actions).sum().backward())
        arm("ddz_q_stage_fwd + ddz_q_stage_bwd", f"rows variant={v}",
            lambda: net._stage(states=states, ids=zero_ids, index=None, table=table, variant=v).sum().backward())
    assert e.status() == 0
    print(f"{count[0]} arms walked")


if __name__ == "__main__":
    main()
