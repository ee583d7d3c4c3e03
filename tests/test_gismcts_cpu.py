"""CPU: tests/gismcts_reference.py (search spec v4, guided ISMCTS, on the oracle) pinned to spec v2 -- with "spec v1's playout
from the leaf" as the evaluator the new spec IS ismcts_reference's, visit for visit -- its leaf rows checked against the oracle
stepped along the traced paths from the root with the iteration's world, and the coverage conditions of the roots
tests/test_gpu_gismcts.py compares on, so that test cannot pass vacuously.  Plus the exported symbols and the host-side
argument checks of ddz_gismcts_*."""
import importlib
import os
import re

import numpy as np
import pytest

import constructed_states as cs
import gismcts_cases as gcs
import gismcts_reference as gir
import guided_reference as gr
import ismcts_reference as ir
import playout_hidden_reference as phr
import playout_reference as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(oracle):
    return cs.Table(*oracle.action_table())


@pytest.fixture(scope="module")
def roots(oracle, table):
    return gcs.build(oracle, table)


_refs = {}


def hashed(oracle, roots, mode, salt):
    """the reference of the GPU test's exact comparison, computed once: (visits, wins, totals, launches, items)"""
    k = (mode, salt)
    if k not in _refs:
        _refs[k] = gir.gismcts(oracle, roots, gcs.BUDGET, gr.hash_leaf, trees=gcs.TREES, mode=mode, seed=gcs.SEED,
                               gid_base=gcs.GID_BASE, salt=salt, roles=gcs.ROLES, trace=True)
    return _refs[k]


def test_value_is_v3s_unit_with_v2s_count():
    v = gir.value(700, 3, 9, 0.7)
    ln = np.float32(np.log(9.0))
    assert v.dtype == np.float32
    assert v == (np.float32(700) / np.float32(3)) * np.float32(2.0 ** -10) + np.float32(0.7) * np.sqrt((np.float32(2) * ln) / np.float32(3))
    nodes = [ir.Node(0), ir.Node(1), ir.Node(1)]
    nodes[0].kids = {5: 1, 9: 2}
    for nd, (V, W, A) in zip(nodes[1:], ((2, 1500, 7), (2, 548, 3))):
        nd.V, nd.W, nd.A = V, W, A
    j, vals, took_max, tied = gir.select([5, 9], nodes[0], nodes, "sides", False, 0.7)      # away from the root's side: V * 1024 - W
    assert took_max and not tied and vals[0] == gir.value(548, 2, 7, 0.7) and vals[1] == gir.value(1500, 2, 3, 0.7) and j == 1
    j, vals, took_max, _ = gir.select([5, 9], nodes[0], nodes, "reference", False, 0.7)     # the opponent's step takes the minimum of W
    assert not took_max and vals[0] == gir.value(1500, 2, 7, 0.7) and vals[1] == gir.value(548, 2, 3, 0.7)
    assert j == int(np.argmin(vals))


@pytest.mark.parametrize("mode", ("reference", "sides"))
def test_v4_with_v1s_playout_is_v2(oracle, roots, mode):
    """the evaluator is spec v1's playout from the leaf, scored for the LEAF's actor: the leaf row holds the iteration's world
    and the draws are domain 7 on (gid, c << 16 | i, ply), so this is k_ismcts's playout: visits are v2's, wins 1024 times v2's"""
    kw = dict(trees=gcs.TREES, mode=mode, seed=gcs.SEED, gid_base=gcs.GID_BASE, salt=3, roles=gcs.ROLES)
    v2 = ir.ismcts(oracle, roots, gcs.BUDGET, **kw)
    assert v2[2][2] == 0 and v2[0].sum() > 0                     # every playout of the old spec finished: inside the domain
    leaf = gr.v1_playout_leaf(oracle, gcs.TREES, seed=gcs.SEED, gid_base=gcs.GID_BASE, salt=3)
    v4 = gir.gismcts(oracle, roots, gcs.BUDGET, leaf, **kw)
    assert np.array_equal(v4[0], v2[0])
    assert np.array_equal(v4[1].astype(np.int64), v2[1].astype(np.int64) * gir.ONE)
    assert v4[2][1] == v2[2][1] and v4[2][3] == v2[2][3] and v4[2][2] == 0      # iterations, nodes; nothing unfinished
    live = list(gcs.LIVE)
    assert (v4[0].sum(1)[live] == gcs.BUDGET * gcs.TREES).all()
    assert not v4[0][[x for x in range(len(roots)) if x not in live]].any()


def test_leaf_rows_are_the_oracle_stepped_along_the_path_in_the_iterations_world(oracle, roots):
    """every launch's leaf row, all 176 bytes, is a fresh oracle env set to the item's root with world c * budget + i as the
    opponents' hands and stepped along the traced indices; items without a pending leaf have an all-zero row and need 0"""
    visits, wins, totals, launches, items = hashed(oracle, roots, "reference", gcs.SALTS[0])
    W, part, bad = phr.worlds(oracle, roots, gcs.TREES * gcs.BUDGET, gcs.SEED, gcs.GID_BASE, gcs.SALTS[0], gcs.ROLES)
    assert part.tolist() == [t in gcs.LIVE for t in range(len(roots))] and bad.tolist() == [t == gcs.OUTSIDE for t in range(len(roots))]
    slots = {it.t * gcs.TREES + it.c: it for it in items}
    seen, worlds_seen = 0, set()
    for i, (rows, need) in enumerate(launches):
        assert rows.shape == (len(roots) * gcs.TREES, 11, 16) and need.shape == (len(roots) * gcs.TREES,)
        for k in range(len(need)):
            rec = slots[k].iters[i] if k in slots else None
            if rec is None or not rec["pending"]:
                assert need[k] == 0 and not rows[k].any()
                continue
            it = slots[k]
            world = W[it.t, it.c * gcs.BUDGET + i]
            assert np.array_equal(world, rec["world"])
            env = oracle.OracleEnv(1, seed=gcs.SEED, gid_base=gcs.GID_BASE + it.t)
            env.state.reshape(1, 11, 16)[:] = phr.with_world(roots[it.t], world)
            for j in rec["choices"]:
                env.legal()
                _, _, illegal, _ = env.step(pr.STEP_CHOICE, np.array([j], np.int32), auto_reset=False)
                assert not illegal.any()
            want = env.state.reshape(11, 16)
            assert need[k] == 1 and np.array_equal(rows[k], want), (i, k)
            m = rows[k, cs.F_META]
            assert m[cs.M_DONE] == 0 and m[pr.M_WINNER] == 0xFF and m[pr.M_DEALT] == 1 and m[3] == 0
            assert np.array_equal(m[8:12], roots[it.t][cs.F_META, 8:12])              # the root's episode
            assert cs.meta_ply(rows[k:k + 1])[0] == cs.meta_ply(roots[it.t][None])[0] + len(rec["choices"])
            assert rows[k, 0:3, 15].tolist() == rows[k, 0:3, :15].sum(1).tolist()     # the count bytes are the hands' sizes
            worlds_seen.add((it.t, world.tobytes()))
            seen += 1
    assert seen > gcs.BUDGET and len(worlds_seen) > 3 * len(gcs.LIVE)                  # one tree's leaves come from many worlds


@pytest.mark.parametrize("mode", ("reference", "sides"))
def test_coverage_of_the_gpu_cases(oracle, roots, mode):
    """what the exact comparison on the device has to walk through, read from the traces of its references"""
    n_root = pr.root_lists(oracle, roots)[0]
    assert 64 < n_root[gcs.MID] < gcs.BUDGET and n_root[gcs.NOT_DEALT] == 0 and n_root[gcs.DONE] == 0
    items = []
    for salt in gcs.SALTS:
        items += hashed(oracle, roots, mode, salt)[4]
    cover = gcs.coverage(items, gcs.BUDGET)
    if mode == "sides":
        assert not cover.pop("a minimum step")                        # (the `sides` mode takes the maximum everywhere)
    assert all(cover.values()), [k for k, v in cover.items() if not v]
    assert {it.t for it in items} == set(gcs.LIVE)


def test_tree_invariants(oracle, roots):
    visits, wins, totals, launches, items = hashed(oracle, roots, "sides", gcs.SALTS[1])
    assert len(launches) == gcs.BUDGET and totals[1] == gcs.BUDGET * len(items) and totals[2] == 0
    assert (wins.astype(np.int64) <= visits.astype(np.int64) * gir.ONE).all()
    assert visits.sum(1)[list(gcs.LIVE)].tolist() == [gcs.BUDGET * gcs.TREES] * len(gcs.LIVE)
    for it in items:
        root = it.nodes[0]
        assert root.V == gcs.BUDGET == sum(it.nodes[x].V for x in root.kids.values())
        assert len(it.nodes) <= gcs.BUDGET + 1                                       # one node per iteration at most
        assert sum(r["expand"] is not None for r in it.iters) == len(it.nodes) - 1
        assert root.W == sum(r["score"] for r in it.iters)
        for nd in it.nodes[1:]:
            assert 1 <= nd.V <= nd.A <= gcs.BUDGET and 0 <= nd.W <= nd.V * gir.ONE   # available whenever visited
            if nd.terminal:
                assert not nd.kids and nd.W in (0, nd.V * gir.ONE)
        for r in it.iters:
            assert r["moves"] == len(r["choices"]) == len(r["path"]) - 1 + (r["expand"] is not None)
    assert totals[3] == sum(len(it.nodes) - 1 for it in items)
    assert totals[0] == sum(r["moves"] for it in items for r in it.iters)


def test_gismcts_symbols_exported_and_argument_checks():
    build = importlib.import_module("doudizhu-rl_amd.build")
    build.build()
    lib = importlib.import_module("doudizhu-rl_amd._lib")
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    serving = importlib.import_module("doudizhu-rl_amd.serving")
    hdr = open(os.path.join(REPO, "include", "ddz_env.h")).read()
    declared = set(re.findall(r"\b(ddz_[a-z_0-9]+)\s*\(", hdr))
    names = ("ddz_gismcts_work_bytes", "ddz_gismcts_open", "ddz_gismcts_step", "ddz_gismcts_close")
    assert set(names) <= declared
    assert "ddz_gismcts.h" in build.DEPS and os.path.exists(os.path.join(build.CSRC, "ddz_gismcts.h"))
    for name in ("guided_ismcts", "guided_ismcts_choose"):
        assert hasattr(engine.BatchedEnv, name)
    assert hasattr(serving, "guided_ismcts_act") and "guided_ismcts" in engine.Teacher.KINDS
    for jk in (False, True):
        L = lib.lib(jk=jk)
        for name in names:
            assert hasattr(L, name) and name in lib.SYMBOLS
    # ddz_guided_*'s arguments minus `hidden`
    for phase in ("open", "step", "close"):
        g, v4 = lib.SYMBOLS[f"ddz_guided_{phase}"][1], lib.SYMBOLS[f"ddz_gismcts_{phase}"][1]
        assert v4 == g[:6] + g[7:]
    L = lib.lib()
    assert L.ddz_gismcts_open(None, 1, 1, 0, 0.7, 0, 7, 512, None, 0, None) == -2                          # EHANDLE
    assert L.ddz_gismcts_step(None, 1, 1, 0, 0.7, 0, 7, 512, None, None, None, None, 0, None) == -2
    assert L.ddz_gismcts_close(None, 1, 1, 0, 0.7, 0, 7, None, 512, None, None, None, None, 0, None) == -2
    # per tree: spec v2's workspace, a 64-byte header and the stored path (SEARCH_PATH = 200 u16)
    for budget in (1, 64, 1000, 4096):
        assert L.ddz_gismcts_work_bytes(1, budget, 1) == L.ddz_ismcts_work_bytes(1, budget, 1) + 64 + 400
        assert L.ddz_gismcts_work_bytes(1, budget, 1) % 16 == 0
        assert L.ddz_gismcts_work_bytes(7, budget, 5) == 35 * L.ddz_gismcts_work_bytes(1, budget, 1)
    # budget * trees * 1024 stays below 2^31
    assert L.ddz_gismcts_work_bytes(1, 4096, 511) > 0 and L.ddz_gismcts_work_bytes(1, 4096, 512) < 0
    assert L.ddz_gismcts_work_bytes(1, 32, 65535) > 0 and L.ddz_gismcts_work_bytes(1, 32, 65536) < 0
    for bad in ((1, 0, 1), (1, 4097, 1), (1, 64, 0), (1, 64, 65537), (-1, 64, 1)):
        assert L.ddz_gismcts_work_bytes(*bad) < 0
