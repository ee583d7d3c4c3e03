"""CPU: the roots and references of tests/jk_cases.py, on which tests/test_gpu_jk_evaluators.py compares the evaluator kernels
of the joker-kicker build with their restatements.  Every coverage condition of every instance is asserted here from the
references' traces alone, so that the exact comparison on the device cannot pass without a joker-kicker row having been
expanded at the root and below it, ended a game, and been descended through again."""
import numpy as np
import pytest

import constructed_states as cs
import gismcts_cases as gcs
import jk_cases as jc
import playout_hidden_reference as phr
import playout_reference as pr

PER_WORLD_HIDDEN = ("k_guided<true>", "k_search<true>")      # tree c on world c alone: below the root only on jk_cases.OWN


def test_roots(oracle):
    st, names = jc.roots(oracle)
    own = jc.own_root()
    assert st.shape == (jc.N_ROOTS, 11, 16) and st.dtype == np.uint8 and own.shape == (1, 11, 16)
    assert st[:, :3, 15].astype(int).sum(1).tolist() == [13, 16, 15, 20] * 4 + [13, 16] and own[0, :3, 15].tolist() == [2, 7, 2]
    assert cs.running(st).all() and cs.running(own).all()
    n_plain = pr.root_lists(oracle, st)[0]
    with oracle.variant(jk=True):
        table = cs.Table(*oracle.action_table())
        cs.check_consistent(own, table)
        n, off, ids = pr.root_lists(oracle, st)
        n_own, _, ids_own = pr.root_lists(oracle, own)
        for states in (st, own):                   # every root is inside the hidden-hand domain and takes part
            W, part, bad = phr.worlds(oracle, states, jc.TREES, jc.SEED, jc.GID_BASE, jc.SALTS[0], jc.ROLES)
            assert part.all() and not bad.any()
    assert n.tolist() == [14, 13, 24, 23] * 4 + [14, 13] and n_plain.tolist() == [13, 13, 23, 23] * 4 + [13, 13]
    assert n.max() < jc.BUDGET and n.max() < jc.SEARCH_BUDGET          # every root is expanded fully
    for t in range(jc.N_ROOTS):                     # one joker-kicker row, the last, in the lists of the "actor" tables alone
        row = ids[off[t]:off[t + 1]]
        assert (row >= jc.NA_PLAIN).sum() == (0 if names[t].endswith("second") else 1) and (row[:-1] < jc.NA_PLAIN).all()
    assert n_own.tolist() == [14] and pr.root_lists(oracle, own)[0].tolist() == [13] and (ids_own >= jc.NA_PLAIN).sum() == 1
    assert len({s.tobytes() for s in st}) == jc.N_ROOTS


def _setting_coverage(oracle, instance, own, kw):
    kernel = jc.INSTANCES[instance][0]
    return jc.coverage(jc.items_of(jc.ref(oracle, kernel, True, own, **kw)), by_id=kernel in ("gismcts", "ismcts"))


@pytest.mark.parametrize("instance", list(jc.INSTANCES))
def test_coverage(oracle, instance):
    """every condition of the instance over its settings; and setting by setting, but for the per-world trees of the hidden
    forms on the 18 roots, which meet the row below the root in a few settings only: jk_cases.OWN is there for them.
    Measured (at the root, below, terminal, descended through again; summed over the settings):
    k_guided<false> 72 195 195 154, k_guided<true> 80 9 9 84, k_gismcts 72 6 6 72, k_search<true> 40 4 4 41, k_ismcts 36 4 4 36"""
    cover = jc.instance_coverage(oracle, instance)
    print(instance, cover)
    assert all(v > 0 for v in cover.values()), (instance, cover)
    for own, kw in jc.INSTANCES[instance][1]:
        c = _setting_coverage(oracle, instance, own, kw)
        if instance in PER_WORLD_HIDDEN and not own:
            c = {k: v for k, v in c.items() if "at the root" in k or "descended" in k}
        assert all(v > 0 for v in c.values()), (instance, own, kw, c)
        items = jc.items_of(jc.ref(oracle, jc.INSTANCES[instance][0], True, own, **kw))
        assert len(items) == (1 if own else jc.N_ROOTS) * jc.TREES                     # every table takes part, tree by tree
        at_root = [it for it, p, _ in jc.jk_children(items, "ismcts" in instance) if p == 0]
        assert len(at_root) == len(items) if own else len(at_root) == len(items) // 2   # the "actor" tables' trees


def test_the_own_root_meets_the_row_three_plies_down(oracle):
    """behind the lead of the 9 both opponents pass in every world: the joker-kicker child below the root is the lord's
    second move, a node of depth 4, and ends the game for the lord"""
    for instance in PER_WORLD_HIDDEN:
        kernel, settings = jc.INSTANCES[instance]
        for own, kw in settings:
            if not own:
                continue
            items = jc.items_of(jc.ref(oracle, kernel, True, own, **kw))
            below = [(it, x) for it, p, x in jc.jk_children(items, False) if p != 0]
            assert below and all(it.nodes[x].depth == 4 and it.nodes[x].terminal and it.nodes[x].winner == 1 for it, x in below)


@pytest.mark.parametrize("instance", list(jc.INSTANCES))
def test_the_rule_sets_differ_on_these_roots(oracle, instance):
    """the plain references the GPU module holds the plain build to are other numbers: a library handle of the wrong build
    cannot pass either comparison"""
    kernel, settings = jc.INSTANCES[instance]
    for own, kw in (settings[0], settings[-1]):
        want, plain = jc.ref(oracle, kernel, True, own, **kw), jc.ref(oracle, kernel, False, own, **kw)
        assert not np.array_equal(want[0], plain[0]) and not np.array_equal(want[1], plain[1])
        assert want[2][2] == 0 and plain[2][2] == 0                                    # nothing unfinished in either
        assert not jc.jk_children(jc.items_of(plain), kernel in ("gismcts", "ismcts"))


def test_the_guided_ismcts_paths_on_these_roots(oracle):
    """gismcts_cases.coverage on the four v4 references: everything but the long list, which no root here has"""
    items = [it for own, kw in jc.INSTANCES["k_gismcts"][1] for it in jc.items_of(jc.ref(oracle, "gismcts", True, own, **kw))]
    cover = gcs.coverage(items, jc.BUDGET)
    assert [k for k, v in cover.items() if not v] == ["an expansion index >= 64 in a list > 64"]
