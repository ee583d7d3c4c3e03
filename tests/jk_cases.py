"""The roots and references on which the evaluator kernels of the joker-kicker build (libddz_hip_jk.so, BatchedEnv(native_
joker_kickers=True)) are compared with their restatements, shared by tests/test_jk_evaluators_cpu.py (the coverage conditions,
without a device) and tests/test_gpu_jk_evaluators.py (the kernels, exactly).  Every reference is computed once per process,
cached by its arguments and never written.
  roots   the 18 "jk leads" of playout_cases.build(jk=True): endings of 13 to 20 cards.  In the nine "actor" tables the root actor
          holds a quad or two adjacent triples with both jokers (one joker-kicker row in the root list), in the nine "second"
          tables the next player holds them and meets the row at depth 1.  The state bytes do not depend on the rule set:
          the plain build searches the same roots against the plain references
  OWN     one more root for the hidden forms of the per-world trees (k_guided<true>, k_search<true>): the lord holds 7777, both
          jokers and a 9 against two cards each (3 8 | 4 8).  Nothing beats the 9 in any world -- no bomb is left in the pool
          of 3 4 8 8 --, so behind the lead of the 9 both opponents pass and the lord's second turn, at depth 3, is the same
          lead in every world: a list of ten moves whose last is 7777 with the jokers, the move that ends the game.  On the 18
          roots those trees meet a joker-kicker row at the root only: the pool of a "second" table rarely deals the next player
          all of it.  It is searched alone, with OWN_BUDGET iterations: enough for the ten moves of a node three plies down
Seed, table-id base, budget, trees and salts are guided_cases'; every role takes part."""
import numpy as np

import gismcts_reference as gir
import guided_cases as gc
import guided_reference as gr
import ismcts_reference as ir
import playout_cases as pc
import playout_hidden_cases as hc
import search_reference as sr

SEED, GID_BASE = gc.SEED, gc.GID_BASE
BUDGET, TREES, SALTS = gc.BUDGET, gc.TREES, gc.SALTS
MODES = ("reference", "sides")
ROLES = 0b111
NA_PLAIN = pc.NA_PLAIN                    # ids from here on are the joker-kicker rows
SEARCH_BUDGET, SEARCH_SALT = 64, SALTS[1]  # k_search<true> and k_ismcts: 64 iterations of 2 trees
OWN_BUDGET = 300
N_ROOTS = 18

_states, _refs = {}, {}


def roots(oracle):
    """states uint8 [18, 11, 16] and their names"""
    if "roots" not in _states:
        import constructed_states as cs
        with oracle.variant(jk=True):
            table = cs.Table(*oracle.action_table())
            s = pc.build(oracle, table, jk=True)["jk leads"]
            cs.check_consistent(s.states, table)
        assert s.T == N_ROOTS and [n.endswith("second") for n in s.names] == [False, True] * 9
        _states["roots"] = (s.states.copy(), list(s.names))
    return _states["roots"]


def own_root():
    """states uint8 [1, 11, 16]: OWN of the header"""
    if "own" not in _states:
        _states["own"] = hc._table({4: 4, pc.BJ: 1, pc.CJ: 1, 6: 1}, {0: 1, 5: 1}, {1: 1, 5: 1}, role=1)
    return _states["own"]


def ref(oracle, kernel, jk, own=False, **kw):
    """the traced reference of one call of `kernel` ("guided", "gismcts", "search", "ismcts") under the rule set `jk`, on the
    18 roots or (own) on OWN alone with OWN_BUDGET iterations: guided / gismcts -> (visits, wins, totals, launches, items) with
    the hashed evaluator, search / ismcts -> (visits, wins, totals, items)"""
    k = (kernel, jk, own, tuple(sorted(kw.items())))
    if k not in _refs:
        st = own_root() if own else roots(oracle)[0]
        common = dict(trees=TREES, seed=SEED, gid_base=GID_BASE, trace=True, **kw)
        with oracle.variant(jk=jk):
            if kernel == "guided":
                _refs[k] = gr.guided(oracle, st, OWN_BUDGET if own else BUDGET, gr.hash_leaf, roles=ROLES if kw.get("hidden") else 0b111,
                                     **common)
            elif kernel == "gismcts":
                _refs[k] = gir.gismcts(oracle, st, OWN_BUDGET if own else BUDGET, gr.hash_leaf, roles=ROLES, **common)
            elif kernel == "search":
                _refs[k] = sr.search(oracle, st, OWN_BUDGET if own else SEARCH_BUDGET, roles=ROLES, **common)
            else:
                assert kernel == "ismcts"
                _refs[k] = ir.ismcts(oracle, st, OWN_BUDGET if own else SEARCH_BUDGET, roles=ROLES, **common)
    return _refs[k]


# the settings of every instance the GPU module launches: {instance: (kernel, [(own, kwargs)])}
INSTANCES = {
    "k_guided<false>": ("guided", [(False, dict(mode=m, salt=s, hidden=False)) for m in MODES for s in SALTS]),
    "k_guided<true>": ("guided", [(own, dict(mode=m, salt=s, hidden=True)) for own in (False, True) for m in MODES for s in SALTS]),
    "k_gismcts": ("gismcts", [(False, dict(mode=m, salt=s)) for m in MODES for s in SALTS]),
    "k_search<true>": ("search", [(own, dict(mode=m, salt=SEARCH_SALT, hidden=True)) for own in (False, True) for m in MODES]),
    "k_ismcts": ("ismcts", [(False, dict(mode=m, salt=SEARCH_SALT)) for m in MODES]),
}


def items_of(want):
    return want[-1]


def jk_children(items, by_id):
    """[(item, parent's node number, child's node number)] of every child made by a joker-kicker row.  by_id: the tree keys
    its children by canonical id (specs v2 / v4); otherwise by list index, and the id stands beside the trace's "expand"
    (specs v1 / v3)"""
    out = []
    for it in items:
        if by_id:
            out += [(it, p, x) for p, nd in enumerate(it.nodes) for a, x in nd.kids.items() if a >= NA_PLAIN]
        else:
            out += [(it, r["expand"][0], it.nodes[r["expand"][0]].kids[r["expand"][1]]) for r in it.iters
                    if r["expand"] is not None and r["expand_id"] >= NA_PLAIN]
    return out


def coverage(items, by_id):
    """{condition: how many joker-kicker children meet it} over the traces of one instance's references: every count must be
    positive for the exact comparison of that instance to say anything about the joker-kicker rows.  A child is descended
    through by a later iteration where its node number stands in that iteration's selected path: its stored move was
    re-applied from the root (specs v1 / v3) or it was found again under its parent by its count word (specs v2 / v4)"""
    kids = jk_children(items, by_id)
    assert len({(id(it), x) for it, _, x in kids}) == len(kids)
    return {
        "a joker-kicker row expanded at the root": sum(p == 0 for _, p, _ in kids),
        "a joker-kicker row expanded below the root": sum(p != 0 for _, p, _ in kids),
        "a joker-kicker child that is terminal": sum(it.nodes[x].terminal for it, _, x in kids),
        "a joker-kicker child descended through by a later iteration": sum(any(x in r["path"] for r in it.iters) for it, _, x in kids),
    }


def instance_coverage(oracle, instance):
    """coverage() over every setting of `instance` under the joker-kicker rule set"""
    kernel, settings = INSTANCES[instance]
    items = [it for own, kw in settings for it in items_of(ref(oracle, kernel, True, own, **kw))]
    return coverage(items, by_id=kernel in ("gismcts", "ismcts"))
