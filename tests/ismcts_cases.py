"""The calls of search spec v2 (ISMCTS) that tests/test_ismcts_cpu.py and tests/test_gpu_ismcts.py share, with their
references (tests/ismcts_reference.py, traced): each is computed once per process, cached by its arguments and never written.
  degenerate  the 7 tables of playout_hidden_cases.degenerate(), seed 13, gid base 2^32 + 5, salt 3
  games       the first 16 tables of playout_hidden_cases.game_states: table 0 is the lord's first lead, a root list of more
              than 64 entries; budget = that list + 8, so the iterations behind the list select at the root over all of it"""
import numpy as np

import ismcts_reference as ir
import playout_hidden_cases as hc
import playout_reference as pr

SEED, GID_BASE, SALT = 13, 2 ** 32 + 5, 3
SEED2, GID_BASE2 = 4, 2 ** 40 + 7                # a second stream, the high word of the counter different again
N_GAMES = 16
GRID = [(trees, mode, c) for trees in (1, 2) for mode in ("reference", "sides") for c in (0.7, 0.0)]

_refs, _states = {}, {}


def ref(oracle, key, states, budget, seed=SEED, gid_base=GID_BASE, jk=False, **kw):
    """(visits, wins, totals, items) of one call"""
    k = (key, budget, seed, gid_base, jk, tuple(sorted(kw.items())))
    if k not in _refs:
        with oracle.variant(jk=jk):
            _refs[k] = ir.ismcts(oracle, states, budget, seed=seed, gid_base=gid_base, trace=True, **kw)
    return _refs[k]


def degenerate():
    if "degenerate" not in _states:
        _states["degenerate"] = hc.degenerate()[1]
    return _states["degenerate"]


def games(oracle):
    """(states [16, 11, 16], the budget: table 0's root list + 8)"""
    if "games" not in _states:
        st = hc.game_states(oracle)[:N_GAMES]
        n = pr.root_lists(oracle, st)[0]
        assert n[0] > 64
        _states["games"] = (st, int(n[0]) + 8)
    return _states["games"]


def degenerate_ref(oracle, budget, trees=1, mode="reference", c=0.7, **kw):
    return ref(oracle, "degenerate", degenerate(), budget, trees=trees, mode=mode, c=c, salt=SALT, **kw)


def games_ref(oracle, **kw):
    st, budget = games(oracle)
    return ref(oracle, "games", st, budget, seed=hc.SEED, gid_base=hc.GID_BASE, salt=SALT, **kw)


def gpu_references(oracle):
    """the items of every reference the GPU tests compare with on the plain build (the coverage conditions read them)"""
    items = []
    for trees, mode, c in GRID:
        items += degenerate_ref(oracle, 64, trees, mode, c)[3]
    for mode in ("reference", "sides"):
        items += degenerate_ref(oracle, 300, 1, mode)[3]
    items += games_ref(oracle, trees=1)[3]
    return items


def strip_noise(states, seed=5):
    return hc.strip_opponents(states, np.random.default_rng(seed))
