#!/usr/bin/env python3
"""Generate tests/golden/cfr_reference.npz -- runs ONLY where the reference is checked out (DDZ_REFERENCE, default
/root/reference).

The REFERENCE's own server/CFR.py is imported and executed: deal() and initiate_game() (ChanceGameState, VanillaCFR.run(8)).
What had to be supplied for the import: module `envi` with r.get_moves -- the native module is absent from the reference; the
stand-in is the CPU oracle's legal list (ascending canonical id, pass first when following) as Python lists of ints, because
CFR.py compares actions with `!= [0] * 15`.

The fixture is data only: per case the arguments of initiate_game (sizes by seat, the pool, the first seat to move, the
combination to beat and its owner), deal()'s output, and the strategy the reference returns at every ROOT information set
(every hand the first mover can hold) as rows (case, hand, action, sigma).  max_deviation = the largest absolute difference
between those values and tests/cfr_reference.py, printed here and stored; the reference walks its deals in the arbitrary
order of a Python set, the restatement in ascending deal order.
"""
import os
import sys
import time
import types

import numpy as np

sys.dont_write_bytecode = True
REF = os.environ.get("DDZ_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REF, "server"))

from oracle import oracle  # noqa: E402

import cfr_cases as cc  # noqa: E402
import cfr_reference as cr  # noqa: E402

ROWS = oracle.action_table()[0]


def _get_moves(hand, last):
    last = None if not any(last) else np.array(list(last) + [0], np.int8)
    ids = oracle.legal(np.array(list(hand) + [0], np.int8), last)
    return [[int(x) for x in ROWS[a, :15]] for a in ids]


_envi = types.ModuleType("envi")
_envi.r = types.SimpleNamespace(get_moves=_get_moves)
sys.modules["envi"] = _envi

import CFR  # noqa: E402  (reference)


def vec(cards):
    """rank values 3..17 -> 15 counts"""
    out = [0] * 15
    for c in cards:
        out[c - 3] += 1
    return out


# (name, sizes [lord, down, up], pool cards, first seat to move, cards to beat, seat that owns them)
CASES = [
    ("six ranks 2/2/2, lord leads", [2, 2, 2], [3, 5, 7, 9, 11, 13], 0, [], 0),
    ("8 9 10 J and both jokers 1/1/4, up leads", [1, 1, 4], [8, 9, 10, 11, 16, 17], 2, [], 2),
    ("a pair, down leads", [1, 2, 1], [3, 3, 5, 7], 1, [], 1),
    ("a triple 2/2/1, lord leads", [2, 2, 1], [4, 4, 4, 9, 13], 0, [], 0),
    ("a triple with kicker 1/4/1, down leads", [1, 4, 1], [6, 6, 6, 8, 10, 14], 1, [], 1),
    ("a bomb 3/1/1, up leads", [3, 1, 1], [6, 6, 6, 6, 14], 2, [], 2),
    ("the rocket 2/1/1, down leads", [2, 1, 1], [3, 4, 16, 17], 1, [], 1),
    ("down follows the lord's single", [1, 2, 1], [5, 8, 11, 15], 1, [4], 0),
    ("up follows the lord's pair behind a pass", [2, 1, 2], [7, 7, 9, 9, 13], 2, [5, 5], 0),
    ("lord follows down's single behind a pass", [2, 2, 2], [4, 6, 6, 10, 12, 15], 0, [9], 1),
    ("lord follows up's pair", [3, 1, 2], [5, 5, 8, 8, 16, 17], 0, [4, 4], 2),
    ("down follows a bomb", [1, 3, 1], [3, 9, 9, 9, 9], 1, [7, 7, 7, 7], 2),
    ("1/1/1, up leads", [1, 1, 1], [3, 8, 15], 2, [], 2),
    ("1/2/3 with a pair, lord leads", [1, 2, 3], [4, 4, 7, 7, 12, 14], 0, [], 0),
]


def main():
    rec = {k: [] for k in ("case", "hand", "action", "sigma")}
    arg = {k: [] for k in ("sizes", "pool", "first", "beat", "owner", "deals")}
    deal_case, deal_rows = [], []
    worst = 0.0
    for c, (name, sizes, pool, first, beat, owner) in enumerate(CASES):
        pool, beat = vec(pool), vec(beat)
        t0 = time.time()
        deals = CFR.deal(sizes[:], pool[:])
        sigma = CFR.initiate_game(sizes[:], pool[:], first, beat[:], owner)
        want = cr.solve(oracle, cc.case_state(oracle, ROWS, sizes, pool, first, beat, owner))
        assert want.n > 0, name
        n_root = 0
        for key, row in sigma.items():
            parts = key.split()
            if len(parts) != 1:
                continue
            hand = tuple(int(ch) for ch in parts[0])
            ids, mine = want.sigma_all[(first, hand, ())]
            assert len(row) == len(ids), (name, key)
            for (a, p), aid, q in zip(row.items(), ids, mine):
                action = [int(ch) for ch in a]
                assert action == [int(x) for x in ROWS[aid, :15]], (name, key, a)
                rec["case"].append(c)
                rec["hand"].append(hand)
                rec["action"].append(action)
                rec["sigma"].append(p)
                worst = max(worst, abs(p - q))
            n_root += 1
        for k, v in zip(("sizes", "pool", "first", "beat", "owner", "deals"), (sizes, pool, first, beat, owner, len(deals))):
            arg[k].append(v)
        for d in deals:
            deal_case.append(c)
            deal_rows.append(d)
        print(f"{name}: {len(deals)} deals, {want.nodes} nodes, {want.infosets} information sets, {n_root} root sets, "
              f"{time.time() - t0:.1f} s, deviation so far {worst:.3g}")
    out = os.path.join(HERE, "cfr_reference.npz")
    np.savez_compressed(
        out, names=np.array([c[0] for c in CASES]), sizes=np.array(arg["sizes"], np.int8), pool=np.array(arg["pool"], np.int8),
        first=np.array(arg["first"], np.int8), beat=np.array(arg["beat"], np.int8), owner=np.array(arg["owner"], np.int8),
        n_deals=np.array(arg["deals"], np.int32), deal_case=np.array(deal_case, np.int16), deals=np.array(deal_rows, np.int8),
        case=np.array(rec["case"], np.int16), hand=np.array(rec["hand"], np.int8), action=np.array(rec["action"], np.int8),
        sigma=np.array(rec["sigma"], np.float64), max_deviation=np.array(worst, np.float64))
    print(f"{out}: {len(rec['sigma'])} entries, max deviation {worst:.3g}")


if __name__ == "__main__":
    main()
