#!/usr/bin/env python3
"""Size the capacities of csrc/ddz_cfr.h: the largest forest of CFR spec v1 over every endgame shape (CPU only).

An endgame of at most 6 cards holds no chain, so only the ORDER of its ranks, their counts and the jokers matter.  Swept:
  pool     every composition of 3..6 cards into counts of 1..4 in ascending rank order; where the highest count (the two
           highest counts) is 1, also with that rank (those ranks) a joker (the rocket)
  sizes    every split of the cards over the three seats, at least one card each
  actor    each of the three seats
  root     a lead; a follow of a single, a pair or a triple below every rank of the pool, owned by the previous seat and by
           the one before it (the previous seat having passed)
The forest is a function of these alone (tests/cfr_reference.py, built with no iteration).  Prints the maxima and the shape
that attains each; profiles/r14_notes.md records the output.  usage: cfr_sweep.py [processes]  (default: half the CPUs, at most 16)"""
import itertools
import multiprocessing
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

FIELDS = ("deals", "nodes", "infosets", "pairs", "histories", "depth", "widest", "members")


def compositions(n):
    if n == 0:
        yield ()
        return
    for first in range(1, min(4, n) + 1):
        for rest in compositions(n - first):
            yield (first,) + rest


def pools():
    """15-count vectors: ranks 1, 2, ... (rank 0 stays free for the combination to beat), the jokers at 13 / 14"""
    for n in range(3, 7):
        for comp in compositions(n):
            forms = [[(1 + i, c) for i, c in enumerate(comp)]]
            if comp[-1] == 1:
                forms.append([(1 + i, c) for i, c in enumerate(comp[:-1])] + [(14, 1)])
                if len(comp) >= 2 and comp[-2] == 1:
                    forms.append([(1 + i, c) for i, c in enumerate(comp[:-2])] + [(13, 1), (14, 1)])
            for f in forms:
                pool = [0] * 15
                for r, c in f:
                    pool[r] = c
                yield pool


def splits(n):
    return [s for s in itertools.product(range(1, 5), repeat=3) if sum(s) == n]


def work(job):
    from oracle import oracle

    import cfr_reference as cr
    cr.MAX_NODES = cr.MAX_INFOSETS = cr.MAX_PAIRS = cr.MAX_HISTORIES = 1 << 30
    cr.MAX_DEPTH = 1 << 30
    rows = oracle.action_table()[0]
    pool, sizes = job
    best = {k: (0, None) for k in FIELDS}
    for first in range(3):
        role = (first + 1) % 3
        hand = cr.deal(list(sizes), pool)[0][first]
        left = [sizes[2], sizes[0], sizes[1]]
        roots = [("lead", {})]
        for copies in (1, 2, 3):
            beat = np.zeros(15, np.int8)
            beat[0] = copies
            aid = oracle.lookup(beat)
            roots.append((f"{copies} below, previous seat", {(role + 2) % 3: aid}))
            roots.append((f"{copies} below, the seat before", {(role + 1) % 3: aid}))
        for name, recent in roots:
            taken = cr.DECK - np.array(pool)
            st = cr.make_state(hand, role, left, taken, recent, rows)
            r = cr.solve(oracle, st, 0, rows)
            assert r.n > 0 and r.depth <= 24 and r.deals <= 90, (pool, sizes, first, name)
            for k in FIELDS:
                v = getattr(r, k)
                if v > best[k][0]:
                    best[k] = (v, (pool, sizes, first, name))
    return best


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else max(1, min(16, (os.cpu_count() or 2) // 2))
    jobs = [(p, s) for p in pools() for s in splits(sum(p))]
    print(f"{len(jobs)} (pool, sizes) pairs x 3 actors x 7 roots", flush=True)
    best = {k: (0, None) for k in FIELDS}
    with multiprocessing.Pool(procs) as pool:
        for done, b in enumerate(pool.imap_unordered(work, jobs, chunksize=4)):
            for k in FIELDS:
                if b[k][0] > best[k][0]:
                    best[k] = b[k]
            if (done + 1) % 100 == 0:
                print(done + 1, {k: best[k][0] for k in FIELDS}, flush=True)
    for k in FIELDS:
        print(f"max {k}: {best[k][0]}  at pool {best[k][1][0]} sizes (lord, down, up) {best[k][1][1]} first seat {best[k][1][2]} {best[k][1][3]}")


if __name__ == "__main__":
    main()
