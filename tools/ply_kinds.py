"""Diagnostic (CPU oracle, no GPU): which list path the plies of a random rollout take in k_rollout -- follow of a single /
pair / triple, closed-form lead, closed-form follow of another category, hybrid (closed-form round + planner tail) -- and
how long their lists are.  The split is the kernel's scalar test as tests/rollout_list_cases.py states it in numpy.
  python tools/ply_kinds.py [TABLES] [FIRST] [LAST] [EVERY]      (default 4096 tables, seed 0, iterations 200..699, every 5th)"""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import constructed_states as cs  # noqa: E402
import rollout_list_cases as rc  # noqa: E402
from oracle import oracle  # noqa: E402

T, first, last, every = (int(x) for x in (sys.argv[1:5] + ["4096", "200", "699", "5"][len(sys.argv) - 1:]))
table = cs.Table(*oracle.action_table())
env = oracle.OracleEnv(T, seed=0)
env.reset()
kinds = collections.Counter()
rows = collections.Counter()
tails = collections.Counter()
for it in range(last + 1):
    off, _, ids = env.legal()   # (the oracle steps on the lists of its last legal())
    if it >= first and (it - first) % every == 0:
        s = env.state.reshape(T, cs.NFIELDS, cs.ROW)
        n = np.diff(off)
        beat = cs.to_beat(s, table)
        role = s[:, cs.F_META, cs.M_ROLE].astype(np.int64)
        hand = s[np.arange(T), cs.F_HAND0 + role, :15].astype(np.int64)
        for t in np.flatnonzero(cs.running(s)):
            b = int(beat[t])
            cat = int(table.cat[b]) if b else 0
            n0, tail = rc.scalar_split(hand[t], cat, int(table.value[b]), int(table.length[b]))
            kind = ("follow of single / pair / triple" if 1 <= cat <= 3 else
                    ("lead" if cat == 0 else "follow of another category") + (", hybrid" if tail else ", closed form"))
            if 1 <= cat <= 3:
                n0 = int(n[t])
            else:   # the split holds on the oracle's list: the round is its first n0 ids, and without a tail all of it
                head, rest = ids[off[t]:off[t] + n0], ids[off[t] + n0:off[t + 1]]
                base = (head >= 1) & (head <= 54) if cat == 0 else (head == 0) | ((head >= 42) & (head <= 54))
                assert len(head) == n0 and np.all(base | ((head == rc.ID_BIGBANG) & (not tail))), (it, t)
                assert (tail or not len(rest)) and not np.any((rest <= 54) & ((rest >= (1 if cat == 0 else 42)) | (rest == 0))), (it, t)
            kinds[kind] += 1
            rows[kind] += int(n[t])
            tails[kind] += int(n[t]) - n0
    env.step(oracle.STEP_RANDOM, auto_reset=True)
tot = sum(kinds.values())
print(f"{T} tables, seed 0, iterations {first}..{last} every {every}: {tot} plies, mean list {sum(rows.values()) / tot:.2f} rows")
for k in sorted(kinds, key=lambda k: -kinds[k]):
    print(f"  {k:42s} {100 * kinds[k] / tot:5.1f} % of plies, mean rows {rows[k] / kinds[k]:6.2f}, of them behind the round {tails[k] / kinds[k]:6.2f}")
