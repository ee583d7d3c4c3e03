"""CFR spec v1 restated on the CPU oracle: what ddz_cfr / ddz_cfr_choose must give, independent of the engine.
The reference's final_card / initiate_game / VanillaCFR (server/CFR.py) with everything it leaves to chance pinned.  numpy
and the oracle module (handed in) only; every floating-point value is an IEEE double (a Python float), every operation is
written out on its own, in the order the spec names.

  seats      the reference's player numbers: 0 lord, 1 down, 2 up = role (seat + 1) % 3; the turn order is seat 0, 1, 2
  domain     running; left[0] + left[1] + left[2] <= 6 (else n = -1, no status bit); every left >= 1, pool = deck - taken
             with 0 <= pool and sum pool = sum left, the actor's hand row inside pool (else n = -1 and status bit 6).
             left[actor] = the cards of its hand row; the other two = byte 15 of their hand rows, whose counts are not read
  deals      CFR.py:deal's order: per rank ascending, (lord's count, down's count) ascending; every deal weighs 1 / D
  forest     built breadth-first over all deals at once: the roots in deal order, children appended in parent order
  info set   (mover, the mover's hand in the deal, the actions from the root): at most one node per deal
  iteration  reaches top-down, values bottom-up, regrets added per information set in ascending node index (= deal order),
             then sigma_a = max(R_a, 0) / S (S = the positive R_a added in action order), 1 / n where S <= 0
solve() also says how large everything was (the capacities of csrc/ddz_cfr.h are sized from these) and how the kernel's two
open-addressing tables probe (their coverage condition; nothing computed depends on them)."""
import numpy as np

ROW, NFIELDS = 16, 11
F_HAND0, F_HIST0, F_RECENT0, F_TAKEN, F_META = 0, 3, 6, 9, 10
M_ROLE, M_DONE, M_DEALT = 0, 1, 6
DECK = np.array([4] * 13 + [1, 1], np.int64)
STRIDE = 16                # DDZ_CFR_STRIDE
MAX_CARDS = 6              # DDZ_CFR_MAX_CARDS
MAX_DEALS, MAX_ACTIONS, MAX_DEPTH = 90, 8, 24
MAX_NODES, MAX_INFOSETS, MAX_PAIRS, MAX_HISTORIES = 32768, 8192, 8192, 4096
MAX_ITERATIONS = 64
STATUS_DOMAIN, STATUS_CAPACITY = 64, 128
DOMAIN_CHOOSE = 8


def deal(card_n, remainder):
    """CFR.py:393-423: every distinct assignment of `remainder` to three seats of sizes card_n, in its order"""
    out = []

    def rec(n, rem, cards):
        if sum(rem) == 0:
            out.append(cards)
            return
        i = next(k for k in range(15) if rem[k] > 0)
        r = list(rem)
        r[i] = 0
        for a in range(min(rem[i], n[0]) + 1):
            for b in range(min(rem[i] - a, n[1]) + 1):
                c = rem[i] - a - b
                if c <= n[2]:
                    nxt = [list(x) for x in cards]
                    nxt[0][i] += a
                    nxt[1][i] += b
                    nxt[2][i] += c
                    rec([n[0] - a, n[1] - b, n[2] - c], r, nxt)

    assert sum(remainder) == sum(card_n)
    rec(list(card_n), [int(x) for x in remainder], [[0] * 15 for _ in range(3)])
    return [tuple(tuple(h) for h in d) for d in out]


def hand16(hand):
    """a hand of at most 4 cards in 16 bits: nibble j = 1 + the rank of its j-th lowest card"""
    w, j = 0, 0
    for r in range(15):
        for _ in range(hand[r]):
            w |= (r + 1) << (4 * j)
            j += 1
    assert j <= 4
    return w


class Probe:
    """an open-addressing table of the kernel: slot = (key * 2654435761 mod 2^32) >> (32 - log), linear probing"""

    def __init__(self, log):
        self.log, self.slots, self.longest = log, {}, 0

    def insert(self, key):
        h = ((key * 2654435761) & 0xFFFFFFFF) >> (32 - self.log)
        steps = 0
        while h in self.slots:
            h = (h + 1) & ((1 << self.log) - 1)
            steps += 1
        self.slots[h] = key
        self.longest = max(self.longest, steps)


class Result:
    """one table: n (list size, 0 idle, -1 outside, -2 over capacity), status bits, ids / sigma of the root row, value,
    and of the whole forest: sigma_all {(seat, hand tuple, action ids tuple): (ids, [sigma])}, deals, nodes, infosets, pairs,
    histories, depth, widest level, longest member chain, longest probes"""

    def __init__(self):
        self.n, self.status, self.ids, self.sigma, self.value = 0, 0, [], [], 0.0
        self.sigma_all = {}
        self.deals = self.nodes = self.infosets = self.pairs = self.histories = self.depth = self.widest = self.members = 0
        self.probe_info = self.probe_hist = 0
        self.deal_list, self.snap = [], {}


_legal_cache = {}


def _legal(oracle, hand, last):
    k = (oracle.num_actions(), hand, last)
    if k not in _legal_cache:
        _legal_cache[k] = [int(x) for x in oracle.legal(np.array(hand + (0,), np.int8),
                                                          None if last is None else np.array(last + (0,), np.int8))]
    return _legal_cache[k]


def decode(state):
    """(running, role, left [3] by role, pool [15], actor's hand [15], last tuple or None, owner role) as the kernel reads
    a table: the opponents' count bytes are not touched"""
    s = np.asarray(state, np.uint8).reshape(NFIELDS, ROW)
    m = s[F_META]
    run = bool(m[M_DEALT]) and not m[M_DONE]
    role = int(m[M_ROLE]) if m[M_ROLE] <= 2 else 0
    hand = s[F_HAND0 + role, :15].astype(np.int64)
    left = [int(s[F_HAND0 + r, 15]) for r in range(3)]
    left[role] = int(hand.sum())
    pool = DECK - s[F_TAKEN, :15].astype(np.int64)
    prev, nxt = (role + 2) % 3, (role + 1) % 3
    last, owner = None, role
    if s[F_RECENT0 + prev, :15].any():
        last, owner = tuple(int(x) for x in s[F_RECENT0 + prev, :15]), prev
    elif s[F_RECENT0 + nxt, :15].any():
        last, owner = tuple(int(x) for x in s[F_RECENT0 + nxt, :15]), nxt
    return run, role, left, pool, hand, last, owner


def solve(oracle, state, iterations=8, rows=None):
    """CFR spec v1 for one table (uint8 [11, 16]) -> Result"""
    assert 0 <= iterations <= MAX_ITERATIONS
    res = Result()
    run, role, left, pool, hand, last, owner_role = decode(state)
    if not run:
        return res
    if sum(left) > MAX_CARDS:
        res.n = -1
        return res
    if min(left) < 1 or (pool < 0).any() or pool.sum() != sum(left) or (hand > pool).any():
        res.n, res.status = -1, STATUS_DOMAIN
        return res
    if rows is None:
        rows = oracle.action_table()[0]
    seat_of = lambda r: (r + 2) % 3
    first, owner0 = seat_of(role), seat_of(owner_role)
    sizes = [left[1], left[2], left[0]]
    deals = deal(sizes, pool)
    D = len(deals)
    res.deal_list = deals
    my_hand = tuple(int(x) for x in hand)
    root_ids = _legal(oracle, my_hand, last)

    def over():
        res.n, res.status = -2, STATUS_CAPACITY
        return res

    if D > MAX_DEALS or len(root_ids) > MAX_ACTIONS:
        return over()
    # ---- the forest, breadth-first; node arrays
    parent, act, nact, info, child0, util = [], [], [], [], [], []
    levels = []                       # (first node, end) of every level
    hist_ids = {(): 0}
    hist_probe, info_probe = Probe(13), Probe(14)
    info_key, info_n, info_ids, members = {}, [], [], []
    frontier = [(d, deals[d], last, owner0, ()) for d in range(D)]     # (deal, hands by seat, to beat, its owner, history)
    for d in range(D):
        parent.append(-1)
        act.append(0)
    depth = 0
    while frontier:
        if depth > MAX_DEPTH:
            return over()
        lo = len(nact)
        levels.append((lo, lo + len(frontier)))
        mover = (first + depth) % 3
        nxt_frontier = []
        for (d, hands, lst, owner, hist) in frontier:
            i = len(nact)
            if any(sum(h) == 0 for h in hands):
                nact.append(0)
                info.append(-1)
                child0.append(-1)
                util.append(1.0 if sum(hands[0]) == 0 else -1.0)
                continue
            ids = _legal(oracle, hands[mover], lst)
            n = len(ids)
            if n > MAX_ACTIONS or n == 0:
                return over()
            key = (hist_ids[hist], hand16(deals[d][mover]))
            if key not in info_key:
                if len(info_n) >= MAX_INFOSETS or sum(info_n) + n > MAX_PAIRS:
                    return over()
                info_key[key] = len(info_n)
                info_probe.insert((key[0] << 16) | key[1])
                info_n.append(n)
                info_ids.append((mover, deals[d][mover], hist, ids))
                members.append([])
            I = info_key[key]
            assert info_n[I] == n and info_ids[I][3] == ids
            members[I].append(i)
            nact.append(n)
            info.append(I)
            util.append(0.0)
            child0.append(len(parent))
            if len(parent) + n > MAX_NODES:
                return over()
            for a, aid in enumerate(ids):
                h2 = hist + (aid,)
                if h2 not in hist_ids:
                    if len(hist_ids) >= MAX_HISTORIES:
                        return over()
                    hist_probe.insert((hist_ids[hist] << 14 | aid) + 1)
                    hist_ids[h2] = len(hist_ids)
                row = tuple(int(x) for x in rows[aid, :15])
                parent.append(i)
                act.append(a)
                if aid != 0:
                    hs = list(hands)
                    hs[mover] = tuple(x - y for x, y in zip(hands[mover], row))
                    nxt_frontier.append((d, tuple(hs), row, mover, h2))
                elif (mover + 1) % 3 == owner:
                    nxt_frontier.append((d, hands, None, owner, h2))
                else:
                    nxt_frontier.append((d, hands, lst, owner, h2))
        frontier = nxt_frontier
        depth += 1
    N = len(nact)
    assert N == len(parent)
    res.deals, res.nodes, res.infosets, res.pairs = D, N, len(info_n), sum(info_n)
    res.histories, res.depth = len(hist_ids), len(levels)
    res.widest = max(b - a for a, b in levels)
    res.members = max(len(m) for m in members)
    res.probe_info, res.probe_hist = info_probe.longest, hist_probe.longest
    # ---- the iterations
    sigma = [[1.0 / n] * n for n in info_n]
    R = [[0.0] * n for n in info_n]
    reach = [[1.0, 1.0, 1.0] for _ in range(N)]
    u = list(util)
    value = 0.0
    I0 = info_key[(0, hand16(my_hand))]
    assert info_ids[I0][3] == root_ids
    res.snap = {0: (list(sigma[I0]), 0.0)}            # after k iterations: (the root row, value)
    for it in range(iterations):
        for dep, (lo, hi) in enumerate(levels):           # top-down: the reaches
            if dep == 0:
                continue
            pm = (first + dep - 1) % 3
            for i in range(lo, hi):
                p = parent[i]
                r = list(reach[p])
                r[pm] = r[pm] * sigma[info[p]][act[i]]
                reach[i] = r
        for dep in range(len(levels) - 1, -1, -1):        # bottom-up: the values
            lo, hi = levels[dep]
            for i in range(lo, hi):
                if nact[i] == 0:
                    continue
                s = sigma[info[i]]
                v = 0.0
                for a in range(nact[i]):
                    prod = s[a] * u[child0[i] + a]
                    v = v + prod
                u[i] = v
        for I, mem in enumerate(members):                 # the regrets, members in ascending node index
            mover = info_ids[I][0]
            for i in mem:
                ra, rb, rc = reach[i]
                cr = rb * rc if mover == 0 else ra * rc if mover == 1 else ra * rb
                for a in range(info_n[I]):
                    diff = u[child0[i] + a] - u[i]
                    reg = cr * diff
                    if mover != 0:
                        reg = -reg
                    R[I][a] = R[I][a] + reg
            S = 0.0
            for a in range(info_n[I]):
                if R[I][a] > 0:
                    S = S + R[I][a]
            for a in range(info_n[I]):
                sigma[I][a] = (max(R[I][a], 0.0) / S) if S > 0 else 1.0 / info_n[I]
        tot = 0.0
        for d in range(D):
            tot = tot + u[d]
        value = (1.0 / D) * tot
        res.snap[it + 1] = (list(sigma[I0]), value)
    for I, (mover, h, hist, ids) in enumerate(info_ids):
        res.sigma_all[(mover, h, hist)] = (ids, list(sigma[I]))
    res.n, res.ids, res.sigma, res.value = len(root_ids), list(root_ids), list(sigma[I0]), value
    return res


_solved = {}      # (state bytes, rule set) -> (iterations solved, Result): a table is solved once for every iteration count


def cfr(oracle, states, iterations=8, roles=0b111, slots=None, order=None):
    """ddz_cfr for states uint8 [T, 11, 16] -> (n int32 [T], ids int32 [T, 16], sigma float64 [T, 16], value float64 [T],
    totals int64 [4], status, results).  slots: the number of workspace slots; order: the order in which the in-domain
    tables take them (default ascending t; the device hands them out as its wavefronts arrive) -- a table without a slot
    gets n = -2 and status bit 7."""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T = len(states)
    n = np.zeros(T, np.int32)
    ids = np.full((T, STRIDE), -1, np.int32)
    sigma = np.zeros((T, STRIDE), np.float64)
    value = np.zeros(T, np.float64)
    totals = np.zeros(4, np.int64)
    status, results, used = 0, [None] * T, 0
    rows = oracle.action_table()[0]
    for t in (range(T) if order is None else order):
        run, role = decode(states[t])[:2]
        if not run or not (roles >> role) & 1:
            results[t] = Result()
            continue
        key = (states[t].tobytes(), oracle.num_actions())
        if key not in _solved or _solved[key][0] < iterations:
            _solved[key] = (iterations, solve(oracle, states[t], iterations, rows))
        r = _solved[key][1]
        if r.n >= 0 or r.n == -2:
            if slots is not None and used >= slots:
                r = Result()
                r.n, r.status, r.snap = -2, STATUS_CAPACITY, {}
            used += 1
        results[t] = r
        n[t], status = r.n, status | r.status
        if r.n > 0:
            ids[t, :r.n], (sigma[t, :r.n], value[t]) = r.ids, r.snap[iterations]
            totals += (r.deals, r.nodes, r.infosets, r.pairs)
    return n, ids, sigma, value, totals, status, results


def draw_u(oracle, gid, seed, salt):
    """the uniform draw of ddz_cfr_choose: x * 2^-32, x = philox((gid_lo, gid_hi, 0, 8 << 16), (seed_lo ^ salt, seed_hi)).x"""
    x = oracle.philox([gid & 0xFFFFFFFF, (gid >> 32) & 0xFFFFFFFF, 0, DOMAIN_CHOOSE << 16],
                      [(seed ^ salt) & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])[0]
    return float(int(x)) * (1.0 / 4294967296.0)


def choose(oracle, n, ids, sigma, seed=0, gid_base=0, salt=0, greedy=False):
    """ddz_cfr_choose: int32 [T] canonical ids, -1 where n <= 0.  greedy: the first maximum of sigma; else the first j with
    u below the running sum of sigma in list order, falling back to the last j with sigma_j > 0"""
    out = np.full(len(n), -1, np.int32)
    for t in range(len(n)):
        k = int(n[t])
        if k <= 0:
            continue
        s = [float(x) for x in sigma[t, :k]]
        if greedy:
            j = max(range(k), key=lambda a: (s[a], -a))
        else:
            u = draw_u(oracle, gid_base + t, seed, salt)
            acc, j = 0.0, -1
            for a in range(k):
                acc = acc + s[a]
                if u < acc:
                    j = a
                    break
            if j < 0:
                pos = [a for a in range(k) if s[a] > 0]
                j = pos[-1] if pos else k - 1
        out[t] = ids[t, j]
    return out


def make_state(hand, role, left, taken, recent=None, rows=None, fill_opponents=None):
    """a running table uint8 [11, 16] for the solver: `hand` (15 counts) in the actor's row, `left` by role, `taken` (15
    counts), recent {role: action id}; fill_opponents {role: 15 counts} writes count bytes the solver must not read"""
    s = np.zeros((NFIELDS, ROW), np.uint8)
    s[F_HAND0 + role, :15] = hand
    for r in range(3):
        s[F_HAND0 + r, 15] = left[r]
    s[F_TAKEN, :15] = taken
    s[F_HIST0, :15] = taken                # (the histories are not read by the solver; a payload's taken row is their sum)
    for r, aid in (recent or {}).items():
        s[F_RECENT0 + r] = rows[aid].astype(np.uint8)
    for r, c in (fill_opponents or {}).items():
        s[F_HAND0 + r, :15] = c
    s[F_META, M_ROLE], s[F_META, 2], s[F_META, M_DEALT] = role, 0xFF, 1
    return s
