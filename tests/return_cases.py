"""A byte-level model of the return recorder (return spec v1: include/ddz_env.h ddz_mc_before / ddz_mc_after, the layout in the
header of doudizhu-rl_amd/csrc/ddz_returns.h) and the constructed call scripts it is held to, shared by
tests/test_return_recorder_cpu.py (model against dqn_glue.ReturnAssembler, against returns computed from plain Python lists of
decisions, and the scripts against the shape they are meant to have) and tests/test_gpu_return_recorder.py (the kernels against
the model, bit for bit, on rings filled with a sentinel).  numpy only; written from the header text, not from the kernels.

  ReturnModel   per table a log of L entries (rows u8 [176], act int32, who u8 {role, ordinal}), cnt u8 {n, c[3]}, lost u32; hdr
                int64 [8] of the last after(); per ring the count and the five fields with a written-mask per entry.  before() /
                after() are plain loops over the tables in ascending order; emit g of a call into a ring goes to entry
                (count + g - drop) % capacity, the first drop = max(0, E - capacity) emits are not written, the count moves by
                E - drop; hdr[k] = count - drop, hdr[4 + k] = drop (a NULL ring: its count reads as 0 and hdr[4 + k] = E).
  discounted    the f32 return after `togo` multiplications by f32(gamma)
  CASES         name -> a function that builds the script (namespace: T, log_cap, capacity, present, counts0, gamma, calls and
                what the script declares about itself).  State rows are arbitrary bytes from a seeded generator with the role
                byte set per table: the recorder does not validate a game.  chosen = (7 t + 1 + 31 c) modulo the action count.
"""
import types

import numpy as np

from constructed_states import F_META, M_ROLE, NFIELDS, ROW

ROW_BYTES = NFIELDS * ROW                    # 176
ROLE_BYTE = F_META * ROW + M_ROLE
N_ACTIONS = 13527
BLOCK_TABLES = 256                           # tables per block of the scan; the scan takes 256 blocks per trip
SENTINEL = 0xA5
REWARDS = (0.5, 2.0, 0.25)                   # distinct per role: a reward taken from another role's entry shows
RING_FIELDS = ("count", "s0", "a0", "ret", "table", "togo")
WS_REGIONS = ("rows", "act", "who", "cnt", "lost", "rank", "blk", "hdr")


def _align(x):
    return (x + 255) // 256 * 256


def ws_layout(T, L):
    """{region: byte offset} of the workspace and its size (each region 256-aligned)"""
    nb = (T + BLOCK_TABLES - 1) // BLOCK_TABLES
    sizes = (T * L * ROW_BYTES, T * L * 4, T * L * 2, T * 4, T * 4, T * 16, nb * 16, 64)
    off, o = {}, 0
    for name, n in zip(WS_REGIONS, sizes):
        off[name] = o
        o = _align(o + n)
    return off, o


def ring_layout(cap):
    """{field: byte offset} of a ring and its size: the fields in RING_FIELDS order, each 256-aligned"""
    sizes = (8, cap * ROW_BYTES, cap * 4, cap * 4, cap * 4, cap)
    off, o = {}, 0
    for name, n in zip(RING_FIELDS, sizes):
        off[name] = o
        o = _align(o + n)
    return off, o


def discounted(g, gamma, togo):
    g, gamma = np.float32(g), np.float32(gamma)
    for _ in range(int(togo)):
        g = np.float32(g * gamma)
    return g


class Ring:
    def __init__(self, cap, count):
        self.cap, self.count = cap, int(count)
        self.s0 = np.zeros((cap, ROW_BYTES), np.uint8)
        self.a0 = np.zeros(cap, np.int32)
        self.ret = np.zeros(cap, np.float32)
        self.table = np.zeros(cap, np.int32)
        self.togo = np.zeros(cap, np.uint8)
        self.written = np.zeros(cap, bool)

    def image(self, fill=SENTINEL):
        """the ring's bytes: `fill` everywhere, the count, and the fields of the entries ever written"""
        off, nbytes = ring_layout(self.cap)
        img = np.full(nbytes, fill, np.uint8)
        img[:8] = np.array([self.count], np.int64).view(np.uint8)
        w = self.written
        for name in RING_FIELDS[1:]:
            a = getattr(self, name)
            width = a.dtype.itemsize * (ROW_BYTES if a.ndim == 2 else 1)
            region = img[off[name]: off[name] + self.cap * width].reshape(self.cap, width)
            region[w] = a[w].reshape(-1, 1).view(np.uint8).reshape(-1, width) if a.ndim == 1 else a[w]
        return img


class ReturnModel:
    def __init__(self, T, L, capacity, rings_present, counts0):
        self.T, self.L, self.cap = int(T), int(L), int(capacity)
        self.rows = np.zeros((T, L, ROW_BYTES), np.uint8)
        self.act = np.zeros((T, L), np.int32)
        self.who = np.zeros((T, L, 2), np.uint8)
        self.cnt = np.zeros((T, 4), np.uint8)
        self.lost = np.zeros(T, np.uint32)
        self.hdr = np.zeros(8, np.int64)
        self.rings = [Ring(self.cap, counts0[k]) if rings_present[k] else None for k in range(3)]
        self.last_E = [0, 0, 0]              # emits of the last after() per ring, the dropped ones included
        self.emitted = []                    # every emit ever made, dropped or not: (role, table, a0, ret, togo)

    def before(self, states, chosen, active, trained):
        states = np.asarray(states, np.uint8).reshape(self.T, ROW_BYTES)
        role = states[:, ROLE_BYTE].astype(np.int64)
        take = role <= 2
        if active is not None:
            take &= np.asarray(active).astype(bool)
        take &= ((trained >> np.minimum(role, 2)) & 1).astype(bool)
        for t in np.flatnonzero(take):
            k, n = int(role[t]), int(self.cnt[t, 0])
            c = int(self.cnt[t, 1 + k])
            if n < self.L:
                self.rows[t, n], self.act[t, n], self.who[t, n] = states[t], chosen[t], (k, c)
                self.cnt[t, 0] = n + 1
            else:
                self.lost[t] = min(int(self.lost[t]) + 1, 2 ** 32 - 1)
            self.cnt[t, 1 + k] = min(c + 1, 255)

    def after(self, done, r, reward, gamma):
        emits = ([], [], [])
        for t in np.flatnonzero(np.asarray(done)):
            lord_won = int(r[t]) < 0
            for p in range(int(self.cnt[t, 0])):
                k, j = int(self.who[t, p, 0]), int(self.who[t, p, 1])
                togo = int(self.cnt[t, 1 + k]) - 1 - j
                g = reward[k] if lord_won == (k == 1) else -reward[k]      # the two farmers are one side
                emits[k].append((int(t), self.rows[t, p].copy(), int(self.act[t, p]), discounted(g, gamma, togo), togo))
            self.cnt[t] = 0
        self.store(emits)

    def store(self, emits):
        """one call's emits per ring, each (table, row, a0, ret, togo) in emit order, into the rings; hdr as the scan leaves it"""
        for k in range(3):
            E = len(emits[k])
            self.last_E[k] = E
            self.emitted += [(k, t, a, ret, togo) for t, _, a, ret, togo in emits[k]]
            ring = self.rings[k]
            drop = max(0, E - self.cap)
            if ring is None:                 # a role without a ring drops everything (its count reads as 0)
                self.hdr[k], self.hdr[4 + k] = -drop, E
                continue
            self.hdr[k], self.hdr[4 + k] = ring.count - drop, drop
            now = np.zeros(self.cap, bool)
            for g in range(drop, E):
                e = (ring.count + g - drop) % self.cap
                assert not now[e], "two emits of one call into one entry"
                now[e] = True
                ring.table[e], ring.s0[e], ring.a0[e], ring.ret[e], ring.togo[e] = emits[k][g]
            ring.written |= now
            ring.count += E - drop

    def apply(self, call):
        if call.kind == "before":
            self.before(call.states, call.chosen, call.active, call.trained)
        else:
            self.after(call.done, call.r, call.reward, call.gamma)


def model_of(case):
    return ReturnModel(case.T, case.log_cap, case.capacity, case.present, case.counts0)


# ---- building blocks ------------------------------------------------------------------------------------------------------------
def _rows(rng, T, role):
    rows = rng.integers(0, 256, (T, ROW_BYTES), dtype=np.uint8)
    rows[:, ROLE_BYTE] = role
    return rows


def _before(rng, T, role, active, trained, c):
    chosen = ((7 * np.arange(T, dtype=np.int64) + 1 + 31 * c) % N_ACTIONS).astype(np.int32)
    return types.SimpleNamespace(kind="before", states=_rows(rng, T, role), chosen=chosen,
                                 active=None if active is None else np.asarray(active, np.uint8), trained=int(trained))


def _after(rng, T, done, gamma):
    return types.SimpleNamespace(kind="after", done=np.asarray(done, np.uint8), r=rng.integers(-1, 2, T).astype(np.int8),
                                 reward=REWARDS, gamma=float(gamma))


def _case(T, L, cap, calls, gamma, present=(1, 1, 1), counts0=(0, 0, 0), **more):
    return types.SimpleNamespace(T=T, log_cap=L, capacity=cap, present=tuple(bool(x) for x in present),
                                 counts0=tuple(int(x) for x in counts0), gamma=float(gamma), calls=calls, **more)


def play(seed, T, L, cap, iters, gamma=1.0, trained=7, present=None, counts0=(0, 0, 0), p_done=0.15, p_active=None,
         role_pool=(0, 1, 2), finish=None, **more):
    """a seeded script of `iters` iterations (before, after): table t's actor cycles through role_pool from a seeded start, a
    table finishes with probability p_done (finish: {iteration: tables} that finish for certain), active is a seeded mask with
    density p_active (None: no mask, and every fourth iteration of a masked script too); the last after() finishes every table"""
    rng = np.random.default_rng(seed)
    pool = np.asarray(role_pool)
    start = rng.integers(0, len(pool), T)
    calls = []
    for it in range(iters):
        role = pool[(start + it) % len(pool)]
        active = None if p_active is None or it % 4 == 3 else rng.random(T) < p_active
        calls.append(_before(rng, T, role, active, trained, it))
        done = rng.random(T) < p_done if it < iters - 1 else np.ones(T, bool)
        for t in (finish or {}).get(it, ()):
            done[t] = True
        calls.append(_after(rng, T, done, gamma))
    present = [(trained >> k) & 1 for k in range(3)] if present is None else present
    return _case(T, L, cap, calls, gamma, present, counts0, **more)


CASES = {}


def _register(name, fn, *args, **kw):
    assert name not in CASES
    CASES[name] = lambda: fn(*args, **kw)


# ---- the smallest, two blocks, a second trip of the block-total scan -----------------------------------------------------------------
for _g in (1.0, 0.95, 0.0):
    _register(f"smallest-gamma{_g}", play, 100 + int(_g * 100), 3, 6, 16, 7, gamma=_g, p_done=0.3)
_register("two-blocks", play, 200, 300, 5, 2048, 6, gamma=0.95, p_done=0.1, finish={1: (255, 256, 299), 3: (0, 255, 256, 299)})
# 65,537 tables = 257 blocks: two trips of the scan's 256-block loop, the second one of a single block with a single table
# (the last after() finishes every table: about 40,000 emits per ring of 4,096 entries)
_register("second-scan-trip", play, 300, 65537, 2, 4096, 3, gamma=0.95, p_done=0.02,
          finish={0: (0, 255, 256, 65535, 65536), 1: (65280, 65536)})


# ---- the log overflows ------------------------------------------------------------------------------------------------------------------
def log_overflow():
    """log_cap 2, five decisions of the lord on table 0 (lost 3, the two logged entries have togo 4 and 3) while tables 1 and 2
    alternate between two roles (table 1: lost 3 too, across roles)"""
    rng = np.random.default_rng(400)
    T = 3
    calls = [_before(rng, T, np.array([1, (it % 2) * 2, it % 3]), None, 7, it) for it in range(5)]
    calls.append(_after(rng, T, np.ones(T), 0.95))
    calls += [_before(rng, T, np.array([1, 1, 1]), None, 7, 9), _after(rng, T, np.ones(T), 0.95)]     # lost stays, the logs restart
    return _case(T, 2, 16, calls, 0.95, lost=(3, 3, 3), togo0=(4, 3))


_register("log-overflow", log_overflow)


# ---- the ring wraps and overflows ---------------------------------------------------------------------------------------------------------
_register("ring-wrap-capacity7", play, 500, 5, 4, 7, 9, gamma=0.95, p_done=0.3, counts0=(0, 5, 7 * 3 + 6))


def ring_overflow(E_lord, cap):
    """one after() in which the lord's ring takes E_lord emits and the farmers' rings fewer than capacity: T tables, one logged
    decision each, the first E_lord tables the lord's"""
    rng = np.random.default_rng(600 + E_lord)
    T = 300
    role = np.where(np.arange(T) < E_lord, 1, np.where(np.arange(T) < E_lord + cap - 1, 0, 2))
    role = role[rng.permutation(T)]
    calls = [_before(rng, T, role, None, 7, 0), _after(rng, T, role != 2, 0.95),
             _before(rng, T, role, None, 7, 1), _after(rng, T, np.ones(T), 0.95)]
    return _case(T, 3, cap, calls, 0.95, counts0=(3, cap - 2, 0), E_first=(cap - 1, E_lord, 0))


_register("ring-overflow-E=capacity+1", ring_overflow, 8, 7)
_register("ring-overflow-E>>capacity", ring_overflow, 250, 7)

# ---- a NULL ring for a role with logged entries, a role byte of 3, an active mask, one and two trained roles -------------------------------
_register("null-ring", play, 700, 40, 6, 64, 6, gamma=0.95, p_done=0.2, present=(1, 0, 1))
_register("role-byte-3", play, 800, 40, 6, 64, 6, gamma=1.0, p_done=0.2, role_pool=(0, 3, 1, 2, 3))
_register("active-mask", play, 900, 300, 6, 512, 8, gamma=0.95, p_done=0.15, p_active=0.6)
_register("one-trained-role", play, 1000, 40, 6, 64, 8, gamma=0.95, trained=0b010)
_register("two-trained-roles", play, 1100, 40, 6, 64, 8, gamma=1.0, trained=0b101)


# ---- one role with 54 decisions, and finished tables whose log is empty ---------------------------------------------------------------------
def long_run():
    """table 0: 54 decisions of the lord in a log of 54 (togo 53 .. 0); table 1 cycles through the roles (18 each); table 2 is
    inactive throughout and finishes with an empty log"""
    rng = np.random.default_rng(1200)
    T = 3
    calls = [_before(rng, T, np.array([1, it % 3, 2]), np.array([1, 1, 0]), 7, it) for it in range(54)]
    calls.append(_after(rng, T, np.ones(T), 0.95))
    return _case(T, 54, 128, calls, 0.95)


_register("long-run-54", long_run)


def empty_log():
    """every table finishes before any decision was logged, then a played iteration, then tables of an untrained role finish"""
    rng = np.random.default_rng(1300)
    T = 20
    role = np.arange(T) % 3
    calls = [_after(rng, T, np.ones(T), 1.0), _before(rng, T, role, None, 0b011, 0), _after(rng, T, np.ones(T), 1.0)]
    return _case(T, 4, 32, calls, 1.0)


_register("empty-log", empty_log)
