"""A byte-level model of the teacher pass (teacher spec v1: include/ddz_env.h ddz_teach, the workspace in the header of
doudizhu-rl_amd/csrc/ddz_teach.h) and the constructed call scripts it is held to, shared by tests/test_teach_cpu.py (the model
against dqn_glue.TeacherAssembler, against targets worked out with fractions.Fraction from plain Python lists, and the scripts
against the shape they declare) and tests/test_gpu_teach.py (the kernels against the model, bit for bit, on rings filled with
a sentinel).  numpy only; written from the header text, not from the kernels.

  TeachModel    per ring the count and the five fields with a written-mask per entry (return_cases.Ring: the rings are the
                return recorder's), hdr int64 [8] of the last call.  label() is a plain loop over the tables in ascending order
                and over j; the rings' order and overflow rule is return_cases.ReturnModel.store, the one statement of it.
  teach_ret     the f32 target: np.float32(reward) * (np.float32(int64 2 num - p) / np.float32(int64 p))
  CASES         name -> a function that builds the script (namespace: T, stride, capacity, present, counts0, calls, declares).
                State rows are arbitrary bytes from a seeded generator with the role byte set per table: the pass does not
                validate a game.  ids[t, j] = (7 t + 13 j + 1 + 31 c) modulo the action count.  `declares` says what the script
                is meant to exercise; tests/test_teach_cpu.py holds every script to it.
"""
import types

import numpy as np

import return_cases as mc
from return_cases import N_ACTIONS, REWARDS, ROLE_BYTE, ROW_BYTES, SENTINEL, Ring, ring_layout   # noqa: F401

BLOCK_TABLES = mc.BLOCK_TABLES               # tables per block of the scan; the scan takes 256 blocks per trip
WS_REGIONS = ("rank", "blk", "hdr")
HDR_WRITTEN = (0, 1, 2, 4, 5, 6)             # hdr[3] and hdr[7] are not written
GUIDED_ONE = 1024


def ws_layout(T):
    """{region: byte offset} of the per-call scratch and its size (each region 256-aligned)"""
    nb = (T + BLOCK_TABLES - 1) // BLOCK_TABLES
    off, o = {}, 0
    for name, n in zip(WS_REGIONS, (T * 16, nb * 16, 64)):
        off[name] = o
        o = mc._align(o + n)
    return off, o


def teach_ret(reward, num, d, scale):
    p = np.int64(d) * np.int64(scale)
    top = np.int64(2) * np.int64(num) - p
    return np.float32(reward) * (np.float32(top) / np.float32(p))


class TeachModel:
    store = mc.ReturnModel.store             # (rings, cap, hdr, last_E, emitted: the fields it uses)

    def __init__(self, T, capacity, rings_present, counts0):
        self.T, self.cap = int(T), int(capacity)
        self.hdr = np.zeros(8, np.int64)
        self.rings = [Ring(self.cap, counts0[k]) if rings_present[k] else None for k in range(3)]
        self.last_E = [0, 0, 0]
        self.emitted = []                    # every emit ever made, dropped or not: (role, table, a0, ret, togo)

    def label(self, call):
        states = np.asarray(call.states, np.uint8).reshape(self.T, ROW_BYTES)
        stride = call.num.shape[1]
        emits = ([], [], [])
        for t in range(self.T):
            k = int(states[t, ROLE_BYTE])
            if k > 2 or (call.active is not None and not call.active[t]) or not (call.trained >> k) & 1 or call.counts[t] <= 0:
                continue
            for j in range(min(int(call.counts[t]), stride)):
                d = int(call.den[t, j]) if call.den is not None else int(call.den_const)
                if call.unknown is not None:
                    d -= int(call.unknown[t, j])
                if d < call.min_den:
                    continue
                ret = teach_ret(call.reward[k], int(call.num[t, j]), d, call.scale)
                emits[k].append((t, states[t].copy(), int(call.ids[t, j]), ret, 0))
        self.store(emits)


def model_of(case):
    return TeachModel(case.T, case.capacity, case.present, case.counts0)


# ---- building blocks ------------------------------------------------------------------------------------------------------------
def _ids(T, stride, c):
    t, j = np.arange(T, dtype=np.int64)[:, None], np.arange(stride, dtype=np.int64)[None, :]
    return ((7 * t + 13 * j + 1 + 31 * c) % N_ACTIONS).astype(np.int32)


def _call(rng, T, stride, c, role, counts, num, den=None, den_const=0, unknown=None, scale=1, min_den=1, active=None, trained=7):
    states = rng.integers(0, 256, (T, ROW_BYTES), dtype=np.uint8)
    states[:, ROLE_BYTE] = role
    arr = lambda x: None if x is None else np.array(np.broadcast_to(np.asarray(x, np.int32), (T, stride)))   # noqa: E731
    return types.SimpleNamespace(states=states, counts=np.array(np.broadcast_to(np.asarray(counts, np.int32), (T,))),
                                 ids=_ids(T, stride, c), num=arr(num), den=arr(den), den_const=int(den_const),
                                 unknown=arr(unknown), scale=int(scale), min_den=int(min_den),
                                 active=None if active is None else np.asarray(active, np.uint8), trained=int(trained),
                                 reward=REWARDS)


def _case(T, stride, cap, calls, present=(1, 1, 1), counts0=(0, 0, 0), **declares):
    return types.SimpleNamespace(T=T, stride=stride, capacity=cap, present=tuple(bool(x) for x in present),
                                 counts0=tuple(int(x) for x in counts0), calls=calls, declares=declares)


def visits_script(seed, T, stride, cap, n_calls, lengths=None, p_zero=0.3, role_pool=(0, 1, 2), p_active=None, trained=(7,),
                  min_den=1, present=(1, 1, 1), counts0=(0, 0, 0), **declares):
    """n_calls calls with a den array (visit counts 0 .. 40, zero with probability p_zero) and num in 0 .. den: lengths[t] moves
    per table (None: seeded, 0 .. stride), roles seeded from role_pool, an active mask of density p_active (None: no mask)"""
    rng = np.random.default_rng(seed)
    calls = []
    for c in range(n_calls):
        counts = rng.integers(0, stride + 1, T) if lengths is None else np.asarray(lengths)[(np.arange(T) + c) % len(lengths)]
        den = rng.integers(1, 41, (T, stride)) * (rng.random((T, stride)) >= p_zero)
        num = (rng.random((T, stride)) * (den + 1)).astype(np.int64).clip(0, den)
        active = None if p_active is None else rng.random(T) < p_active
        calls.append(_call(rng, T, stride, c, rng.choice(role_pool, T), counts, num, den, min_den=min_den, active=active,
                           trained=trained[c % len(trained)]))
    return _case(T, stride, cap, calls, present, counts0, **declares)


CASES = {}


def _register(name, fn, *args, **kw):
    assert name not in CASES
    CASES[name] = lambda: fn(*args, **kw)


# ---- the smallest; two and three scan blocks with a ragged tail; a second trip of the block-total scan ---------------------------------
def smallest():
    rng = np.random.default_rng(10)
    calls = [_call(rng, 1, 1, c, [c % 3], [1], [[c]], den_const=3) for c in range(4)]
    return _case(1, 1, 4, calls, blocks=1, emits_per_call=1, den_null=True)


_register("one-table-one-move", smallest)
_register("two-blocks-257", visits_script, 20, 257, 8, 4096, 3, blocks=2, some_skip=True)
_register("three-blocks-700", visits_script, 30, 700, 8, 8192, 3, blocks=3, some_skip=True)
# 65,540 tables = 257 blocks: two trips of the scan's 256-block loop, the second one of a single block with four tables
_register("second-scan-trip", visits_script, 40, 65537 + 3, 2, 4096, 2, p_zero=0.5, blocks=257, overflow=True)

# ---- the chunk and lane-group boundaries of the rank prefix: lists of 0 .. 497 moves at stride 512 -------------------------------------
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 128, 497)
_register("list-lengths-stride512", visits_script, 50, 2 * len(LENGTHS), 512, 4096, 3, lengths=LENGTHS, p_zero=0.35,
          lengths_seen=LENGTHS)
_register("list-lengths-all-qualify", visits_script, 51, len(LENGTHS) + 3, 512, 4096, 2, lengths=LENGTHS, p_zero=0.0,
          lengths_seen=LENGTHS)


# ---- tables that qualify nowhere between tables that emit; counts above the stride and below zero ----------------------------------------
def holes():
    """every third table has no visited move at all (den 0 everywhere), every fourth an empty list"""
    case = visits_script(60, 40, 16, 2048, 3, p_zero=0.2)
    for call in case.calls:
        call.den[::3] = 0
        call.counts[::4] = 0
    case.declares = dict(dead_tables_between=True)
    return case


def counts_out_of_range():
    case = visits_script(70, 30, 8, 1024, 3, p_zero=0.1)
    for c, call in enumerate(case.calls):
        call.counts[c::5] = 8 + 1 + c * 1000            # clamped to the stride
        call.counts[(c + 2)::5] = -1 - c * 7            # a negative size: the table takes no part
    case.declares = dict(counts_above_stride=True, counts_negative=True)
    return case


_register("dead-tables-between", holes)
_register("counts-clamped-and-negative", counts_out_of_range)


# ---- a total per table instead of a den array; unknown; min_den ------------------------------------------------------------------------
def den_const(seed, T, stride, K, min_den=1, with_unknown=False, **declares):
    rng = np.random.default_rng(seed)
    calls = []
    for c in range(3):
        unknown = rng.integers(0, K + 1, (T, stride)) if with_unknown else None
        left = K - (unknown if with_unknown else 0)
        num = (rng.random((T, stride)) * (left + 1)).astype(np.int64).clip(0, None)
        calls.append(_call(rng, T, stride, c, rng.integers(0, 3, T), rng.integers(0, stride + 1, T), num, None, K, unknown,
                           min_den=min_den))
    return _case(T, stride, 2048, calls, den_null=True, **declares)


_register("den-const-8", den_const, 80, 50, 12, 8)
_register("unknown-to-zero", den_const, 90, 50, 12, 4, with_unknown=True, d_values=(0, 1, 4))
_register("unknown-around-min-den-2", den_const, 100, 50, 12, 4, min_den=2, with_unknown=True, d_values=(0, 1, 2, 3))
_register("min-den-3-visits", visits_script, 110, 60, 10, 2048, 3, min_den=3, p_zero=0.1, d_values=(2, 3, 4))


# ---- the arithmetic: int64 products, num unvalidated, f32 rounding of the integers ----------------------------------------------------------
def guided_scale():
    """scale 1024 with visit counts of 1 .. 4 million and num above 2^30: 2 num does not fit int32, and where the visits exceed
    2^21 neither does p"""
    rng = np.random.default_rng(120)
    T, stride = 12, 6
    den = rng.integers(1_060_000, 4_000_000, (T, stride))
    num = rng.integers(2 ** 30 + 1, np.minimum(den * GUIDED_ONE, 2 ** 31 - 2) + 1)
    calls = [_call(rng, T, stride, c, rng.integers(0, 3, T), rng.integers(1, stride + 1, T), num, den, scale=GUIDED_ONE)
             for c in range(2)]
    return _case(T, stride, 256, calls, int32_overflow=True)


def num_edges():
    """num = 0 (ret = -reward), num = p (ret = +reward), num below 0 and above p (not validated: ret outside the rewards)"""
    rng = np.random.default_rng(130)
    T, stride = 9, 6
    den = rng.integers(1, 30, (T, stride))
    num = np.stack([np.zeros(T, np.int64), den[:, 1], -den[:, 2] - 3, 2 * den[:, 3] + 1, den[:, 4] // 2, den[:, 5] * 5], 1)
    calls = [_call(rng, T, stride, c, np.arange(T) % 3, np.full(T, stride), num, den) for c in range(2)]
    return _case(T, stride, 256, calls, num_edges=True)


def big_p():
    """p between 2^24 and 2^31: neither 2 num - p nor p is a f32, both conversions round"""
    rng = np.random.default_rng(140)
    T, stride = 16, 8
    den = rng.integers(2 ** 24 + 1, 2 ** 31 - 1, (T, stride)) | 1
    num = (rng.random((T, stride)) * den).astype(np.int64) | 1
    calls = [_call(rng, T, stride, c, rng.integers(0, 3, T), rng.integers(1, stride + 1, T), num, den) for c in range(2)]
    return _case(T, stride, 512, calls, inexact_f32=True)


_register("scale-1024-num-above-2^30", guided_scale)
_register("num-0-p-and-outside", num_edges)
_register("p-above-2^24", big_p)

# ---- role byte above 2, active mask, untrained roles, a NULL ring for a trained role ------------------------------------------------------
_register("role-byte-above-2", visits_script, 150, 60, 8, 1024, 3, role_pool=(0, 3, 1, 2, 255, 4), role_above_2=True)
_register("active-mask", visits_script, 160, 300, 8, 4096, 3, p_active=0.6, blocks=2, masked=True)
_register("untrained-roles", visits_script, 170, 60, 8, 1024, 4, trained=(0b010, 0b101, 0b000, 0b110), untrained=True)
_register("null-ring", visits_script, 180, 60, 8, 1024, 3, present=(1, 0, 1), null_drops=True)


# ---- the ring exactly full, overflowing in one call, wrapping across calls ---------------------------------------------------------------
def ring_fill(E_lord, cap, counts0=(0, 0, 0), T=30, stride=16, **declares):
    """every call gives the lord's ring exactly E_lord emits (whole lists of lord tables, all qualifying) and the farmers' rings
    a few"""
    rng = np.random.default_rng(190 + E_lord)
    calls = []
    for c in range(3):
        role = np.where(np.arange(T) % 3 == 0, 1, np.where(np.arange(T) % 3 == 1, 0, 2))
        counts = np.zeros(T, np.int64)
        lord = np.flatnonzero(role == 1)
        left = E_lord
        for t in lord:                                   # E_lord moves over the lord tables, at most `stride` each
            counts[t] = min(stride, left)
            left -= counts[t]
        assert left == 0
        counts[role != 1] = rng.integers(0, 3, int((role != 1).sum()))
        den = rng.integers(1, 20, (T, stride))
        calls.append(_call(rng, T, stride, c, role, counts, (rng.random((T, stride)) * (den + 1)).astype(np.int64), den))
    return _case(T, stride, cap, calls, counts0=counts0, E_lord=E_lord, **declares)


_register("E-equals-capacity", ring_fill, 48, 48)
_register("E-capacity+1", ring_fill, 8, 7, counts0=(3, 5, 0))
_register("E-much-above-capacity", ring_fill, 150, 7, counts0=(3, 7 * 3 + 6, 0), overflow=True)
_register("wrap-across-calls", visits_script, 200, 5, 4, 7, 6, p_zero=0.2, counts0=(0, 5, 7 * 3 + 6), wraps=True)
