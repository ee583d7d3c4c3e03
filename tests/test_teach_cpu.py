"""CPU: teacher spec v1 (include/ddz_env.h: ddz_teach) on the host -- tests/teach_cases.py's byte-level TeachModel and
dqn_glue.TeacherAssembler against each other on every constructed script, both against targets worked out from plain Python
lists with fractions.Fraction rounded once per operation, every script against the shape it declares, the sizes and layouts the
library answers, and the argument errors that are raised before a device is needed.  Every comparison is exact."""
import ctypes as C
import importlib
import struct
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import return_cases as mc
import teach_cases as tc

ROLES = ("up", "lord", "down")
REWARD_DICT = dict(zip(ROLES, tc.REWARDS))


@pytest.fixture(scope="module")
def glue():
    importlib.import_module("doudizhu-rl_amd.build").build()
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


@pytest.fixture(scope="module")
def engine(glue):
    return importlib.import_module("doudizhu-rl_amd.engine")


@pytest.fixture(scope="module")
def built():
    """every script, built once and left unchanged"""
    return {name: make() for name, make in tc.CASES.items()}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _t(x):
    return None if x is None else torch.from_numpy(x)


# ---- the model against the host statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_model_equals_the_assembler(glue, built, name):
    case = built[name]
    m = tc.model_of(case)
    for i, call in enumerate(case.calls):
        before = len(m.emitted)
        m.label(call)
        asm = glue.TeacherAssembler(REWARD_DICT, [bool((call.trained >> k) & 1) for k in range(3)])
        out = asm.label(_t(call.states), _t(call.counts), _t(call.ids), _t(call.num), _t(call.den), call.den_const,
                        _t(call.unknown), call.scale, call.min_den, _t(call.active))
        order = np.argsort(out["role"].numpy(), kind="stable")               # per ring, in emit order
        want = m.emitted[before:]
        assert len(order) == len(want), f"call {i}"
        for key, col in (("role", 0), ("table", 1), ("a0", 2), ("togo", 4)):
            assert out[key].numpy()[order].tolist() == [e[col] for e in want], f"call {i}: {key}"
        assert np.array_equal(_bits(out["ret"].numpy()[order]), _bits([e[3] for e in want])), f"call {i}: ret"
        assert np.array_equal(out["s0"].numpy()[order], call.states[[e[1] for e in want]]), f"call {i}: s0"


# ---- the model against the definition ---------------------------------------------------------------------------------------------------
def _f32(x):
    """the f32 nearest to the rational x (ties to even): one rounding, done by struct on an exactly representable double or, where
    the double itself would round, by comparing the two neighbouring f32 values as fractions"""
    lo = struct.unpack("f", struct.pack("f", float(x)))[0]                  # close; then walk to the nearest
    cands = {lo, float(np.nextafter(np.float32(lo), np.float32(np.inf))), float(np.nextafter(np.float32(lo), np.float32(-np.inf)))}
    best = min(cands, key=lambda c: (abs(Fraction(c) - x), int(np.float32(c).view(np.uint32)) & 1))
    return Fraction(best)


def _definition(call, T, stride):
    """emits per ring from plain lists: (table, a0, ret as a Fraction that is a f32)"""
    out = ([], [], [])
    role = call.states[:, tc.ROLE_BYTE].tolist()
    counts, ids, num = call.counts.tolist(), call.ids.tolist(), call.num.tolist()
    den = None if call.den is None else call.den.tolist()
    unknown = None if call.unknown is None else call.unknown.tolist()
    active = None if call.active is None else call.active.tolist()
    for t in range(T):
        k = role[t]
        if k > 2 or not (call.trained >> k) & 1 or (active is not None and not active[t]) or counts[t] <= 0:
            continue
        for j in range(min(counts[t], stride)):
            d = (call.den_const if den is None else den[t][j]) - (0 if unknown is None else unknown[t][j])
            if d < call.min_den:
                continue
            p = d * call.scale
            value = _f32(_f32(Fraction(2 * num[t][j] - p)) / _f32(Fraction(p)))
            out[k].append((t, ids[t][j], _f32(Fraction(float(np.float32(call.reward[k]))) * value)))
    return out


@pytest.mark.parametrize("name", [n for n in tc.CASES if n != "second-scan-trip"])
def test_model_equals_the_definition(built, name):
    case = built[name]
    m = tc.model_of(case)
    for i, call in enumerate(case.calls):
        before = len(m.emitted)
        m.label(call)
        got = m.emitted[before:]
        want = _definition(call, case.T, case.stride)
        assert [len(w) for w in want] == m.last_E, f"call {i}"
        flat = [(k, t, a, r) for k in range(3) for t, a, r in want[k]]
        assert [(e[0], e[1], e[2]) for e in got] == [(k, t, a) for k, t, a, _ in flat], f"call {i}"
        assert [Fraction(float(e[3])) for e in got] == [r for *_, r in flat], f"call {i}: ret"
        assert all(e[4] == 0 for e in got)


def test_rounding_helper():
    assert _f32(Fraction(1, 3)) == Fraction(float(np.float32(1) / np.float32(3)))
    assert _f32(Fraction(2 ** 24 + 1)) == 2 ** 24 and _f32(Fraction(2 ** 24 + 3)) == 2 ** 24 + 4      # ties to even
    assert _f32(Fraction(-(2 ** 31) + 129)) == Fraction(float(np.float32(np.int64(-(2 ** 31) + 129))))


# ---- every script has the shape it declares ---------------------------------------------------------------------------------------------
def _d(call):
    d = (np.full(call.num.shape, call.den_const, np.int64) if call.den is None else call.den.astype(np.int64))
    return d - (0 if call.unknown is None else call.unknown)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_script_shape(built, name):
    case = built[name]
    dec = case.declares
    T, stride, cap = case.T, case.stride, case.capacity
    assert len(case.calls) >= 2 or T > 60000                 # several calls: the counts carry over
    m = tc.model_of(case)
    E, drops, counts_before = [], [], []
    for call in case.calls:
        assert call.states.shape == (T, tc.ROW_BYTES) and call.counts.shape == (T,) and call.num.shape == (T, stride)
        assert call.ids.shape == (T, stride) and all(x is None or x.shape == (T, stride) for x in (call.den, call.unknown))
        assert 0 <= call.ids.min() and call.ids.max() < tc.N_ACTIONS
        counts_before.append([None if r is None else r.count for r in m.rings])
        m.label(call)
        E.append(list(m.last_E))
        drops.append(m.hdr[4:7].tolist())
    assert len(set(tc.REWARDS)) == 3
    assert any(sum(e) for e in E)
    if "blocks" in dec:
        assert (T + 255) // 256 == dec["blocks"] and (dec["blocks"] == 1 or T % 256)
        if dec["blocks"] > 1:       # every block holds tables that emit
            for call in case.calls[:1]:
                live = (call.counts > 0) & (call.states[:, tc.ROLE_BYTE] <= 2)
                assert all(live[b * 256:(b + 1) * 256].any() for b in range(dec["blocks"]))
    if dec.get("emits_per_call"):
        assert all(sum(e) == dec["emits_per_call"] for e in E)
    if dec.get("some_skip"):
        assert any((c.counts == 0).any() for c in case.calls)
    if "lengths_seen" in dec:
        assert stride == 512 and set(dec["lengths_seen"]) <= set(case.calls[0].counts.tolist())
        assert set(dec["lengths_seen"]) >= {0, 1, 15, 16, 17, 63, 64, 65, 128, 497}
    if dec.get("dead_tables_between"):
        call = case.calls[0]
        dead = ((_d(call) >= call.min_den) & (np.arange(stride)[None, :] < call.counts[:, None])).sum(1) == 0
        assert dead[1:-1].any() and (~dead[:-2] & dead[1:-1]).any() and (dead[1:-1] & ~dead[2:]).any()
        assert ((call.counts > 0) & dead).any() and (call.counts == 0).any()
    if dec.get("counts_above_stride"):
        assert any((c.counts > stride).any() for c in case.calls)
    if dec.get("counts_negative"):
        assert any((c.counts < 0).any() for c in case.calls)
    if dec.get("den_null"):
        assert all(c.den is None and c.den_const >= 1 for c in case.calls)
    else:
        assert all(c.den is not None for c in case.calls)
    if "d_values" in dec:
        seen = set(np.unique(np.concatenate([_d(c).ravel() for c in case.calls])).tolist())
        assert set(dec["d_values"]) <= seen and min(dec["d_values"]) < case.calls[0].min_den <= max(dec["d_values"])
        assert case.calls[0].min_den in seen
    if dec.get("int32_overflow"):
        assert all(c.scale == 1024 for c in case.calls) and (case.calls[0].num > 2 ** 30).all()
        assert (_d(case.calls[0]) * 1024 > 2 ** 31).any()
    if dec.get("num_edges"):
        call = case.calls[0]
        p = _d(call)
        assert (call.num == 0).any() and (call.num == p).any() and (call.num < 0).any() and (call.num > p).any()
        rets = {abs(float(e[3])) / tc.REWARDS[e[0]] for e in m.emitted}
        assert 1.0 in rets and max(rets) > 1.0
    if dec.get("inexact_f32"):
        p = _d(case.calls[0])
        assert (p > 2 ** 24).all() and (p.astype(np.float32).astype(np.int64) != p).any()
    if dec.get("role_above_2"):
        assert any((c.states[:, tc.ROLE_BYTE] > 2).any() for c in case.calls)
    if dec.get("masked"):
        assert all(c.active is not None and 0 < c.active.sum() < T for c in case.calls)
    if dec.get("untrained"):
        assert {c.trained for c in case.calls} >= {0b010, 0b101, 0}
    if dec.get("null_drops"):
        k = case.present.index(False)
        assert all(c.trained >> k & 1 for c in case.calls) and all(e[k] > 0 and d[k] == e[k] for e, d in zip(E, drops))
    if "E_lord" in dec:
        assert all(e[1] == dec["E_lord"] for e in E)
        assert (dec["E_lord"] == cap) == (name == "E-equals-capacity")
    if dec.get("overflow"):
        assert any(e[k] > cap and d[k] == e[k] - cap for e, d in zip(E, drops) for k in range(3) if case.present[k])
    if dec.get("wraps"):
        assert any(c % cap for c in case.counts0) and all(r.count > cap + c0 for r, c0 in zip(m.rings, case.counts0) if c0)
    if T > 60000:
        assert T >= 65537 + 3 and stride == 2 and (T + 255) // 256 > 256


# ---- sizes, layouts, argument errors --------------------------------------------------------------------------------------------------------
def test_sizes_and_layouts(engine):
    L = engine._lib.lib()
    for T in (1, 3, 256, 257, 700, 4096, 65540):
        off, nbytes = tc.ws_layout(T)
        assert L.ddz_teach_ws_bytes(T) == nbytes == engine.teach_ws_bytes(T) and nbytes % 256 == 0
        got = (C.c_int64 * 3)()
        assert L.ddz_teach_ws_layout(T, got) == 0 and [off[f] for f in tc.WS_REGIONS] == list(got)
        assert engine.teach_ws_layout(T) == off
    assert tc.ring_layout(7) == mc.ring_layout(7)                                # the return recorder's rings


def test_library_argument_errors(engine):
    L = engine._lib.lib()
    assert L.ddz_teach_ws_bytes(0) < 0 and L.ddz_teach_ws_bytes((1 << 30) + 1) < 0
    assert L.ddz_teach_ws_layout(0, (C.c_int64 * 3)()) == -1 and L.ddz_teach_ws_layout(4, None) == -1
    buf, rings, reward = (C.c_int64 * 64)(), (C.c_void_p * 3)(), (C.c_float * 3)(50, 100, 50)
    assert L.ddz_teach(None, buf, buf, 4, buf, None, 8, None, 1, 1, None, 7, buf, 512, rings, 0, 64, reward, None) == -2
    for bad in (0, -3):
        with pytest.raises(ValueError):
            engine.teach_ws_bytes(bad)
        with pytest.raises(ValueError):
            engine.teach_ws_layout(bad)


def test_host_argument_errors(glue, engine, monkeypatch):
    Teacher = engine.Teacher
    for make in (lambda: Teacher("minimax"), lambda: Teacher("playout"), lambda: Teacher("search"),
                 lambda: Teacher("playout", n_playouts=2, wins=None), lambda: Teacher("search", budget=8, depth=3),
                 lambda: Teacher("guided", budget=8), lambda: Teacher("playout", n_playouts=2, evaluator=lambda s: None),
                 lambda: Teacher("playout", n_playouts=2, roles=0b010), lambda: Teacher("solve", roles=9, hidden=True)):
        with pytest.raises(ValueError):
            make()
    t = Teacher("playout", n_playouts=2, hidden=True, roles=0b010)
    assert t.kind == "playout" and t.roles == 0b010 and Teacher("ismcts", budget=8, roles=0b101).roles == 0b101
    assert Teacher("solve").roles == 7 and Teacher("guided", budget=4, evaluator=engine.PlayoutLeaf(1)).evaluator is not None
    for kw in (dict(targets="teacher"), dict(targets="teacher", teacher="playout"), dict(targets="mc", teacher=t),
               dict(targets="td", act="teacher"), dict(targets="teacher", teacher=t, label_every=0),
               dict(targets="teacher", teacher=t, min_den=0), dict(targets="teacher", teacher=t, act="both")):
        with pytest.raises(ValueError):
            glue.TrainLoop(None, {}, 3, **kw)
        with pytest.raises(ValueError):
            glue.train(3, {"lord": None}, 1, **kw)
    for bad in (dict(scale=0), dict(scale=1025), dict(min_den=0), dict(den_const=0), dict()):
        with pytest.raises(ValueError):
            glue.TeacherAssembler().label(torch.zeros((1, 176), dtype=torch.uint8), torch.ones(1), torch.zeros((1, 2)),
                                          torch.zeros((1, 2)), **bad)
    # the recorder's own checks, with the device question answered for it (its buffers are plain tensors)
    with pytest.raises(importlib.import_module("doudizhu-rl_amd").DdzError):
        glue.TeacherRecorder(types.SimpleNamespace(T=4, device="cpu"), 64)
    monkeypatch.setattr(engine, "_require_gpu", lambda device: torch.device(device))
    monkeypatch.setattr(engine, "action_table", lambda dev, jk=False: torch.zeros((tc.N_ACTIONS, 16), dtype=torch.int8))
    env = types.SimpleNamespace(T=4, device="cpu", native_joker_kickers=False)
    for bad in (dict(capacity=0), dict(capacity=64, min_den=0), dict(capacity=64, trained_roles=(True, True))):
        with pytest.raises(ValueError):
            glue.TeacherRecorder(env, **bad)
    rec = glue.TeacherRecorder(env, 64, trained_roles=(False, True, True))
    assert rec.ws.numel() == engine.teach_ws_bytes(4) and rec.rings[0] is None
    assert rec.rings[1].numel() == engine.mc_ring_bytes(64)
    with pytest.raises(TypeError):
        rec.before(None, None)
    with pytest.raises(TypeError):
        rec.after(None, None)
    with pytest.raises(ValueError):
        rec.count("up")
    batch = rec.packed("lord", torch.tensor([0, 5]), 3)
    assert isinstance(batch, glue.ReturnBatch) and batch.n == 2


def test_engine_refuses_bad_buffers_before_the_library(monkeypatch):
    """env.teach goes through the one place that checks a caller's buffers (tests/test_engine_arguments_cpu.py: the stand-in
    library records launches and answers every size query with 64)"""
    import test_engine_arguments_cpu as ea
    E = importlib.import_module("doudizhu-rl_amd.engine")
    lib = ea.StandIn()
    monkeypatch.setattr(E._lib, "lib", lambda jk=False: lib)
    monkeypatch.setattr(E, "_stream", lambda device: None)
    env = ea.make_env(E)
    T, st = ea.T, env.slab_stride
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)               # noqa: E731
    ws, ring, num = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), i32(T * st)
    rings = [None, ring, ring]
    env.teach(ws, rings, 8, num, den_const=4)
    env.teach(ws, rings, 8, num, den=i32(T * st), unknown=i32(T * st), scale=1024, min_den=2, active=torch.ones(T, dtype=torch.bool),
              trained_roles=0b110, reward=(1.0, 2.0, 3.0))
    env.teach(ws, rings, 8, i32(T * 3), den_const=1, counts=i32(T), ids=i32(T * 3), stride=3)
    assert lib.calls == ["ddz_teach"] * 3
    bad = [lambda: env.teach(ws, rings, 8, num), lambda: env.teach(ws, rings, 8, num, den_const=0),
           lambda: env.teach(ws[:63], rings, 8, num, den_const=4), lambda: env.teach(ws, rings[:2], 8, num, den_const=4),
           lambda: env.teach(ws, [None, ring[:63], ring], 8, num, den_const=4),
           lambda: env.teach(ws, rings, 8, num.long(), den_const=4), lambda: env.teach(ws, rings, 8, num[:-1], den_const=4),
           lambda: env.teach(ws, rings, 8, num, den=i32(T * st - 1)), lambda: env.teach(ws, rings, 8, num, den=i32(T * st).float()),
           lambda: env.teach(ws, rings, 8, num, den_const=4, unknown=i32(T * st + 1)),
           lambda: env.teach(ws, rings, 8, num, den_const=4, scale=0), lambda: env.teach(ws, rings, 8, num, den_const=4, scale=1025),
           lambda: env.teach(ws, rings, 8, num, den_const=4, min_den=0),
           lambda: env.teach(ws, rings, 8, num, den_const=4, active=torch.ones(T - 1, dtype=torch.uint8)),
           lambda: env.teach(ws, rings, 8, num, den_const=4, trained_roles=8),
           lambda: env.teach(ws, rings, 8, num, den_const=4, reward=(1.0, 2.0)),
           lambda: env.teach(ws, rings, 8, num, den_const=4, counts=i32(T)),
           lambda: env.teach(ws, rings, 8, num, den_const=4, stride=3),
           lambda: env.teach(ws, rings, 8, i32(T * 3), den_const=4, counts=i32(T), ids=i32(T * 3 - 1), stride=3),
           lambda: env.teach(ws, rings, 8, num, den_const=4, counts=i32(T), ids=i32(T * st), stride=0),
           lambda: env.teach(ws.to("meta"), rings, 8, num, den_const=4)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            raise AssertionError(f"bad call {i} was accepted")
    assert lib.calls == ["ddz_teach"] * 3
