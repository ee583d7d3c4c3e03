"""GPU (-m gpu): the transition recorder's kernels (csrc/ddz_replay.h: k_tr_mark, k_tr_scan, k_tr_emit behind ddz_tr_before /
ddz_tr_after) alone, on the constructed workspaces of tests/recorder_cases.py, against its RecorderModel (held to
dqn_glue.TransitionAssembler + Replay in tests/test_recorder_cases_cpu.py).  Per case: the rows are imported into a BatchedEnv,
the workspace carries the case's slots and flags, every ring is 0xA5 in every byte but its count, and after EVERY call
  * the whole slots region and the whole meta region of the workspace (mark, blk and hdr are per-call scratch),
  * every byte of every ring: the count, the entries the model wrote, and 0xA5 everywhere else -- entries that should have been
    dropped, entries of a ring nothing emits into, the padding between the fields --
are the model's, bit for bit; status() == 0 at the end.  No index, id or pointer handed to the device is outside its buffer:
the role bytes above 2 rely on the kernels' own guard, and the sentinel is what reports a stray store.

TransitionRecorder.draw: its device-side clamp of the count, on counts written into the ring directly."""
import importlib

import numpy as np
import pytest
import torch

import recorder_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _ring_difference(got, ring):
    """where a ring differs from the model's image, in words"""
    off, nbytes = rc.ring_layout(ring.cap)
    bad = np.flatnonzero(got != ring.image())
    names = list(rc.RING_FIELDS)
    field = names[int(np.searchsorted([off[f] for f in names], bad[0], side="right")) - 1]
    width = {"count": 8, "s0": rc.ROW_BYTES, "s1": rc.ROW_BYTES, "done": 1}.get(field, 4)
    e = int(bad[0] - off[field]) // width
    where = "padding" if e >= ring.cap else f"entry {e} ({'written' if ring.written[e] else 'not written'} by the model)"
    return f"{len(bad)} bytes differ, the first at byte {int(bad[0])}: field {field}, {where}, got {int(got[bad[0]])}"


def _compare(m, ws, rings, step):
    off, _ = rc.ws_layout(m.T)
    got = ws.cpu().numpy()
    slots = got[: m.slots.size].reshape(m.slots.shape)
    if not np.array_equal(slots, m.slots):
        t, k = np.argwhere((slots != m.slots).any(2))[0]
        raise AssertionError(f"{step}: slot of table {t}, role {k} differs")
    meta = got[off["meta"]: off["meta"] + m.T * 16].view(np.uint32).reshape(m.T, 4)
    if not np.array_equal(meta, m.meta):
        t = int(np.flatnonzero((meta != m.meta).any(1))[0])
        raise AssertionError(f"{step}: meta of table {t}: got {meta[t].tolist()}, model {m.meta[t].tolist()}")
    for k in range(3):
        if rings[k] is None:
            continue
        g = rings[k].cpu().numpy()
        count = int(g[:8].view(np.int64)[0])
        assert count == m.rings[k].count, f"{step}: count of ring {k}: got {count}, model {m.rings[k].count}"
        if not np.array_equal(g, m.rings[k].image()):
            raise AssertionError(f"{step}: ring {k}: {_ring_difference(g, m.rings[k])}")


@pytest.mark.parametrize("name", list(rc.CASES))
def test_device_equals_model(pkg, name):
    case = rc.CASES[name]()
    T, cap = case.T, case.capacity
    m = rc.model_of(case)
    env = pkg.BatchedEnv(T, seed=1, device="cuda:0")
    ws = _dev(m.ws_image())
    assert ws.numel() == pkg.tr_ws_bytes(T)
    rings = [None if r is None else _dev(r.image()) for r in m.rings]
    assert all(r is None or r.numel() == pkg.tr_ring_bytes(cap) for r in rings)
    for i, call in enumerate(case.calls):
        env.state_import(torch.from_numpy(call.states.reshape(-1)))
        m.apply(call)
        if call.kind == "before":
            env.tr_before(ws, rings, cap, _dev(call.chosen), _dev(call.greedy), None if call.active is None else _dev(call.active),
                          call.trained)
        else:
            env.tr_after(ws, rings, cap, _dev(call.done), _dev(call.r), call.reward, call.quirk)
        _compare(m, ws, rings, f"{name}, call {i} ({call.kind})")
    assert env.status() == 0
    env.close()


# ---- TransitionRecorder.draw ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorder(pkg, glue):
    env = pkg.BatchedEnv(64, seed=3, device="cuda:0")
    env.reset()
    return glue.TransitionRecorder(env, 64, trained_roles=(False, True, True))


@pytest.mark.parametrize("count", [1, 3, 63, 64, 65, 2 ** 40])
def test_draw_stays_inside_the_live_entries(recorder, count):
    recorder.fields[1]["count"].fill_(count)
    assert int(recorder.count("lord")) == count and int(recorder.count("down")) == 0
    idx = recorder.draw("lord", 4096, at_least=1)
    assert idx.dtype == torch.int64 and idx.shape == (4096,) and idx.device.type == "cuda"
    live = min(count, 64)
    assert int(idx.min()) >= 0 and int(idx.max()) <= live - 1
    if count == 3:
        assert set(idx.unique().tolist()) == {0, 1, 2}
    if count == 1:
        assert not bool(idx.any())


def test_draw_needs_a_known_count(recorder):
    recorder.fields[1]["count"].fill_(5)
    with pytest.raises(ValueError):
        recorder.draw("lord", 4096, at_least=0)
    with pytest.raises(ValueError):
        recorder.draw("lord", 4096)                       # known[] is still 0: note_counts() was never called
    with pytest.raises(ValueError):
        recorder.draw("up", 4096, at_least=1)             # no ring
