"""CPU: the host side of the transition recorder's entry points (include/ddz_env.h: ddz_tr_*, ddz_observe_states) -- sizes,
layout and argument errors, all answered before anything touches a device -- and the Python classes' behaviour without a GPU."""
import ctypes as C
import importlib
import types

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    importlib.import_module("doudizhu-rl_amd.build").build()
    return importlib.import_module("doudizhu-rl_amd._lib").lib()


def test_new_symbols_are_bound(L):
    lib = importlib.import_module("doudizhu-rl_amd._lib")
    for name in ("ddz_tr_ws_bytes", "ddz_tr_ring_bytes", "ddz_tr_ring_layout", "ddz_tr_before", "ddz_tr_after",
                 "ddz_observe_states"):
        assert name in lib.SYMBOLS and getattr(L, name)
    assert L.ddz_abi_version() == 1                       # the additions are additive


def test_workspace_size_is_monotone_and_aligned(L):
    prev = 0
    for T in (1, 2, 37, 255, 256, 257, 700, 4096, 65536, 1 << 20):
        n = L.ddz_tr_ws_bytes(T)
        assert n % 256 == 0 and n > prev
        assert n >= T * (3 * 176 + 16 + 4)                # three state rows, the ids + flags word, the per-call mark
        assert n <= T * 548 + 256 * 5 + ((T + 255) // 256) * 16 + 256
        prev = n
    assert L.ddz_tr_ws_bytes(0) < 0 and L.ddz_tr_ws_bytes(-3) < 0 and L.ddz_tr_ws_bytes((1 << 30) + 1) < 0


def test_ring_layout(L):
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    prev = 0
    for cap in (1, 64, 1000, 20000):
        n = L.ddz_tr_ring_bytes(cap)
        off = (C.c_int64 * 8)()
        assert L.ddz_tr_ring_layout(cap, off) == 0
        off = list(off)
        sizes = [8, cap * 176, cap * 176, cap * 4, cap * 4, cap * 4, cap * 4, cap]
        assert off[0] == 0 and all(o % 256 == 0 for o in off) and n % 256 == 0 and n > prev
        for k in range(8):                                # the fields follow each other without overlap, inside the ring
            assert off[k] + sizes[k] <= (off[k + 1] if k < 7 else n)
        assert engine.tr_ring_bytes(cap) == n and engine.tr_ring_layout(cap) == dict(zip(engine.TR_RING_FIELDS, off))
        prev = n
    assert L.ddz_tr_ring_bytes(0) < 0 and L.ddz_tr_ring_bytes((1 << 30) + 1) < 0
    assert L.ddz_tr_ring_layout(64, None) == -1 and L.ddz_tr_ring_layout(0, (C.c_int64 * 8)()) == -1   # EINVAL
    with pytest.raises(ValueError):
        engine.tr_ring_bytes(0)
    with pytest.raises(ValueError):
        engine.tr_ws_bytes(0)


def test_argument_errors(L):
    buf = (C.c_int64 * 64)()
    rings = (C.c_void_p * 3)()
    reward = (C.c_float * 3)(50, 100, 50)
    # a null handle is DDZ_EHANDLE, as the neighbouring entry points answer
    assert L.ddz_tr_before(None, buf, 512, rings, 0, 64, buf, buf, None, 7, None) == -2
    assert L.ddz_tr_after(None, buf, 512, rings, 0, 64, buf, buf, reward, 0, None) == -2
    # the handle-free decoder: null / misaligned buffers, a bad variant, a negative n are DDZ_EINVAL; n = 0 is a no-op
    assert L.ddz_observe_states(0, None, None, 4, 2, buf, None) == -1
    assert L.ddz_observe_states(0, buf, None, 4, 2, None, None) == -1
    assert L.ddz_observe_states(0, buf, None, 4, 4, buf, None) == -1
    assert L.ddz_observe_states(0, buf, None, -1, 2, buf, None) == -1
    assert L.ddz_observe_states(0, C.c_void_p(C.addressof(buf) + 4), None, 1, 2, buf, None) == -1
    assert L.ddz_observe_states(0, None, None, 0, 2, None, None) == 0


def test_recorder_needs_a_gpu():
    """no CPU fall-back, as BatchedEnv: without a device (or on another device than a GPU) the classes raise DdzError"""
    pkg = importlib.import_module("doudizhu-rl_amd")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    with pytest.raises(pkg.DdzError):
        pkg.BatchedEnv(4, device="cpu")
    with pytest.raises(pkg.DdzError):
        glue.TransitionRecorder(types.SimpleNamespace(T=4, device="cpu"), 64)
    with pytest.raises(pkg.DdzError):
        pkg.observe_states(torch.zeros((2, 176), dtype=torch.uint8), None, 2)
