"""CPU: what the host layer of the recorders and evaluators says to the library, without a device.

The stand-in library of tests/test_engine_arguments_cpu.py records every launch with its arguments.  Two statements:

  choose-rule equivalence   Teacher.evaluate + Teacher.choose issue the launches of the matching BatchedEnv.*_choose -- same entry
                            points, same order, same scalar arguments -- for every Teacher kind, so the moves a teacher loop trains on
                            are the moves the same evaluator serves; and a second evaluate() hands the library the buffers of the
                            first (no allocation per call).  "guided" owns no cached statistics: a GuidedSearch makes its own root
                            sums, so there the trace is compared and the buffers are only required to be the search's.
  call trace                one call each of tr_before, tr_after, mc_before, mc_after, teach, every evaluator verb and every
                            *_choose gives the (entry point, scalar arguments) sequence of tests/golden/host_trace.json, recorded
                            once before the host layer was restated (python tests/test_host_trace_cpu.py writes it anew).

T = 4, stride 512, as in that file; every comparison is exact."""
import importlib
import json
import os

import pytest
import torch

from test_engine_arguments_cpu import (CAP, E, STRIDE, T, StandIn, addresses, cfr_out, i8, i32, i64, make_env, rings, scalars, u8,  # noqa: F401
                                       z)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_trace.json")


def nothing(search):
    """a leaf evaluator that leaves .values as they are"""


# kind: (Teacher keywords, the *_choose call with the same keywords)
KINDS = {
    "playout": (dict(n_playouts=4, salt=3, chunks=2), lambda e, kw: e.playout_choose(**kw)),
    "playout_hidden": (dict(n_playouts=4, hidden=True, roles=0b010), lambda e, kw: e.playout_choose(**kw)),
    "search": (dict(budget=8, trees=2, mode="sides", c=0.5, salt=1), lambda e, kw: e.search_choose(**kw)),
    "ismcts": (dict(budget=8, trees=2, salt=2, roles=0b101), lambda e, kw: e.ismcts_choose(**kw)),
    "solve": (dict(budget=64, max_cards=8, worlds=3, hidden=True, roles=0b110, salt=5, chunks=2, tt_entries=256),
              lambda e, kw: e.solve_choose(**kw)[0]),
    "guided": (dict(budget=2, trees=2, salt=4, hidden=True), lambda e, kw: e.guided_choose(nothing, **kw)),
}
# the launch that writes the statistics, and where its statistic buffers stand among its addresses (the handle and the stream are no
# c_void_p of the stand-in env; totals is null)
STATS_OF = {"playout": ("ddz_playout", (0,)), "playout_hidden": ("ddz_playout_hidden", (0,)), "search": ("ddz_search", (0, 1)),
            "ismcts": ("ddz_ismcts", (0, 1)), "solve": ("ddz_solve", (0, 1, 2))}


def teacher_of(E, kind):
    kw = KINDS[kind][0]
    name = kind.split("_")[0]
    return E.Teacher(name, evaluator=nothing if name == "guided" else None, **kw)


def told(E):
    """the launches so far as [entry point, scalar arguments], and the record emptied"""
    lib = E._lib.lib()
    out = [[name, scalars(args)] for name, args in lib.trace]
    del lib.trace[:], lib.calls[:]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_issues_the_calls_of_the_choose_verb(E, kind):
    kw, choose = KINDS[kind]
    env = make_env(E)
    choose(env, kw)
    served = told(E)
    assert served, "the choose verb reached the library"
    env, teacher = make_env(E), teacher_of(E, kind)
    stats = teacher.evaluate(env)
    out = teacher.choose(env, stats)
    assert out.dtype == i32 and out.numel() == T
    assert told(E) == served


@pytest.mark.parametrize("kind", KINDS)
def test_second_evaluate_reuses_the_statistic_buffers(E, kind):
    env, teacher, lib = make_env(E), teacher_of(E, kind), E._lib.lib()
    first = teacher.evaluate(env)
    one = list(lib.trace)
    del lib.trace[:]
    second = teacher.evaluate(env)
    two = list(lib.trace)
    assert [n for n, _ in one] == [n for n, _ in two]
    if kind == "guided":
        # the root sums are the search's own: what evaluate hands out is what ddz_guided_close wrote
        close = addresses(two[-1][1])
        assert two[-1][0] == "ddz_guided_close" and second.den.data_ptr() in close and second.num.data_ptr() in close
        return
    name, where = STATS_OF[kind]
    a, b = (addresses(next(args for n, args in t if n == name)) for t in (one, two))
    assert [a[k] for k in where] == [b[k] for k in where] and all(a[k] for k in where)
    for x, y in zip(first, second):
        if torch.is_tensor(x):
            assert x.data_ptr() == y.data_ptr() and x.shape == y.shape


# ---- the call trace ----
def _stats():
    return {"num": z(CAP, dt=i32), "den": z(CAP, dt=i32), "unknown": z(CAP, dt=i32)}


# name: the call on a fresh stand-in env (E: the engine module)
VERBS = {
    "tr_before": lambda E, e: e.tr_before(z(64, dt=u8), rings(), 8, z(T, dt=i32), z(T, dt=i32), torch.ones(T, dtype=torch.bool), 0b110),
    "tr_before_all": lambda E, e: e.tr_before(z(64, dt=u8), [z(64, dt=u8)] * 3, 8, z(T, dt=i32), z(T, dt=i32)),
    "tr_after": lambda E, e: e.tr_after(z(64, dt=u8), rings(), 8, z(T, dt=u8), z(T, dt=i8), (50.0, 100.0, 50.0), True),
    "mc_before": lambda E, e: e.mc_before(z(64, dt=u8), 54, z(T, dt=i32), z(T, dt=u8), 0b011),
    "mc_after": lambda E, e: e.mc_after(z(64, dt=u8), 54, rings(), 8, z(T, dt=u8), z(T, dt=i8), (1.0, 2.0, 3.0), 0.5),
    "teach_den": lambda E, e: e.teach(z(64, dt=u8), rings(), 8, scale=1024, min_den=2, active=torch.ones(T, dtype=torch.bool),
                                      trained_roles=0b110, **_stats()),
    "teach_const": lambda E, e: e.teach(z(64, dt=u8), rings(), 8, z(2 * T, dt=i32), den_const=4, counts=z(T, dt=i32),
                                        ids=z(2 * T, dt=i32), stride=2, reward=(1.0, 2.0, 3.0)),
    "playout": lambda E, e: e.playout(4, salt=-1, totals=z(4, dt=i64)),
    "playout_default_chunks_hidden": lambda E, e: e.playout(64, hidden=True, roles=0b010),
    "playout_worlds": lambda E, e: e.playout_worlds(3, salt=7, roles=0b100),
    "search": lambda E, e: e.search(8, totals=z(4, dt=i64)),
    "search_hidden": lambda E, e: e.search(16, trees=3, mode="sides", c=1.25, salt=9, hidden=True, roles=0b001),
    "ismcts": lambda E, e: e.ismcts(8, trees=2, c=0.0, salt=2, roles=0b101),
    "guided": lambda E, e: e.guided(3, trees=2, salt=4).run(nothing, totals=z(4, dt=i64)),
    "cfr": lambda E, e: e.cfr(),
    "cfr_slots": lambda E, e: e.cfr(4, roles=0b010, slots=2, totals=z(4, dt=i64), out=cfr_out()),
    "solve": lambda E, e: e.solve(),
    "solve_hidden": lambda E, e: e.solve(64, 8, 3, True, 0b110, 5, 2, 256, totals=z(4, dt=i64)),
    "playout_choose": lambda E, e: e.playout_choose(4, salt=1, out=z(T, dt=i32)),
    "search_choose": lambda E, e: e.search_choose(8, trees=2),
    "search_choose_twice": lambda E, e: (e.search_choose(8, trees=2), e.ismcts_choose(8, trees=2)),
    "ismcts_choose": lambda E, e: e.ismcts_choose(8, roles=0b011),
    "guided_choose": lambda E, e: e.guided_choose(nothing, 2, trees=1, hidden=True, roles=0b010),
    "cfr_choose": lambda E, e: e.cfr_choose(salt=3),
    "cfr_choose_greedy_solved": lambda E, e: e.cfr_choose(greedy=True, solved=cfr_out()),
    "solve_choose": lambda E, e: e.solve_choose(),
    "solve_choose_solved": lambda E, e: e.solve_choose(worlds=3, solved=(z(T, dt=i32), z(T, STRIDE, dt=i32), z(T, STRIDE, dt=i32))),
    "teacher_playout": lambda E, e: (lambda t: t.choose(e, t.evaluate(e)))(teacher_of(E, "playout_hidden")),
    "teacher_search": lambda E, e: (lambda t: t.choose(e, t.evaluate(e)))(teacher_of(E, "search")),
    "teacher_ismcts": lambda E, e: (lambda t: t.choose(e, t.evaluate(e)))(teacher_of(E, "ismcts")),
    "teacher_solve": lambda E, e: (lambda t: t.choose(e, t.evaluate(e)))(teacher_of(E, "solve")),
    "teacher_guided": lambda E, e: (lambda t: t.choose(e, t.evaluate(e)))(teacher_of(E, "guided")),
}


def record(E):
    out = {}
    for name, call in VERBS.items():
        call(E, make_env(E))
        out[name] = told(E)
    return out


def test_call_trace_is_the_recorded_one(E):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record(E)))
    assert sorted(got) == sorted(want)
    for name in VERBS:
        assert got[name] == want[name], name


if __name__ == "__main__":
    # writes the fixture from the tree as it stands: the patches of the fixture E, by hand
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    M = importlib.import_module("doudizhu-rl_amd.engine")
    lib = StandIn()
    M._lib.lib = lambda jk=False: lib
    M._stream = lambda device: None
    M._require_gpu = lambda device: torch.device(device)
    with open(GOLDEN, "w") as f:
        json.dump(record(M), f, indent=0, sort_keys=True)
        f.write("\n")
