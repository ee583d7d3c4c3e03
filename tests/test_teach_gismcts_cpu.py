"""CPU: Teacher("guided_ismcts") -- the keywords it accepts and refuses, its roles mask (always the hidden form) -- and, on the
stand-in library of tests/test_engine_arguments_cpu.py, what the host layer of guided_ismcts says to the library: the
ddz_gismcts_* entry points with ddz_guided_*'s arguments minus `hidden`, the launches of guided_ismcts_choose issued by
Teacher.evaluate + Teacher.choose, and the one-open-search guard shared with guided()."""
import importlib

import pytest
import torch

from test_engine_arguments_cpu import E, STRIDE, T, addresses, i32, i64, make_env, scalars, z  # noqa: F401


def nothing(search):
    """a leaf evaluator that leaves .values as they are"""


def told(E):
    lib = E._lib.lib()
    out = [[name, scalars(args)] for name, args in lib.trace]
    del lib.trace[:], lib.calls[:]
    return out


def test_teacher_accepts_and_refuses_the_right_keywords():
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    Teacher = engine.Teacher
    leaf = engine.PlayoutLeaf(1)
    for make in (lambda: Teacher("guided_ismcts", budget=8),                              # no evaluator
                 lambda: Teacher("guided_ismcts", evaluator=leaf),                        # no budget
                 lambda: Teacher("guided_ismcts", evaluator=leaf, budget=8, hidden=True),  # always hidden: no such keyword
                 lambda: Teacher("guided_ismcts", evaluator=leaf, budget=8, depth=3),
                 lambda: Teacher("guided_ismcts", evaluator=leaf, budget=8, out=None),
                 lambda: Teacher("guided_ismcts", evaluator=leaf, budget=8, roles=9),
                 lambda: Teacher("ismcts", budget=8, evaluator=leaf),                     # an evaluator is the guided kinds' alone
                 lambda: Teacher("guided", budget=8)):
        with pytest.raises(ValueError):
            make()
    t = Teacher("guided_ismcts", evaluator=leaf, budget=8, trees=2, mode="sides", c=0.5, salt=3, roles=0b101)
    assert t.kind == "guided_ismcts" and t.evaluator is leaf and t.roles == 0b101
    assert t.kwargs == dict(budget=8, trees=2, mode="sides", c=0.5, salt=3, roles=0b101)
    assert Teacher("guided_ismcts", evaluator=leaf, budget=4).roles == 7
    # a roles mask below 7 is the hidden form's: guided needs hidden=True for it, guided_ismcts takes it as it is
    with pytest.raises(ValueError):
        Teacher("guided", evaluator=leaf, budget=4, roles=0b010)
    assert Teacher("guided", evaluator=leaf, budget=4, roles=0b010, hidden=True).roles == 0b010
    assert Teacher._STATS["guided_ismcts"](type("Env", (), {"counts": 1})(), {}, 2, 3) == (1, 3, 2, None, None, engine.BatchedEnv.GUIDED_ONE)


def test_host_layer_calls_the_gismcts_entry_points(E):
    env = make_env(E)
    totals = z(4, dt=i64)
    search = env.guided_ismcts(3, trees=2, mode="sides", c=0.5, salt=4, roles=0b110)
    assert isinstance(search, E.GuidedSearch) and search.ismcts and search.hidden and search.n_items == T * 2
    assert search.leaves.shape == (T * 2, 11, 16) and search.need.shape == (T * 2,) and search.values.shape == (T * 2,)
    assert search.env is env
    visits, wins = search.run(nothing, totals=totals)
    assert visits.shape == (T, STRIDE) and wins.shape == (T, STRIDE)
    got = told(E)
    common = [None, 3, 2, 1, 0.5, 4, 0b110]
    assert [n for n, _ in got] == ["ddz_gismcts_open"] + ["ddz_gismcts_step"] * 3 + ["ddz_gismcts_close"]
    assert got[0][1] == common + [STRIDE, "ptr", 64, None]
    assert got[1][1] == common + [STRIDE, None, "ptr", "ptr", "ptr", 64, None]           # the first step: no values yet
    assert got[2][1] == got[3][1] == common + [STRIDE, "ptr", "ptr", "ptr", "ptr", 64, None]
    assert got[4][1] == common + ["ptr", STRIDE, "ptr", "ptr", "ptr", "ptr", 64, None]
    # the same calls with `hidden` in its place are guided(hidden=True)'s
    env.guided(3, trees=2, mode="sides", c=0.5, salt=4, hidden=True, roles=0b110).run(nothing, totals=totals)
    for (name, args), (gname, gargs) in zip(got, told(E)):
        assert gname == name.replace("gismcts", "guided") and gargs[:6] + gargs[7:] == args and gargs[6] == 1


def test_teacher_issues_the_calls_of_guided_ismcts_choose(E):
    kw = dict(budget=2, trees=2, salt=4, roles=0b011)
    env = make_env(E)
    out = env.guided_ismcts_choose(nothing, **kw)
    assert out.dtype == i32 and out.numel() == T
    served = told(E)
    assert [n for n, _ in served][:4] == ["ddz_gismcts_open", "ddz_gismcts_step", "ddz_gismcts_step", "ddz_gismcts_close"]
    assert served[-1][0] == "ddz_search_choose"
    env, teacher = make_env(E), E.Teacher("guided_ismcts", evaluator=nothing, **kw)
    stats = teacher.evaluate(env)
    assert stats.scale == E.BatchedEnv.GUIDED_ONE and stats.roles == 0b011 and stats.den_const is None and stats.unknown is None
    lib = E._lib.lib()
    close = addresses(lib.trace[-1][1])
    assert lib.trace[-1][0] == "ddz_gismcts_close" and stats.den.data_ptr() in close and stats.num.data_ptr() in close
    out = teacher.choose(env, stats)
    assert out.dtype == i32 and out.numel() == T
    assert told(E) == served


def test_one_open_search_per_environment_and_misuse(E):
    env = make_env(E)
    s = env.guided_ismcts(4, trees=2)
    with pytest.raises(RuntimeError):
        env.guided_ismcts(4, trees=2)
    with pytest.raises(RuntimeError):
        env.guided(4, trees=2)                       # the guard is the environment's: shared with guided()
    s.step()
    s.close()
    for call in (s.step, s.close):
        with pytest.raises(RuntimeError):
            call()
    g = env.guided(4, trees=2)
    with pytest.raises(RuntimeError):
        env.guided_ismcts(4, trees=2)
    g.close()
    told(E)
    with pytest.raises(ValueError):
        env.guided_ismcts(4096, trees=512)           # budget * trees * 1024 >= 2^31
    for bad in (dict(mode="both"), dict(c=-1.0), dict(trees=0), dict(roles=8)):
        with pytest.raises(ValueError):
            env.guided_ismcts(4, **bad)
    with pytest.raises(ValueError):
        env.guided_ismcts(0)
    assert told(E) == [] and env._guided_pending is None
    n = T * 2
    s = env.guided_ismcts(4, trees=2)
    told(E)
    for name, bad in (("values", torch.zeros(n, dtype=torch.int64)), ("values", torch.zeros(n - 1, dtype=torch.int32)),
                      ("need", torch.zeros(n + 1, dtype=torch.int32)), ("leaves", torch.zeros((n, 11, 16), dtype=torch.int8)),
                      ("leaves", torch.zeros((n - 1, 11, 16), dtype=torch.uint8))):
        keep = getattr(s, name)
        setattr(s, name, bad)
        with pytest.raises(ValueError):
            s.step()
        if name == "values":
            with pytest.raises(ValueError):
                s.close()
        setattr(s, name, keep)
    assert told(E) == [] and s.steps == 0 and not s.closed
    s.close()
