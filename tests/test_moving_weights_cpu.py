"""CPU: the Q caches under moving weights, where no GPU is present (dqn_glue.FactorisedQ / RoleQ on a CPU QNet; the moves of
tests/moving_weights_cases.py).  Three statements:

  detection matrix   _versions() reports every move but a write through `.data`; refresh() returns what it did, and
                     refresh(force=True) is the documented way out for `.data` writes.
  storage pin        the derived tables, and RoleQ's stacked tables, keep their addresses across every refresh(): a captured
                     graph holds those addresses, so a refresh that rebinds a table leaves the graph on freed memory.
  freshness          FactorisedQ.tables + q_csr (and ragged_q's object cached on the network) after every move equal a fresh
                     object's output bit for bit, lie within 1e-5 of the fp64 literal forward on the current weights (64
                     constructed rows, |q| < 1), and differ from the output before the move; the reference itself must move by
                     more than 1e-3 in the median (moving_weights_cases.assert_moved)."""
import importlib

import pytest
import torch

import moving_weights_cases as M


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _net(glue, P, seed):
    torch.manual_seed(seed)
    return glue.QNet(P).eval()


def _addresses(obj, names):
    out = {k: getattr(obj, k).data_ptr() for k in names}
    if hasattr(obj, "W2_jok"):
        out.update({"Wd": obj.Wd.data_ptr(), "W2_jok0": obj.W2_jok[0].data_ptr(), "W2_jok1": obj.W2_jok[1].data_ptr()})
    return out


def _tables(obj, names):
    return {k: getattr(obj, k).clone() for k in names}


@pytest.mark.parametrize("name", M.MOVES)
def test_versions_report_every_move_but_a_data_write(glue, name):
    seen = M.MOVES[name][1]
    net = _net(glue, 6, 3)
    fq = glue.FactorisedQ(net)
    rq = glue.RoleQ({"lord": net, "down": _net(glue, 6, 4), "up": None}, 3)
    v0, r0 = fq._versions(), rq._versions()
    assert fq.refresh() is False and rq.refresh() is False            # nothing moved: nothing recomputed
    M.apply(name, glue, net, seed=1)
    assert (fq._versions() != v0) == seen and (rq._versions() != r0) == seen
    assert fq.refresh() is seen and rq.refresh() is seen
    assert fq.refresh() is False and rq.refresh() is False
    assert fq.refresh(force=True) is True and rq.refresh(force=True) is True


@pytest.mark.parametrize("name", M.MOVES)
def test_refresh_keeps_the_storage_of_every_derived_table(glue, name):
    net, second = _net(glue, 9, 5), _net(glue, 9, 6)
    fq = glue.FactorisedQ(net)
    rq = glue.RoleQ({"lord": net, "down": second, "up": net}, 2)
    fq.tables(M.constructed_rows(9, 1)[0])                             # a workspace exists
    a0, s0, ws0 = _addresses(fq, fq.TABLES), _addresses(rq, rq.STACKED), dict(fq._ws)
    assert len(ws0) == 1
    M.apply(name, glue, net, seed=2)
    fq.refresh(force=True), rq.refresh(force=True)
    assert _addresses(fq, fq.TABLES) == a0 and _addresses(rq, rq.STACKED) == s0
    assert fq._ws.keys() == ws0.keys() and all(fq._ws[k] is ws0[k] for k in ws0)     # refresh() keeps the workspaces
    # and the storage holds the new weights: a fresh object's tables, bit for bit
    fresh = glue.FactorisedQ(net)
    for k in fq.TABLES:
        assert torch.equal(getattr(fq, k), getattr(fresh, k)), k
    assert torch.equal(fq.Wd, fresh.Wd) and all(torch.equal(a, b) for a, b in zip(fq.W2_jok, fresh.W2_jok))
    assert fq.Wd.data_ptr() == fq.W2.data_ptr()


@pytest.mark.parametrize("P", [4, 6, 7, 9])
@pytest.mark.parametrize("name", M.MOVES)
def test_q_after_a_move_is_a_fresh_objects_q(glue, name, P):
    seen = M.MOVES[name][1]
    face, rows, offsets, table = M.constructed_rows(P, seed=10 + P)
    net = _net(glue, P, 7 + P)
    q = lambda fq: fq.q_csr(fq.tables(face), rows, offsets).clone()   # noqa: E731
    fq = glue.FactorisedQ(net)
    before, ragged_before = q(fq), glue.ragged_q(net, face, rows, offsets).clone()
    ref_before = M.reference_q(net, face[table], rows)
    assert float((before.double() - ref_before).abs().max()) < M.Q_BOUND
    M.apply(name, glue, net, seed=3)
    ref = M.reference_q(net, face[table], rows)
    M.assert_moved(ref_before, ref)
    after, ragged_after = q(fq), glue.ragged_q(net, face, rows, offsets).clone()
    if not seen:
        # the documented behaviour of a write through .data: stale, bit for bit, until refresh(force=True)
        assert torch.equal(after, before) and torch.equal(ragged_after, ragged_before)
        assert fq.refresh(force=True) is True and net._ddz_factorised.refresh(force=True) is True
        after, ragged_after = q(fq), glue.ragged_q(net, face, rows, offsets).clone()
    fresh = q(glue.FactorisedQ(net))
    assert torch.equal(after, fresh) and torch.equal(ragged_after, fresh)
    assert float((after.double() - ref).abs().max()) < M.Q_BOUND
    assert int(((after - before).abs() > 1e-4).sum()) * 2 >= after.numel()           # not a no-op


@pytest.mark.parametrize("name", M.SEEN)
def test_role_q_rewrites_the_moved_slot_and_no_other(glue, name):
    A, B, C = (_net(glue, 6, s) for s in (21, 22, 23))
    maps = (({"lord": A, "down": B, "up": C}, B, 2), ({"lord": A, "down": A, "up": B}, A, 1), ({"lord": A, "down": A, "up": B}, B, 0),
            ({"lord": None, "down": B, "up": C}, C, 0))                # (role map, the network that moves, its slot: up first)
    for i, (nets, moved, slot) in enumerate(maps):
        rq = glue.RoleQ(nets, 3)
        assert rq.nets[slot] is moved
        old = _tables(rq, rq.STACKED)
        M.apply(name, glue, moved, seed=4 + i)
        assert rq.refresh() is True
        fresh = glue.FactorisedQ(moved)
        for k in rq.STACKED:
            now = getattr(rq, k)
            for s in range(rq.N):
                if s == slot:
                    assert torch.equal(now[s], getattr(fresh, k).view(now[s].shape)), (k, s)
                else:
                    assert torch.equal(now[s], old[k][s]), (k, s)
        assert any(not torch.equal(getattr(rq, k)[slot], old[k][slot]) for k in rq.STACKED)
        # a RoleQ built now stacks the same tables
        built = glue.RoleQ(nets, 3)
        assert all(torch.equal(getattr(rq, k), getattr(built, k)) for k in rq.STACKED)


def test_every_parameter_reaches_a_derived_table(glue):
    """one parameter at a time (all ten): the version tuple sees it and at least one derived table changes -- no parameter is
    missing from _versions() or from refresh()"""
    net = _net(glue, 7, 31)
    fq = glue.FactorisedQ(net)
    for pname, p in net.named_parameters():
        old = _tables(fq, fq.TABLES)
        with torch.no_grad():
            p.add_(0.05)
        assert fq.refresh() is True, pname
        changed = [k for k in fq.TABLES if not torch.equal(getattr(fq, k), old[k])]
        assert changed, pname
        fresh = glue.FactorisedQ(net)
        assert all(torch.equal(getattr(fq, k), getattr(fresh, k)) for k in fq.TABLES), pname


@pytest.mark.parametrize("name", ["adam", "perturb", "load"])
def test_no_derived_table_is_a_view_of_a_parameter(glue, name):
    """A derived table that is a VIEW of a parameter (w2 once was fc2.weight[0]) follows in-place writes on its own -- a cache
    that is half stale after a .data write, and a captured graph that plays new fc2 weights on old tables -- and, cached on the
    network by ragged_q, makes copy.deepcopy(net) raise once the parameter has been written in place: train() makes its target
    networks that way."""
    import copy
    net = _net(glue, 6, 41)
    face, rows, offsets, _ = M.constructed_rows(6, seed=2)
    glue.ragged_q(net, face, rows, offsets)
    fq = net._ddz_factorised
    owned = {p.untyped_storage().data_ptr() for p in net.parameters()}
    tables = [getattr(fq, k) for k in fq.TABLES] + list(fq.W2_jok)
    assert not any(t.untyped_storage().data_ptr() in owned for t in tables)
    M.apply(name, glue, net, seed=5)
    twin = copy.deepcopy(net)
    assert torch.equal(glue.ragged_q(twin, face, rows, offsets), glue.ragged_q(net, face, rows, offsets))
