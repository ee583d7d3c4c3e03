"""GPU (-m gpu): the return recorder (csrc/ddz_returns.h: k_mc_append behind ddz_mc_before; k_mc_mark, k_tr_scan, k_mc_emit behind
ddz_mc_after; dqn_glue.ReturnRecorder, mc_step, TrainLoop / train with targets="mc").
  1. the kernels alone on the constructed scripts of tests/return_cases.py against its ReturnModel (held to
     dqn_glue.ReturnAssembler and to the definition in tests/test_return_recorder_cpu.py): the rows are imported into a
     BatchedEnv, every ring is 0xA5 in every byte but its count, and after EVERY call the workspace's cnt, lost and hdr regions,
     the live log entries and every byte of every ring -- the count, the entries the model wrote, and 0xA5 everywhere else --
     are the model's, bit for bit;
  2. a live TrainLoop(targets="mc") run: what it handed the recorder, fed to ReturnAssembler, gives the same rings; decode()
     against observe_states of the recorded rows in every face variant;
  3. a captured iteration replayed leaves what eager iterations leave;
  4. train(targets="mc") end to end."""
import importlib
import math

import numpy as np
import pytest
import torch

import return_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _compare_rings(m, rings, step):
    for k in range(3):
        if rings[k] is None:
            continue
        g = rings[k].cpu().numpy()
        count = int(g[:8].view(np.int64)[0])
        assert count == m.rings[k].count, f"{step}: count of ring {k}: got {count}, model {m.rings[k].count}"
        want = m.rings[k].image()
        if not np.array_equal(g, want):
            off, _ = mc.ring_layout(m.cap)
            bad = np.flatnonzero(g != want)
            field = [f for f in mc.RING_FIELDS if off[f] <= bad[0]][-1]
            raise AssertionError(f"{step}: ring {k}: {len(bad)} bytes differ, the first at byte {int(bad[0])} "
                                 f"(field {field} + {int(bad[0]) - off[field]}): got {int(g[bad[0]])}, model {int(want[bad[0]])}")


def _compare(m, ws, rings, step):
    off, nbytes = mc.ws_layout(m.T, m.L)
    got = ws.cpu().numpy()
    T, L = m.T, m.L
    cnt = got[off["cnt"]: off["cnt"] + T * 4].reshape(T, 4)
    if not np.array_equal(cnt, m.cnt):
        t = int(np.flatnonzero((cnt != m.cnt).any(1))[0])
        raise AssertionError(f"{step}: n, c of table {t}: got {cnt[t].tolist()}, model {m.cnt[t].tolist()}")
    assert np.array_equal(got[off["lost"]: off["lost"] + T * 4].view(np.uint32), m.lost), f"{step}: lost"
    hdr = got[off["hdr"]: off["hdr"] + 64].view(np.int64)
    assert np.array_equal(hdr, m.hdr), f"{step}: hdr: got {hdr.tolist()}, model {m.hdr.tolist()}"
    live = np.arange(L)[None, :] < m.cnt[:, :1]
    rows = got[off["rows"]: off["rows"] + T * L * mc.ROW_BYTES].reshape(T, L, mc.ROW_BYTES)
    act = got[off["act"]: off["act"] + T * L * 4].view(np.int32).reshape(T, L)
    who = got[off["who"]: off["who"] + T * L * 2].reshape(T, L, 2)
    assert np.array_equal(rows[live], m.rows[live]) and np.array_equal(act[live], m.act[live]), f"{step}: log rows / actions"
    assert np.array_equal(who[live], m.who[live]), f"{step}: log role / ordinal"
    _compare_rings(m, rings, step)


# ---- 1. the kernels against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_device_equals_model(pkg, name):
    case = mc.CASES[name]()
    T, L, cap = case.T, case.log_cap, case.capacity
    m = mc.model_of(case)
    env = pkg.BatchedEnv(T, seed=1, device="cuda:0")
    ws = torch.zeros(pkg.mc_ws_bytes(T, L), dtype=torch.uint8, device="cuda:0")
    assert ws.numel() == mc.ws_layout(T, L)[1]
    rings = [None if r is None else _dev(r.image()) for r in m.rings]
    assert all(r is None or r.numel() == pkg.mc_ring_bytes(cap) for r in rings)
    for i, call in enumerate(case.calls):
        m.apply(call)
        if call.kind == "before":
            env.state_import(torch.from_numpy(call.states.reshape(-1)))
            env.mc_before(ws, L, _dev(call.chosen), None if call.active is None else _dev(call.active), call.trained)
        else:
            env.mc_after(ws, L, rings, cap, _dev(call.done), _dev(call.r), call.reward, call.gamma)
        _compare(m, ws, rings, f"{name}, call {i} ({call.kind})")
    assert env.status() == 0
    env.close()


# ---- 2. a live run -------------------------------------------------------------------------------------------------------------------
def _nets(glue, seed):
    torch.manual_seed(seed)
    return {"lord": glue.QNet(9).cuda().eval(), "down": glue.QNet(9).cuda().eval(), "up": None}


def test_live_run_equals_the_assembler(pkg, glue):
    T, cap, variant, gamma = 300, 1024, 2, 0.95
    env = pkg.BatchedEnv(T, seed=41, device="cuda:0")
    env.reset()
    env.legal_slab()
    nets = _nets(glue, 43)
    loop = glue.TrainLoop(env, nets, variant, capacity=cap, epsilon=0.5, targets="mc", gamma=gamma)
    rec = loop.rec
    assert isinstance(rec, glue.ReturnRecorder) and rec.trained == (False, True, True) and rec.log_cap == 108
    assert not hasattr(loop, "_greedy_ids")
    fed = []
    before, after = rec.before, rec.after
    rec.before = lambda ids, active=None: (fed.append(("before", env.state.clone(), ids.clone(), active.clone())),
                                           before(ids, active))[1]
    rec.after = lambda done, r: (fed.append(("after", done.clone(), r.clone())), after(done, r))[1]
    loop.run(120)
    assert len(fed) == 240 and int(env.stats()["episodes"]) >= T // 2

    asm = glue.ReturnAssembler(T, rec.log_cap, "cpu", None, rec.trained, gamma)
    m = mc.ReturnModel(T, rec.log_cap, cap, rec.trained, (0, 0, 0))          # (its rings and its store() only)
    for call in fed:
        if call[0] == "before":
            rows = call[1].cpu().view(T, 176)
            asm.before(rows[:, mc.ROLE_BYTE].long(), rows, call[2].cpu(), call[3].cpu())
        else:
            out = asm.after(call[1].cpu(), call[2].cpu())
            emits = ([], [], [])
            for i in range(out["ret"].numel()):
                emits[int(out["role"][i])].append((int(out["table"][i]), out["s0"][i].numpy(), int(out["a0"][i]),
                                                   out["ret"][i].numpy(), int(out["togo"][i])))
            m.store(emits)
    assert {e[0] for e in m.emitted} == {1, 2}
    for k in (1, 2):
        ring = m.rings[k]
        assert ring.count > cap                                              # (the rings wrapped)
        assert np.array_equal(rec.rings[k].cpu().numpy(), ring.image(fill=0)), f"ring {k}"
        assert len(set(ring.togo.tolist())) > 5 and (ring.ret > 0).any() and (ring.ret < 0).any()
    assert not rec.ws[pkg.mc_ws_layout(T, rec.log_cap)["lost"]:][:T * 4].any()          # no game overflows the default log
    index = torch.arange(cap, device="cuda:0")
    table = pkg.action_table("cuda:0")
    for k, role in ((1, "lord"), (2, "down")):
        ring = m.rings[k]
        for variant in range(4):
            d = rec.decode(role, index, variant)
            assert set(d) == {"s0", "a0", "ret", "togo"}
            assert torch.equal(d["s0"], pkg.observe_states(_dev(ring.s0), None, variant))
            assert torch.equal(d["a0"], pkg.rows_to_onehot(table[_dev(ring.a0).long()]))
            assert torch.equal(d["ret"], _dev(ring.ret)) and torch.equal(d["togo"], _dev(ring.togo))
    with pytest.raises(ValueError):
        rec.count("up")                                                      # the rule agent's role has no ring
    # a packed batch is side 0 of what decode gives, bit for bit, and has no side 1
    rec.note_counts()
    net = nets["lord"]
    batch = rec.sample_packed("lord", 64, 2)
    d = rec.decode("lord", batch.index, 2)
    with torch.no_grad():
        assert torch.equal(net.forward_packed(batch, 0), net.forward_stage(d["s0"], d["a0"]))
    with pytest.raises(ValueError):
        net.forward_packed(batch, 1)
    # clear(): the masked tables' logs are forgotten, the others' are not
    cnt = rec._cnt.clone()
    mask = torch.arange(T, device="cuda:0") % 2 == 0
    rec.clear(mask)
    assert not rec._cnt[mask].any() and torch.equal(rec._cnt[~mask], cnt[~mask]) and bool(cnt[mask].any())
    assert env.status() == 0


# ---- 3. no host in the loop ----------------------------------------------------------------------------------------------------------
def test_mc_train_loop_captured_equals_eager(pkg, glue):
    """capture fails on any host synchronisation inside the iteration, and the replayed graph must leave what eager calls do"""
    T, variant, cap = 300, 2, 512
    nets = _nets(glue, 17)

    def make():
        env = pkg.BatchedEnv(T, seed=23, device="cuda:0")
        env.reset()
        env.legal_slab()
        return env, glue.TrainLoop(env, nets, variant, capacity=cap, epsilon=0.0, targets="mc")

    env_a, eager = make()
    eager.run(150)
    env_b, cap_loop = make()
    cap_loop.run(3)
    graph = cap_loop.capture(1)
    for _ in range(147):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(env_a.state, env_b.state)
    for k in (1, 2):
        assert int(eager.rec.count(k)) > 0 and torch.equal(eager.rec.rings[k], cap_loop.rec.rings[k]), k
    assert torch.equal(eager.rec.ws, cap_loop.rec.ws)
    assert env_a.status() == 0 and env_b.status() == 0


# ---- 4. train() ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, "packed"])
def test_train_mc_smoke(pkg, glue, fused, monkeypatch):
    import copy
    torch.manual_seed(29)
    nets = {"lord": glue.QNet(9), "down": glue.QNet(9), "up": None}
    start = {r: [p.detach().clone() for p in nets[r].parameters()] for r in ("lord", "down")}
    seen = []
    step = glue.mc_step
    monkeypatch.setattr(glue, "mc_step", lambda policy, opt, batch, fused=False: (seen.append(type(batch)),
                                                                                  step(policy, opt, batch, fused=fused))[1])
    monkeypatch.setattr(glue, "td_step", None)                               # (not called)
    copies, deepcopy = [], copy.deepcopy
    monkeypatch.setattr(copy, "deepcopy", lambda x, *a: (copies.append(type(x)), deepcopy(x, *a))[1])
    out = glue.train(2, nets, episodes=30, tables=64, seed=31, fused=fused, batch_size=16, check_every=4, targets="mc")
    assert set(out) == {"lord", "down", "up", "episodes", "iterations", "loss", "checkpoints"}
    assert out["episodes"] >= 30 and out["lord"] + out["down"] + out["up"] == out["episodes"]
    assert set(out["loss"]) == {"lord", "down"}
    assert all(v is not None and math.isfinite(v) for v in out["loss"].values()), out["loss"]
    assert glue.QNet not in copies                                           # no target network was made
    assert seen and all(t is (glue.ReturnBatch if fused == "packed" else dict) for t in seen)
    for r in ("lord", "down"):
        assert any(not torch.equal(a, p.detach().cpu()) for a, p in zip(start[r], nets[r].parameters())), r
