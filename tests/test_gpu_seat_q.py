"""GPU (-m gpu): per-role Q-networks in one shared-rows forward (csrc/ddz_qnet.h section 7; dqn_glue.RoleQ), the SeatLoop built
on it and the batched Game.compete: q of every network table bit for bit what the single-network form of its role's network
gives, the (slot, rank) row layout, rule tables left out of the chain, the loop against the same loop built from the existing
calls, graph capture with a rule role, and compete against plain step_auto loops."""
import copy
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANES = {1: 7, 2: 9, 3: 6}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _dev():
    return torch.device("cuda:0")


def _nets(glue, P):
    out = []
    for seed in (11, 12, 13):
        torch.manual_seed(seed)
        out.append(glue.QNet(P).to(_dev()).eval())
    return out


def _maps(A, B, C):
    return [{"lord": A, "down": A, "up": A}, {"lord": A, "down": B, "up": B}, {"lord": None, "down": B, "up": C},
            {"lord": A, "down": B, "up": None}, {"lord": A, "down": B, "up": C}]


QSH_COLS = 625 * 441      # csrc/ddz_qnet.h section 5: (hand, taken, b1, b2) in 0..4 x (n1, n2) in 0..20
QSH_KEYS = 15 * QSH_COLS


def _direct_key(state):
    """the direct-addressed key of section 5 (variant 3) from the packed states (int64 [T, 15]), restated on the CPU"""
    st = state.cpu().view(-1, 11, 16).long()
    T = st.shape[0]
    role = st[:, 10, 0].clone()
    role[role > 2] = 0
    ar = torch.arange(T)
    rm1, rp1 = (role + 2) % 3, (role + 1) % 3
    c4 = lambda x: x.clamp(max=4)                                             # noqa: E731
    hand, taken = c4(st[ar, role, :15]), c4(st[:, 9, :15])
    b1, b2 = c4(st[ar, 6 + rm1, :15]), c4(st[ar, 6 + rp1, :15])
    n1, n2 = st[ar, rp1, 15].clamp(max=20), st[ar, rm1, 15].clamp(max=20)
    g = torch.gcd(n1, n2).clamp(min=1)
    total = torch.where(torch.arange(15) < 13, 4, 1)[None, :]
    ncode = torch.where(hand + taken >= total, torch.zeros(1, dtype=torch.long), ((n1 // g) * 21 + n2 // g)[:, None])
    return torch.arange(15)[None, :] * QSH_COLS + (((hand * 5 + taken) * 5 + b1) * 5 + b2) * 441 + ncode


def _key(state, variant):
    """the hashed key of section 5b (variants 1 / 2) from the packed states (int64 [T, 15]), restated on the CPU (a copy of the
    helper of tests/test_gpu_shared_rows_cooperation.py)"""
    st = state.cpu().view(-1, 11, 16).long()
    T = st.shape[0]
    role = st[:, 10, 0].clone()
    role[role > 2] = 0
    ar = torch.arange(T)
    rm1, rp1 = (role + 2) % 3, (role + 1) % 3
    c4 = lambda x: x.clamp(max=4)                                             # noqa: E731
    hand, taken = c4(st[ar, role, :15]), c4(st[:, 9, :15])
    fields = [hand, taken, c4(st[ar, 3 + rm1, :15]), c4(st[ar, 3 + role, :15]), c4(st[ar, 3 + rp1, :15])]
    if variant == 2:
        fields += [c4(st[ar, 6 + rm1, :15]), c4(st[ar, 6 + rp1, :15])]
    n1, n2 = st[ar, rp1, 15].clamp(max=20), st[ar, rm1, 15].clamp(max=20)
    g = torch.gcd(n1, n2).clamp(min=1)
    total = torch.where(torch.arange(15) < 13, 4, 1)[None, :]
    ncode = torch.where(hand + taken >= total, torch.zeros(1, dtype=torch.long), ((n1 // g) * 21 + n2 // g)[:, None])
    key = torch.arange(15)[None, :].expand(T, 15).clone()
    for f in fields:
        key = (key << 3) | f
    return (key << 9) | ncode


@pytest.mark.parametrize("T", [37, 700, 5000])
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_role_q_equals_the_single_network_form(pkg, glue, variant, T):
    """q[t, :counts[t]] of every network table bit for bit FactorisedQ(net of t's role).needed(shared="all") + q_slab, rule
    tables' rows untouched (NaN sentinel), a sample within 1e-5 of the literal network, a clean status word."""
    P = PLANES[variant]
    A, B, C = _nets(glue, P)
    cpu = {id(n): copy.deepcopy(n).cpu() for n in (A, B, C)}
    fqs = {id(n): glue.FactorisedQ(n) for n in (A, B, C)}
    for mi, m in enumerate(_maps(A, B, C)):
        env = pkg.BatchedEnv(T, seed=100 + 7 * mi + variant, device=_dev())
        env.reset()
        rq = glue.RoleQ(m, variant)
        assert rq.N == len({id(v) for v in m.values() if v is not None})
        for k in (0, 7, 30, 61):
            if k:
                env.rollout_random(k)
            env.legal_slab()
            face = env.observe(variant)
            q = torch.full((T, env.slab_stride), float("nan"), device=_dev())
            nu = rq.needed(env, face)
            rq.q_slab(env, nu, q)
            counts = env.counts.long()
            valid = torch.arange(env.slab_stride, device=_dev())[None, :] < counts[:, None]
            role = env.role.long()
            net_of_t = [m.get(r) for r in glue.ROLE_ORDER]
            slot = nu.slot.long()
            want_slot = torch.tensor(rq.net_of_role, device=_dev())[role]
            assert torch.equal(slot, want_slot)
            for ri, net in enumerate(net_of_t):
                mine = (role == ri)[:, None] & valid
                if net is None:
                    assert bool(torch.isnan(q[role == ri]).all())
                    continue
                fq = fqs[id(net)]
                ref = fq.q_slab(env, fq.needed(env, face, shared="all"), out=torch.zeros_like(q))
                assert torch.equal(q[mine], ref[mine])
            # the literal network on a sample of network tables' moves
            off, lrows, _ = env.slab_to_csr(rows_per_table=512)
            n = int(off[-1])
            seg_t = torch.repeat_interleave(torch.arange(T), counts.cpu())
            pick = torch.arange(0, n, 11)
            pick = pick[(slot.cpu()[seg_t[pick]] >= 0)]
            if pick.numel():
                acts = (lrows.cpu()[pick, :15].float()[:, :, None] > torch.arange(4)[None, None, :]).float()
                tq = q[valid].cpu()[pick]
                with torch.no_grad():
                    for ri, net in enumerate(net_of_t):
                        sel = role.cpu()[seg_t[pick]] == ri
                        if net is None or not bool(sel.any()):
                            continue
                        want = cpu[id(net)](face.cpu()[seg_t[pick][sel]], acts[sel])[:, 0]
                        assert float((tq[sel] - want).abs().max()) < 1e-5
        assert env.status() == 0
        env.close()


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_role_rows_layout(pkg, glue, variant):
    """(t, r) of a network table in its (slot, rank) segment, its representative's face column bit for bit its own, rows and keys
    in bijection per (slot, rank), the rows-needed word = the distinct (slot, rank, key) triples over network tables, rule tables
    rows -1 and no D rows, padding rep -1 and zero; a one-slot map writes the single-network srows / sseg / dseg words."""
    P, T = PLANES[variant], 3000
    A, B, C = _nets(glue, P)
    env = pkg.BatchedEnv(T, seed=5, device=_dev())
    env.reset()
    env.rollout_random(23)
    env.legal_slab()
    face = env.observe(variant)
    for m in _maps(A, B, C):
        rq = glue.RoleQ(m, variant)
        nu = rq.needed(env, face)
        w = next(iter(rq._ws.values()))
        scap, cap = w["scap"], w["cap"]
        rows, rep, seg = w["srows"].cpu().long(), w["srep"].cpu().long(), w["sseg"].cpu().long()
        slot = nu.slot.cpu().long()
        net_t = slot >= 0
        assert bool((rows[~net_t] == -1).all()) and bool((rows[:, 15] == -1).all())
        assert bool((nu.row_index.cpu()[~net_t] == -1).all())                  # no D row for a rule table
        key = _key(env.state, variant) if variant != 3 else _direct_key(env.state)
        ys = w["ys"].cpu()
        f = face.cpu()
        for s in range(rq.N):
            sg = seg[s].tolist()
            assert sg[33] == 0
            mine = slot == s
            total_s = 0
            for r in range(15):
                rr = rows[mine, r]
                lo, hi = s * scap + sg[r], s * scap + (sg[r + 1] if r < 14 else sg[15])
                assert bool(((rr >= lo) & (rr < hi)).all())
                total_s += torch.unique(rr).numel()
                kr = key[mine][:, r]
                pairs = torch.unique(torch.stack([kr, rr], 1), dim=0)
                assert pairs.shape[0] == torch.unique(kr).numel() == torch.unique(rr).numel()   # a bijection
                if variant == 3:
                    # direct addressing with the slot in front (s * 15 * QSH_COLS + key): rows in key order inside the segment
                    ks = torch.unique(s * QSH_KEYS + kr)
                    assert torch.equal(rr, lo + torch.searchsorted(ks, s * QSH_KEYS + kr))
            assert total_s == sg[32]
            # representatives: the row's face column bit for bit the instance's own
            tt = torch.nonzero(mine)[:, 0]
            for r in range(15):
                rr = rows[tt, r]
                inst = rep[rr]
                src_t, src_r = inst >> 4, inst & 15
                assert bool((src_r == r).all())
                assert torch.equal(f[src_t, :, r].reshape(-1, 4 * P).view(torch.int32),
                                   f[tt, :, r].reshape(-1, 4 * P).view(torch.int32))
                assert torch.equal(ys[rr, 256:256 + 4 * P].view(torch.int32), f[tt].permute(0, 2, 1, 3)[:, r].reshape(-1, 4 * P).view(torch.int32))
            pad = rep[s * scap:(s + 1) * scap] < 0
            assert int((~pad).sum()) == sg[32] and bool((ys[s * scap:(s + 1) * scap][pad] == 0).all())
        if rq.N == 1 and variant == 3:
            fq = glue.FactorisedQ(A)
            fq.needed(env, face, shared="all")
            w1 = fq._ws[("needed", face.device, T)]
            assert torch.equal(w1["srows"], w["srows"]) and torch.equal(w1["sseg"], w["sseg"][0])
            assert torch.equal(w1["dseg"], w["dseg"][0])      # (rep: any instance of the key -- the mark kernel's race winner)
    assert env.status() == 0


def _reference_step(env, fqs, m, eps, q, variant, face):
    """one SeatLoop iteration from the existing calls: FactorisedQ per network, select_slab, slab_ids, auto_choose, step_slab"""
    pkg = importlib.import_module("doudizhu-rl_amd")
    role = env.role.long()
    ids = torch.full((env.T,), -1, dtype=torch.int32, device=_dev())
    auto_roles = sum(1 << k for k, r in enumerate(("up", "lord", "down")) if m.get(r) is None)
    for k, r in enumerate(("up", "lord", "down")):
        net = m.get(r)
        if net is None:
            continue
        fq = fqs[id(net)]
        qq = fq.q_slab(env, fq.needed(env, face, shared="all"), out=q)
        choice = env.select_slab(qq, eps.get(r, 0.0))
        nid = env.slab_ids().gather(1, choice.clamp(min=0).long()[:, None])[:, 0]
        ids = torch.where(role == k, nid, ids)
    if auto_roles:
        auto = env.auto_choose(auto_roles)
        ids = torch.where(auto >= 0, auto, ids)
    out = env.step_slab(ids, pkg.STEP_IDS, auto_reset=True)
    env.observe(variant, out=face)
    return ids, out


def test_seat_loop_equals_the_loop_from_existing_calls(pkg, glue):
    """T = 1500, 40 iterations, variant 2: lord A (epsilon 0.2) against rule farmers, and a rule lord against farmers B / C --
    states, the played ids and done / r bit for bit after every iteration."""
    T, variant = 1500, 2
    A, B, C = _nets(glue, 9)
    fqs = {id(n): glue.FactorisedQ(n) for n in (A, B, C)}
    for m, eps in (({"lord": A}, {"lord": 0.2}), ({"down": B, "up": C}, {})):
        a = pkg.BatchedEnv(T, seed=77, device=_dev())
        b = pkg.BatchedEnv(T, seed=77, device=_dev())
        a.reset(); b.reset()
        loop = glue.SeatLoop(a, m, variant, epsilon=eps)
        b.legal_slab()
        face = b.observe(variant)
        q = torch.zeros((T, b.slab_stride), device=_dev())
        for _ in range(40):
            da, ra, ia = loop.step()
            ids, (db, rb, ib) = _reference_step(b, fqs, m, eps, q, variant, face)
            assert torch.equal(loop.ids, ids)
            assert torch.equal(da, db) and torch.equal(ra, rb) and torch.equal(ia, ib)
            assert torch.equal(a.state, b.state) and torch.equal(loop.face, face)
        assert a.stats() == b.stats() and a.status() == 0 and b.status() == 0


def test_seat_loop_is_graph_capturable_with_a_rule_role(pkg, glue):
    """6 iterations captured with a rule role in the map, replayed 3 times == 18 eager iterations, bit for bit."""
    T, K, variant = 1500, 6, 2
    A, B, _ = _nets(glue, 9)
    for m in ({"lord": A}, {"lord": A, "down": B}):
        a = pkg.BatchedEnv(T, seed=21, device=_dev())
        b = pkg.BatchedEnv(T, seed=21, device=_dev())
        a.reset(); b.reset()
        la = glue.SeatLoop(a, m, variant, epsilon={"lord": 0.1})
        lb = glue.SeatLoop(b, m, variant, epsilon={"lord": 0.1})
        la.run(2); lb.run(2)
        g = la.capture(K)
        for _ in range(3):
            g.replay()
            lb.run(K)
        torch.cuda.synchronize()
        assert torch.equal(a.state, b.state) and torch.equal(la.face, lb.face) and torch.equal(la.ids, lb.ids)
        assert a.stats() == b.stats() and a.status() == 0


def test_compete(pkg, glue, tmp_path):
    """all-rule compete == a step_auto(0b111) loop's stats; a network map == SeatLoop's stats; wins sum to the episodes (>= total);
    a WinRateBook fed by compete holds the same totals; a checkpoint by path == the in-memory network."""
    metrics = importlib.import_module("doudizhu-rl_amd.metrics")
    T = 512
    res = glue.compete(2, {}, total=300, tables=T, seed=3)
    env = pkg.BatchedEnv(T, seed=3, device=_dev())
    env.reset(); env.legal_slab()
    s0 = env.stats()
    for _ in range(res["iterations"]):
        env.step_auto(0b111, slab=True)
    s1 = env.stats()
    assert res["episodes"] == s1["episodes"] - s0["episodes"] >= 300
    assert (res["lord"], res["down"], res["up"]) == tuple(s1[k] - s0[k] for k in ("lord_wins", "down_wins", "up_wins"))
    assert res["lord"] + res["down"] + res["up"] == res["episodes"]
    torch.manual_seed(0)
    net = glue.QNet(9).to(_dev()).eval()
    book = metrics.WinRateBook()
    res = glue.compete(2, {"lord": net}, total=200, tables=T, seed=4, book=book)
    assert res["lord"] + res["down"] + res["up"] == res["episodes"] >= 200
    assert book.episodes == res["episodes"] and all(book.total[r] == res[r] for r in ("lord", "down", "up"))
    env = pkg.BatchedEnv(T, seed=4, device=_dev())
    env.reset(); env.legal_slab()
    loop = glue.SeatLoop(env, {"lord": net}, 2)
    s0 = env.stats()
    loop.run(res["iterations"])
    s1 = env.stats()
    assert res["episodes"] == s1["episodes"] - s0["episodes"] and res["lord"] == s1["lord_wins"] - s0["lord_wins"]
    path = metrics.save_state_dict(net, str(tmp_path), "lord_net.pt")
    res2 = glue.compete(2, {"lord": path}, total=200, tables=T, seed=4)
    assert res2 == res


def test_seat_loop_lord_net_rule_farmers_full_size_with_oracle_slice(pkg, glue, oracle):
    """65,536 tables, EnvCooperation faces, lord = QNet(9) (torch.manual_seed(0), eval, greedy), farmers = the rule agent: tables
    [4096, 6144) are stepped by the oracle -- the lord's move from the SAME q values (the oracle's arg-max), the farmers' from
    the oracle's own rule agent -- played ids, done / r and full states bit-exact every iteration; the faces against the
    oracle's, the lord tables' q against the literal network (fp32, 1e-5) and the farmer tables' q untouched on the slice."""
    T, iters, lo, n = 65536, 8, 4096, 2048
    torch.manual_seed(0)
    net = glue.QNet(9).to(_dev()).eval()
    net_cpu = copy.deepcopy(net).cpu()
    env = pkg.BatchedEnv(T, seed=77, device=_dev())
    ref = oracle.OracleEnv(n, seed=77, gid_base=lo)
    env.reset(); ref.reset()
    loop = glue.SeatLoop(env, {"lord": net, "down": None, "up": None}, 2)
    lords = 0
    for it in range(iters):
        loop.q.fill_(float("nan"))
        loop.act()
        rauto = ref.auto_choose(0b101)
        off, rrows, rids = ref.legal()
        cnt = np.diff(off)
        assert np.array_equal(env.counts[lo:lo + n].cpu().numpy(), cnt)
        is_lord = env.role[lo:lo + n].cpu().numpy() == 1
        assert np.array_equal(rauto >= 0, ~is_lord)
        assert np.array_equal(loop.slot[lo:lo + n].cpu().numpy() >= 0, is_lord)
        qs = loop.q[lo:lo + n].cpu().numpy()
        assert np.isnan(qs[~is_lord]).all()                                   # rule tables: q left alone
        qcsr = np.concatenate([qs[t, :cnt[t]] if is_lord[t] else np.zeros(cnt[t], np.float32) for t in range(n)])
        rchoice = ref.select(qcsr)
        want_ids = np.where(is_lord, rids[off[:-1] + rchoice], rauto).astype(np.int32)
        assert np.array_equal(loop.ids[lo:lo + n].cpu().numpy(), want_ids), it
        assert np.array_equal(loop.choice[lo:lo + n].cpu().numpy()[is_lord], rchoice[is_lord]), it
        lords += int(is_lord.sum())
        if it % 3 == 0 and is_lord.any():
            tl = np.nonzero(is_lord)[0]
            seg = torch.from_numpy(np.concatenate([np.full(cnt[t], t) for t in tl]))
            rows_l = np.concatenate([rrows[off[t]:off[t + 1]] for t in tl])
            acts = (torch.from_numpy(rows_l[:, :15].astype(np.float32))[:, :, None] > torch.arange(4)[None, None, :]).float()
            ql = torch.from_numpy(np.concatenate([qs[t, :cnt[t]] for t in tl]))
            with torch.no_grad():
                want = net_cpu(loop.face[lo:lo + n].cpu()[seg], acts)[:, 0]
            assert float((ql - want).abs().max()) < 1e-5
            assert np.array_equal(loop.face[lo:lo + n].cpu().numpy().view(np.uint32), ref.observe(2).view(np.uint32))
        done, rew, ill = loop.apply()
        rdone, rrew, rill, _ = ref.step(oracle.STEP_IDS, want_ids, auto_reset=True)
        assert not bool(ill.any()) and not rill.any()
        assert np.array_equal(done[lo:lo + n].cpu().numpy(), rdone) and np.array_equal(rew[lo:lo + n].cpu().numpy(), rrew)
        assert np.array_equal(env.state.view(T, -1)[lo:lo + n].cpu().numpy().reshape(-1), ref.state), it
    assert lords > iters * n // 5                                          # the lord moved on the slice in most iterations
    w = next(iter(loop.rq._ws.values()))
    assert int(w["sseg"].cpu()[0, 33]) == 0 and int(w["dseg"].cpu()[0, 33]) == 0
    assert env.status() == 0 and env.stats()["plies"] == T * iters
