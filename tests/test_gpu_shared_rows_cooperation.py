"""GPU (-m gpu): the shared-rows Q forward for the faces of EnvCooperation (variant 2, QNet(9): what the reference's train.py
trains) and EnvComplicated (variant 1, QNet(7)) -- the hashed row finder ddz_q_shared_rows_hashed (csrc/ddz_qnet.h section
5b) and everything downstream of it: the row layout against the key restated on the CPU, H0 / D / q against the dense form
and the literal network, determinism across calls / streams / graph replay, and the full-size loop against the oracle."""
import copy
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


def _key(state, variant):
    """the key of section 5b from the packed states (int64 [T, 15]), restated with torch ops on the CPU"""
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


def _csr_of_slab(env):
    off, rows, _ = env.slab_to_csr(rows_per_table=512)
    n = int(off[-1])
    return off.clone(), rows[:max(n, 1)].clone(), n


@pytest.mark.parametrize("T", [700, 37, 5000])
@pytest.mark.parametrize("P,variant", [(9, 2), (7, 1)])
def test_hashed_shared_rows_equal_the_dense_form(pkg, P, variant, T):
    """needed(shared=True) and needed(shared="all") on the hashed rows against the dense needed() on fresh deals (every lane
    of a wave inserting the same few keys) and mixed states: every (t, r) in rank r's segment, its row's representative has
    its face column bit for bit, two instances share a row exactly when their keys are equal (a lost insert race would give
    one key two rows), seg[32] = the distinct (rank, key) pairs, padding rows rep = -1 and zero; H0 within 1e-5, D bit for
    bit, q bit-identical between True and "all" and across calls and stream modes, within 1e-5 of the dense form and of the
    literal network."""
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    L = importlib.import_module("doudizhu-rl_amd._lib")
    torch.manual_seed(23 + P)
    net = glue.QNet(P).to(_dev()).eval()
    net_cpu = copy.deepcopy(net).cpu()
    env = pkg.BatchedEnv(T, seed=41 + P, device=_dev())
    env.reset()
    fq, fq2, fq3 = glue.FactorisedQ(net), glue.FactorisedQ(net), glue.FactorisedQ(net)
    K = engine.shared_row_width(P)
    for rounds in (0, 7, 30, 61):
        env.rollout_random(rounds) if rounds else None
        env.legal_slab()
        face = env.observe(variant)
        dense = fq2.needed(env, face, gemm="torch")
        nu = fq.needed(env, face, shared=True)
        w = fq._ws[("needed", face.device, T)]
        assert w["y0"] is None and w["svariant"] == variant and tuple(w["ys"].shape) == (w["scap"], K)
        rows, rep, seg = w["srows"].cpu().long(), w["srep"].cpu().long(), w["sseg"].cpu().tolist()
        assert seg[33] == 0 and seg[15] % glue.fc_tile() == 0 and seg[15] <= w["scap"]
        assert bool((rows[:, 15] == -1).all())
        cols = face.cpu().permute(0, 2, 1, 3).reshape(T * 15, P * 4)       # column of instance 15 t + r
        r15 = rows[:, :15]
        for r in range(15):
            lo, hi = seg[r], (seg[r + 1] if r < 14 else seg[15])
            assert bool(((r15[:, r] >= lo) & (r15[:, r] < hi)).all())
        inst = rep[r15]                                                   # [T,15] representative 16 t' + r'
        assert bool((inst >= 0).all()) and bool(((inst & 15) == torch.arange(15)[None, :]).all())
        assert torch.equal(cols[(inst >> 4) * 15 + (inst & 15)], cols.view(T, 15, P * 4))   # same column, bit for bit
        key = _key(env.state, variant)
        n_keys = 0
        for r in range(15):
            uk = torch.unique(key[:, r]).numel()
            pairs = torch.unique(torch.stack([key[:, r], r15[:, r]], 1), dim=0).shape[0]
            assert torch.unique(r15[:, r]).numel() == uk == pairs               # rows <-> keys: a bijection per rank
            n_keys += uk
        assert seg[32] == n_keys
        used = torch.zeros(w["scap"], dtype=torch.bool)
        used[r15.reshape(-1)] = True
        assert bool((rep[~used] == -1).all())
        pad = ~used[: seg[15]]
        if pad.any():
            assert float(w["ys"].cpu()[: seg[15]][pad].abs().max()) == 0.0
        # values: H0 up to fp32 summation order, D bit for bit (the same kernel over the same rows)
        assert float((nu.h0 - dense.h0).abs().max()) < 1e-5
        ri = nu.row_index.cpu()
        sel = ri[ri >= 0].long()
        assert torch.equal(nu.row_index, dense.row_index) and torch.equal(nu.d.cpu()[sel], dense.d.cpu()[sel])
        q = fq.q_slab(env, nu).clone()
        q2 = fq2.q_slab(env, dense)
        counts = env.counts.long()
        valid = torch.arange(env.slab_stride, device=_dev())[None, :] < counts[:, None]
        assert float((q[valid] - q2[valid]).abs().max()) < 1e-5
        # "all": D once per distinct (shared row, count) -- D bit for bit against the dense form's needed rows
        na = fq3.needed(env, face, shared="all")
        ri2 = na.row_index.cpu().long()
        need = ri >= 0
        assert torch.equal(ri2 >= 0, need) and fq3._ws[("needed", face.device, T)]["dseg"].cpu().tolist()[33] == 0
        assert torch.equal(na.d.cpu()[ri2[need]], dense.d.cpu()[ri[need].long()])
        assert float((na.h0 - nu.h0).abs().max()) == 0.0
        q3 = fq3.q_slab(env, na).clone()
        assert torch.equal(q3[valid], q[valid])
        # a second call on the same state (new insert races, possibly another numbering) and the single-stream issue:
        # bit-identical q
        assert torch.equal(fq3.q_slab(env, fq3.needed(env, face, shared="all"))[valid], q3[valid])
        fq3.two_streams = False
        assert torch.equal(fq3.q_slab(env, fq3.needed(env, face, shared="all"))[valid], q3[valid])
        fq3.two_streams = True
        # the literal network on a sample of moves
        off, lrows, n = _csr_of_slab(env)
        seg_t = torch.repeat_interleave(torch.arange(T), counts.cpu())
        pick = torch.arange(0, n, 7)
        acts = (lrows.cpu()[pick, :15].float()[:, :, None] > torch.arange(4)[None, None, :]).float()
        with torch.no_grad():
            want = net_cpu(face.cpu()[seg_t[pick]], acts)[:, 0]
        assert float((q[valid].cpu()[pick] - want).abs().max()) < 1e-5
    assert env.status() == 0
    # argument errors: another variant, too small a workspace, too small a capacity
    for bad in (0, 3):
        with pytest.raises(pkg.DdzError):
            L.check(env.lib.ddz_q_shared_rows_hashed(env._h, bad, engine._p(w["sws"]), w["sws"].numel(), w["scap"],
                                                     engine._p(w["srows"]), engine._p(w["srep"]), engine._p(w["sseg"]),
                                                     engine._stream(env.device)))
    with pytest.raises(pkg.DdzError):
        env.q_shared_rows(w["sws"][: w["sws"].numel() // 2], w["scap"], w["srows"], w["srep"], w["sseg"], variant=variant)
    small = glue.fc_tile() * ((15 * T) // glue.fc_tile())
    with pytest.raises(pkg.DdzError):
        env.q_shared_rows(w["sws"], small, w["srows"], w["srep"][:small], w["sseg"], variant=variant)
    torch.cuda.synchronize()
    assert env.status() == 0


def test_policy_loop_cooperation_shared_is_graph_capturable(pkg):
    """PolicyLoop(QNet(9), face variant 2, shared="all"): 6 iterations captured in a hipGraph and replayed 3 times == the
    same 18 iterations issued one by one (states, faces, choices and q values bit for bit) -- the row numbering of the
    hashed finder may differ between the two, the values may not."""
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    T, K = 1500, 6
    torch.manual_seed(1)
    net = glue.QNet(9).to(_dev()).eval()
    a = pkg.BatchedEnv(T, seed=21, device=_dev())
    b = pkg.BatchedEnv(T, seed=21, device=_dev())
    a.reset(); b.reset()
    la = glue.PolicyLoop(a, net, face_variant=2, epsilon=0.1, shared="all")
    lb = glue.PolicyLoop(b, net, face_variant=2, epsilon=0.1, shared="all")
    assert la.shared == "all" and "hashed" in la.describe()
    assert glue.PolicyLoop(a, net, face_variant=2).shared is False        # (the default for variant 2 stays dense)
    la.run(2); lb.run(2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            la.run(K)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        lb.run(K)
    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and torch.equal(la.face, lb.face) and torch.equal(la.choice, lb.choice)
    valid = torch.arange(a.slab_stride, device=_dev())[None, :] < a.counts.long()[:, None]
    assert torch.equal(a.counts, b.counts) and torch.equal(la.q[valid], lb.q[valid])
    assert a.status() == 0 and a.stats() == b.stats()


def test_policy_loop_cooperation_shared_full_size_with_oracle_slice(pkg, oracle):
    """65,536 tables, EnvCooperation faces, QNet(9) (torch.manual_seed(0), eval), greedy, shared="all": tables [4096, 6144)
    are stepped by the oracle from the SAME q values -- choices, done / r and full states bit-exact every iteration; the faces
    against the oracle's and the q values against the literal network on the slice (fp32, 1e-5)."""
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    T, iters, lo, n = 65536, 8, 4096, 2048
    torch.manual_seed(0)
    net = glue.QNet(9).to(_dev()).eval()
    net_cpu = copy.deepcopy(net).cpu()
    env = pkg.BatchedEnv(T, seed=77, device=_dev())
    ref = oracle.OracleEnv(n, seed=77, gid_base=lo)
    env.reset(); ref.reset()
    loop = glue.PolicyLoop(env, net, face_variant=2, epsilon=0.0, shared="all")
    for it in range(iters):
        q = loop.q_values()
        off, rrows, _ = ref.legal()
        cnt = np.diff(off)
        assert np.array_equal(env.counts[lo:lo + n].cpu().numpy(), cnt)
        qs = q[lo:lo + n].cpu().numpy()
        qcsr = np.concatenate([qs[t, :cnt[t]] for t in range(n)])
        rchoice = ref.select(qcsr)
        if it % 3 == 0:
            seg = torch.from_numpy(np.repeat(np.arange(n), cnt))
            acts = (torch.from_numpy(rrows[:, :15].astype(np.float32))[:, :, None] > torch.arange(4)[None, None, :]).float()
            with torch.no_grad():
                want = net_cpu(loop.face[lo:lo + n].cpu()[seg], acts)[:, 0]
            assert float((torch.from_numpy(qcsr) - want).abs().max()) < 1e-5
            assert np.array_equal(loop.face[lo:lo + n].cpu().numpy().view(np.uint32), ref.observe(2).view(np.uint32))
        done, rew, ill = loop.step()
        assert np.array_equal(loop.choice[lo:lo + n].cpu().numpy(), rchoice), it
        rdone, rrew, rill, _ = ref.step(oracle.STEP_CHOICE, rchoice, auto_reset=True)
        assert not bool(ill.any())
        assert np.array_equal(done[lo:lo + n].cpu().numpy(), rdone) and np.array_equal(rew[lo:lo + n].cpu().numpy(), rrew)
        assert np.array_equal(env.state.view(T, -1)[lo:lo + n].cpu().numpy().reshape(-1), ref.state), it
    w = loop.fq._ws[("needed", loop.face.device, T)]
    assert int(w["sseg"].cpu()[33]) == 0 and int(w["dseg"].cpu()[33]) == 0
    assert env.status() == 0 and env.stats()["plies"] == T * iters
