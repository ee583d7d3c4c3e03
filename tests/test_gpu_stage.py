"""GPU (-m gpu): the learner's whole pre-fc1 stage (csrc/ddz_qtrain.h: ddz_q_stage_fwd / ddz_q_stage_bwd, engine.q_stage_fwd /
q_stage_bwd, dqn_glue.Stage / QNet.forward_stage / forward_packed / td_step on a PackedBatch / train(fused="packed")) against the
fp64 statement of tests/stage_cases.py, against the first-layer entry points, and -- the rows source -- against the faces source
on what TransitionRecorder.decode gives.

  exact case   dyadic operands: h, arg and the ten gradients EQUAL the statement, whatever the order of the sums.
  random case  z within gamma_(15 C + 1) sum |terms|, gws / gbs within gamma_(4 n) sum |gh x| (tests/q_reference.py); the y part as
               tests/test_gpu_first_layer.py bounds it.
  rows source  bit for bit the faces source on decode()'s faces and thermometers (torch.equal).
  twin run     one td_step literal on decode(index) and one packed on the same index from copies of one network: the packed
               path's error against the same step in fp64 is at most 4 x the literal fp32 path's own (floor 2^-23 max |.|), the
               criterion of tests/test_gpu_first_layer.py::test_twin_td_step.
The tiles: 8 samples per block; the blocks of both backward kernels (and of conv_shunzi's forward) stop at 512 and walk further
tiles from n = 4097 (one case of 4102)."""
import copy
import ctypes as C
import importlib
import math

import pytest
import torch

import first_layer_cases as flc
import stage_cases as sc
from q_reference import assert_exact, assert_within, gamma

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_EXACT = (1, 2, 7, 8, 9, 16, 17, 65, 257)
N_MAX = max(N_EXACT)
VARIANT_OF = {4: 0, 7: 1, 9: 2, 6: 3}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _dev(ts):
    return [t.to(DEV).contiguous() for t in ts]


_exact = {}


def exact(planes):
    """the exact case of N_MAX samples and its fp64 first-layer forward, built once per plane count; its heads are the smaller batches"""
    if planes not in _exact:
        case = sc.exact_case(planes, N_MAX)
        _exact[planes] = (case, flc.forward64(sc.first_part(case)))
    return _exact[planes]


def _run(pkg, case, arg=None):
    """(h, arg, h without arg, gw[5], gb[5]) of the kernels on the case's faces; backward routed by `arg` (default: the forward's)"""
    face, actions, gh = _dev([case.face, case.actions, case.gh])
    w, b = _dev(case.weights), _dev(case.biases)
    h, a = pkg.q_stage_fwd(w, b, face=face, actions=actions)
    h0, none = pkg.q_stage_fwd(w, b, want_arg=False, face=face, actions=actions)
    assert none is None
    gw, gb = pkg.q_stage_bwd(gh, a if arg is None else arg.to(DEV), w, face=face, actions=actions)
    return h.cpu(), a.cpu(), h0.cpu(), [t.cpu() for t in gw], [t.cpu() for t in gb]


def _assert_equal_statement(got, st, case):
    h, a, h0, gw, gb = got
    assert h.shape == (case.n, sc.WIDTH)
    assert_exact(h, st.h, st.h_abs, scale=64)
    assert torch.equal(h0, h)
    assert a.dtype == torch.uint8 and torch.equal(a, st.arg)
    for k in range(5):
        assert gw[k].shape == case.weights[k].shape and gb[k].shape == (256,)
        assert_exact(gw[k], st.gw[k], st.gw_abs[k], scale=64)
        assert_exact(gb[k], st.gb[k], st.gb_abs[k], scale=64)


# ---- 1. exact, faces source ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", sc.PLANES)
def test_exact_case(pkg, planes):
    full, fwd_full = exact(planes)
    z = sc.shunzi64(full)[0].reshape(N_MAX, 256, 4)
    # channels 0 and 255 and slots 0 and 3 carry distinct values: a transposed index cannot pass
    corners = [z[:, o, j] for o in (0, 255) for j in (0, 3)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert bool((corners[i] != corners[j]).any())
    assert not torch.equal(z.reshape(N_MAX, 4, 256).transpose(1, 2), z)
    for n in N_EXACT:
        case = sc.head(full, n)
        _assert_equal_statement(_run(pkg, case), sc.statement(case, fwd=flc.head64(fwd_full, n)), case)


# ---- 2. index traps of the conv_shunzi part -----------------------------------------------------------------------------------
CORNERS = [(o, c, r, j) for o in (0, 255) for c in (0, -1) for r in (0, 14) for j in (0, 3)]


@pytest.mark.parametrize("planes", (4, 9))
def test_one_nonzero_gh_lands_in_one_channel(pkg, planes):
    full, _ = exact(planes)
    case = sc.head(full, 17)
    face, actions = _dev([case.face, case.actions])
    w = _dev(case.weights)
    _, a = pkg.q_stage_fwd(w, _dev(case.biases), face=face, actions=actions)
    x = sc.x64(case)                                                # [n,C,15,4]
    for i, o, j in ((0, 0, 0), (16, 0, 3), (8, 255, 0), (16, 255, 3), (7, 130, 1)):
        gh = torch.zeros_like(case.gh)
        gh[i, sc.Y + o * 4 + j] = 2.5
        gw, gb = pkg.q_stage_bwd(gh.to(DEV), a, w, face=face, actions=actions)
        gws, gbs = gw[4].cpu().double(), gb[4].cpu().double()
        want = torch.zeros_like(gws)
        want[o, :, :, 0] = 2.5 * x[i, :, :, j]
        assert torch.equal(gws, want) and bool(want.any())
        assert float(gbs[o]) == 2.5 and int((gbs != 0).sum()) == 1
        for k in range(4):                                          # nothing arrives in the first layer
            assert not bool(gw[k].any()) and not bool(gb[k].any())


@pytest.mark.parametrize("planes", (4, 9))
def test_one_nonzero_shunzi_weight(pkg, planes):
    full, _ = exact(planes)
    case = sc.head(full, 9)
    face, actions = _dev([case.face, case.actions])
    x = sc.x64(case)
    bs = case.biases[4].double()
    for o, c, r, j in CORNERS:
        c = c % (planes + 1)
        ws = torch.zeros_like(case.weights[4])
        ws[o, c, r, 0] = -1.75
        one = sc.with_shunzi(case, ws)
        h, _ = pkg.q_stage_fwd(_dev(one.weights), _dev(one.biases), want_arg=False, face=face, actions=actions)
        z = h[:, sc.Y:].cpu().double().reshape(case.n, 256, 4)
        want = bs[None, :, None].expand(case.n, 256, 4).clone()
        want[:, o, :] += -1.75 * x[:, c, r, :]
        assert torch.equal(z, want)
        assert bool((x[:, c, r, j] != 0).any())                     # (the corner is exercised)


# ---- 3. the first layer inside the stage is the first layer -------------------------------------------------------------------
@pytest.mark.parametrize("planes", sc.PLANES)
def test_first_layer_part_is_bit_equal_to_the_first_layer_entry(pkg, planes):
    case = sc.random_case(planes, 67, seed=2)
    face, actions, gh = _dev([case.face, case.actions, case.gh])
    w, b = _dev(case.weights), _dev(case.biases)
    h, a = pkg.q_stage_fwd(w, b, face=face, actions=actions)
    y, a1 = pkg.q_first_fwd(face, actions, w[:4], b[:4])
    assert torch.equal(h[:, :sc.Y], y) and torch.equal(a, a1)
    gw1, gb1 = pkg.q_first_bwd(face, actions, gh[:, :sc.Y].contiguous(), a1, w[:4])
    for junk in (None, 0.0, 1e30):                          # whatever the z part of gh holds
        g = gh.clone()
        if junk is not None:
            g[:, sc.Y:] = junk
        gw, gb = pkg.q_stage_bwd(g, a, w, face=face, actions=actions)
        for k in range(4):
            assert torch.equal(gw[k], gw1[k]) and torch.equal(gb[k], gb1[k])


# ---- 4. beyond the cap of partials ----------------------------------------------------------------------------------------------
def test_exact_case_beyond_the_cap_of_partials(pkg):
    """n = 4102 = 8 x 512 + 6: 513 tiles on 512 blocks -- block 0 of each backward kernel and of conv_shunzi's forward walks two
    tiles, the second one partial.  The batch is 293 samples fourteen times over with a gh of its own per repeat: h and arg
    repeat, and the gradients -- linear in gh -- are the statement's on the 293 with the sum of the fourteen gh (sum |terms|
    from the sum of their absolute values)."""
    base, reps = sc.exact_case(9, 293, seed=5), 14
    g = torch.Generator().manual_seed(9)
    ghs = [torch.randint(-32, 33, base.gh.shape, generator=g).float() / 8 for _ in range(reps)]
    fwd = flc.forward64(sc.first_part(base))
    st = sc.statement(sc.with_gh(base, sum(ghs)), fwd=fwd)
    st_abs = sc.statement(sc.with_gh(base, sum(x.abs() for x in ghs)), fwd=fwd)
    st.gw_abs, st.gb_abs = st_abs.gw_abs, st_abs.gb_abs
    st.h, st.arg, st.h_abs = st.h.repeat(reps, 1), st.arg.repeat(reps, 1), st.h_abs.repeat(reps, 1)
    case = sc.with_gh(base, torch.cat(ghs))
    case.face, case.actions, case.n = base.face.repeat(reps, 1, 1, 1), base.actions.repeat(reps, 1, 1), 293 * reps
    assert case.n == 4102
    _assert_equal_statement(_run(pkg, case), st, case)


# ---- 5. random case -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", sc.PLANES)
def test_random_case(pkg, planes):
    case = sc.random_case(planes, 67)
    st = sc.statement(case)
    h, a, h0, gw, gb = _run(pkg, case, arg=st.arg)                 # backward routed by the statement's arg
    assert torch.equal(h0, h)
    nt = flc.forward_terms(planes)
    assert_within(h[:, :sc.Y], st.y, st.abs_max, nt)
    assert_within(h[:, sc.Y:], st.z, st.z_abs, sc.shunzi_terms(planes))
    decided = st.margin > 2 * gamma(nt) * st.abs_max              # both of the two largest chains within the forward bound
    skipped = 1.0 - float(decided.double().mean())
    print(f"planes {planes}: arg compared on {1 - skipped:.6f} of the elements")
    assert skipped <= 0.01
    assert torch.equal(a[decided], st.arg[decided])
    for k in range(4):
        m = st.rows[k].clamp(min=1)
        assert_within(gw[k], st.gw[k], st.gw_abs[k], m[:, None, None, None].expand_as(st.gw[k]))
        assert_within(gb[k], st.gb[k], st.gb_abs[k], m)
    assert_within(gw[4], st.gw[4], st.gw_abs[4], 4 * case.n)
    assert_within(gb[4], st.gb[4], st.gb_abs[4], 4 * case.n)


# ---- 6. rows source == faces source, bit for bit --------------------------------------------------------------------------------
_loops = {}


def _stepped_loop(pkg, glue, variant, jk=False, iterations=100):
    """(TrainLoop, {role: network of the variant's planes}): a TrainLoop at 64 tables, one untrained network per role, stepped until
    every ring holds finished and unfinished transitions; built once per (variant, rule set).  The rings are packed states: they
    serve every face variant, so variant 0 -- whose faces the loop's shared rows do not key -- is decoded from a loop that
    plays on variant 3, by networks of its own."""
    key = (variant, jk)
    if key not in _loops:
        play = variant or 3
        torch.manual_seed(40 + variant)
        mk = lambda v: {r: glue.QNet(pkg.FACE_PLANES[v]).to(DEV).eval() for r in ("lord", "down", "up")}   # noqa: E731
        nets = mk(play)
        env = pkg.BatchedEnv(64, seed=50 + variant, device=DEV, native_joker_kickers=jk)
        env.reset()
        env.legal_slab()
        loop = glue.TrainLoop(env, nets, play, capacity=4096, epsilon=0.1)
        loop.run(iterations)
        torch.cuda.synchronize()
        assert env.status() == 0
        _loops[key] = (loop, nets if play == variant else mk(variant))
    return _loops[key]


def _mixed_index(rec, role, n, seed):
    """n live entries of the role's ring: finished ones (written by ddz_tr_after: done = 1, a1 = pass) and unfinished ones (written
    by ddz_tr_before) alternating, with duplicates, shuffled"""
    f = rec._ring(role)
    live = min(int(rec.count(role)), rec.capacity)
    done = f["done"][:live].bool().cpu()
    d, nd = done.nonzero()[:, 0], (~done).nonzero()[:, 0]
    assert d.numel() > 0 and nd.numel() > 0, (role, live)
    g = torch.Generator().manual_seed(seed)
    if n == 1:
        return d[:1].to(DEV)
    half = (n + 1) // 2
    pick = lambda pool, k: pool[torch.randint(0, pool.numel(), (k,), generator=g)]   # noqa: E731  (with replacement: duplicates)
    index = torch.cat((pick(d, half - 1), d[:1], pick(nd, n - half - 1), nd[:1]))
    index[-2] = index[0]                                            # a certain duplicate
    return index[torch.randperm(n, generator=g)].to(DEV)


@pytest.mark.parametrize("variant,jk", ((0, False), (1, False), (2, False), (3, False), (3, True)))
def test_rows_source_equals_faces_source(pkg, glue, variant, jk):
    loop, nets = _stepped_loop(pkg, glue, variant, jk)
    rec, P = loop.rec, pkg.FACE_PLANES[variant]
    assert rec._rows.shape[0] == (13551 if jk else 13527)
    g = torch.Generator(device=DEV).manual_seed(variant)
    for role in ("lord", "down", "up"):
        net = nets[role]
        w = [cv.weight.detach() for cv in (net.conv1, net.conv2, net.conv3, net.conv4, net.conv_shunzi)]
        b = [cv.bias.detach() for cv in (net.conv1, net.conv2, net.conv3, net.conv4, net.conv_shunzi)]
        for n in (1, 9, 67):
            index = _mixed_index(rec, role, n, seed=n)
            dec = rec.decode(role, index, variant)
            pb = rec.packed(role, index, variant)
            if n > 1:
                assert bool(dec["done"].any()) and not bool(dec["done"].all())
                assert index.unique().numel() < n
                assert not bool(dec["a1"][dec["done"]].any())       # a finished transition's a1 is the pass
            gh = torch.randn((n, sc.WIDTH), generator=g, device=DEV)
            for side, (s, a_) in enumerate((("s0", "a0"), ("s1", "a1"))):
                assert tuple(dec[s].shape) == (n, P, 15, 4)
                states, ids = (pb.s0, pb.a0) if side == 0 else (pb.s1, pb.a1)
                rows = {"states": states, "ids": ids, "index": pb.index, "table": pb.table, "variant": variant}
                faces = {"face": dec[s], "actions": dec[a_]}
                h_f, arg_f = pkg.q_stage_fwd(w, b, **faces)
                h_r, arg_r = pkg.q_stage_fwd(w, b, **rows)
                assert torch.equal(h_f, h_r) and torch.equal(arg_f, arg_r), (role, n, side)
                assert torch.equal(pkg.q_stage_fwd(w, b, want_arg=False, **rows)[0], h_f)
                g_f, g_r = pkg.q_stage_bwd(gh, arg_f, w, **faces), pkg.q_stage_bwd(gh, arg_r, w, **rows)
                for x, y in zip(g_f[0] + g_f[1], g_r[0] + g_r[1]):
                    assert torch.equal(x, y), (role, n, side)
                assert bool(g_f[0][4].any()) and bool(g_f[0][0].any())
        # identity index (NULL): the whole ring in order
        whole = {"states": rec._ring(role)["s0"][:16], "ids": rec._ring(role)["a0"][:16], "table": rec._rows, "variant": variant}
        first16 = rec.decode(role, torch.arange(16, device=DEV), variant)
        assert torch.equal(pkg.q_stage_fwd(w, b, want_arg=False, **whole)[0],
                           pkg.q_stage_fwd(w, b, want_arg=False, face=first16["s0"], actions=first16["a0"])[0])


def test_sample_is_decode_of_draw_and_sample_packed_its_packed_twin(pkg, glue):
    loop, _ = _stepped_loop(pkg, glue, 3)
    rec = loop.rec
    rec.note_counts()
    torch.manual_seed(5)
    f = rec._ring("lord")
    n = f["count"][0].clamp(min=1, max=rec.capacity)
    idx = (torch.rand(33, dtype=torch.float64, device=DEV) * n.double()).long().minimum(n - 1)   # the draw sample() always made
    want = rec.decode("lord", idx, 3)
    torch.manual_seed(5)
    got = rec.sample("lord", 33, 3)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    torch.manual_seed(5)
    pb = rec.sample_packed("lord", 33, 3)
    assert torch.equal(pb.index, idx) and pb.variant == 3 and pb.n == 33
    assert pb.s0.data_ptr() == f["s0"].data_ptr() and pb.a1.data_ptr() == f["a1"].data_ptr()    # views of the ring


# ---- 7. the twin run ------------------------------------------------------------------------------------------------------------
class _Mask(torch.nn.Module):
    """dropout with a given keep mask (p = 0.5: kept values are doubled)"""

    def __init__(self, keep):
        super().__init__()
        self.keep = keep

    def forward(self, h):
        return h * self.keep * 2.0


def _step(glue, net, target, batch, seed):
    """one td_step with an optimizer that leaves the parameters alone -> (loss, gradients, the dropout keep mask)"""
    seen = []
    hook = net.drop.register_forward_hook(lambda mod, inp, out: seen.append(torch.where(inp[0] != 0, out != 0, True)))
    torch.manual_seed(seed)
    loss = glue.td_step(net, target, torch.optim.SGD(net.parameters(), lr=0.0), batch, 0.95)
    hook.remove()
    return float(loss.double()), {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()}, seen[0].cpu()


@pytest.mark.parametrize("dropout", (False, True))
@pytest.mark.parametrize("planes", (6, 9))
def test_twin_td_step(pkg, glue, planes, dropout):
    """literal on decode(index) against packed on the same index; prints both paths' errors against fp64 (profiles/r09_notes.md)"""
    variant = VARIANT_OF[planes]
    loop, _ = _stepped_loop(pkg, glue, variant)
    index = _mixed_index(loop.rec, "lord", 20, seed=3)
    dec, pb = loop.rec.decode("lord", index, variant), loop.rec.packed("lord", index, variant)
    assert bool(dec["done"].any()) and not bool(dec["done"].all())
    torch.manual_seed(11 + planes)
    net = glue.QNet(planes)
    target = copy.deepcopy(net).eval()
    with torch.no_grad():                                          # (a target that differs from the policy, as in training)
        for p in target.parameters():
            p.add_(0.01 * torch.randn_like(p))
    net.train(dropout)
    lit, pak = copy.deepcopy(net).to(DEV), copy.deepcopy(net).to(DEV)
    tl, tp = copy.deepcopy(target).to(DEV), copy.deepcopy(target).to(DEV)
    loss_l, g_l, keep_l = _step(glue, lit, tl, dec, seed=5)
    loss_p, g_p, keep_p = _step(glue, pak, tp, pb, seed=5)
    if dropout:
        assert torch.equal(keep_l, keep_p) and 0.4 < float(keep_l.float().mean()) < 0.6   # one RNG state: the literal's mask
    # the authority: the same step in fp64 on the literal network (CPU), the mask taken from the fp32 run
    net64, t64 = copy.deepcopy(net).double(), copy.deepcopy(target).double()
    if dropout:
        net64.drop = _Mask(keep_l.double())
    b64 = {k: (v.cpu().double() if v.dtype == torch.float32 else v.cpu()) for k, v in dec.items()}
    loss_64 = float(glue.td_step(net64, t64, torch.optim.SGD(net64.parameters(), lr=0.0), b64, 0.95))
    g_64 = {k: p.grad.detach() for k, p in net64.named_parameters()}
    rows = [("loss", abs(loss_l - loss_64), abs(loss_p - loss_64), 2.0 ** -23 * abs(loss_64))]
    for k in g_64:
        rows.append((k, float((g_l[k] - g_64[k]).abs().max()), float((g_p[k] - g_64[k]).abs().max()),
                     2.0 ** -23 * float(g_64[k].abs().max())))
    for name, e_l, e_p, floor in rows:
        print(f"planes {planes} dropout {dropout} {name}: literal {e_l:.3e} packed {e_p:.3e} floor {floor:.3e}")
    for name, e_l, e_p, floor in rows:
        assert e_p <= max(4 * e_l, floor), (name, e_l, e_p, floor)


# ---- 8. determinism -------------------------------------------------------------------------------------------------------------
def test_backward_is_deterministic(pkg):
    case = sc.random_case(9, 257, seed=3)
    face, actions, gh = _dev([case.face, case.actions, case.gh])
    w, b = _dev(case.weights), _dev(case.biases)
    _, a = pkg.q_stage_fwd(w, b, face=face, actions=actions)
    L = importlib.import_module("doudizhu-rl_amd._lib")
    src = L.QSrc()
    src.kind, src.planes, src.face, src.action = 0, 9, face.data_ptr(), actions.data_ptr()
    p5 = lambda ts: (C.c_void_p * 5)(*[t.data_ptr() for t in ts])   # noqa: E731
    nbytes = L.lib().ddz_q_stage_bwd_ws_bytes(257, 9)
    out = []
    for fill in (0x00, 0xFF):                                       # a workspace dirtied two ways (0xFF..: NaNs)
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        gw, gb = [torch.empty_like(x) for x in w], [torch.empty_like(x) for x in b]
        rc = L.lib().ddz_q_stage_bwd(0, C.byref(src), 257, C.c_void_p(gh.data_ptr()), sc.WIDTH, C.c_void_p(a.data_ptr()), p5(gw), p5(gb),
                                     C.c_void_p(ws.data_ptr()), nbytes, None)
        assert rc == 0
        torch.cuda.synchronize()
        out.append(gw + gb)
    for x, y in zip(*out):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    again = pkg.q_stage_bwd(gh, a, w, face=face, actions=actions)
    for x, y in zip(out[0], again[0] + again[1]):
        assert torch.equal(x, y)


# ---- 9. capture -----------------------------------------------------------------------------------------------------------------
def _learner(glue, planes, seed):
    torch.manual_seed(seed)
    net = glue.QNet(planes).to(DEV).eval()
    target = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), 1e-4, capturable=True)
    return net, target, opt


def test_captured_packed_td_step_equals_eager(pkg, glue):
    planes, n = 6, 40
    loop, _ = _stepped_loop(pkg, glue, 3)
    batch = loop.rec.packed("lord", _mixed_index(loop.rec, "lord", n, seed=8), 3)
    a_net, a_target, a_opt = _learner(glue, planes, 3)
    b_net, b_target, b_opt = _learner(glue, planes, 3)
    start = copy.deepcopy(b_net.state_dict())
    # warm-up on a side stream (libraries pick their kernels, Adam makes its state), then back to the start
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        for _ in range(3):
            glue.td_step(b_net, b_target, b_opt, batch, 0.95)
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize(DEV)
    with torch.no_grad():
        b_net.load_state_dict(start)
        for st in b_opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
    graph = torch.cuda.CUDAGraph()
    b_opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss_b = glue.td_step(b_net, b_target, b_opt, batch, 0.95)
    eager = []
    for _ in range(2):
        eager.append(float(glue.td_step(a_net, a_target, a_opt, batch, 0.95)))
    replayed = []
    for _ in range(2):
        graph.replay()
        replayed.append(float(loss_b))
    assert replayed == eager and eager[0] != eager[1]
    for (name, p), q in zip(a_net.named_parameters(), b_net.parameters()):
        assert torch.equal(p, q), name
    assert not torch.equal(a_net.conv1.weight, start["conv1.weight"])            # the steps moved the first layer
    assert not torch.equal(a_net.conv_shunzi.weight, start["conv_shunzi.weight"])   # ... and conv_shunzi


# ---- 10. errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg, glue):
    case = sc.random_case(6, 4)
    face, actions, gh = _dev([case.face, case.actions, case.gh])
    w, b = _dev(case.weights), _dev(case.biases)
    _, arg = pkg.q_stage_fwd(w, b, face=face, actions=actions)
    loop, nets = _stepped_loop(pkg, glue, 3)
    rec = loop.rec
    f = rec._ring("lord")
    rows = {"states": f["s0"], "ids": f["a0"], "index": torch.arange(4, device=DEV), "table": rec._rows, "variant": 3}
    bad = [
        lambda: pkg.q_stage_fwd(w, b, face=face.double(), actions=actions),
        lambda: pkg.q_stage_fwd(w, b, face=face[:, :5], actions=actions),               # five planes, and not contiguous
        lambda: pkg.q_stage_fwd(w, b, face=face, actions=actions[:3]),
        lambda: pkg.q_stage_fwd(w, b, face=face, actions=actions.cpu()),
        lambda: pkg.q_stage_fwd(w, b, face=face),
        lambda: pkg.q_stage_fwd(w[:4], b, face=face, actions=actions),
        lambda: pkg.q_stage_fwd([w[0], w[1], w[2], w[4], w[3]], b, face=face, actions=actions),
        lambda: pkg.q_stage_fwd(w, [x.cpu() for x in b], face=face, actions=actions),
        lambda: pkg.q_stage_fwd(w[:4] + [w[4].transpose(2, 3)], b, face=face, actions=actions),
        lambda: pkg.q_stage_bwd(gh[:3], arg, w, face=face, actions=actions),
        lambda: pkg.q_stage_bwd(gh[:, :3840], arg, w, face=face, actions=actions),
        lambda: pkg.q_stage_bwd(gh.t(), arg, w, face=face, actions=actions),
        lambda: pkg.q_stage_bwd(gh, arg.int(), w, face=face, actions=actions),
        lambda: pkg.q_stage_bwd(gh, None, w, face=face, actions=actions),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "variant": 4}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "variant": 2}),                        # nine planes against six-plane weights
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "states": f["s0"][:, :160]}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "states": f["s0"].cpu()}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "ids": f["a0"].long()}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "ids": f["a0"][:8]}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "index": rows["index"].int()}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "index": rows["index"].cpu()}),
        lambda: pkg.q_stage_fwd(w, b, **{**rows, "table": rec._rows[:, :15]}),
        lambda: nets["lord"].forward_packed(rec.packed("lord", rows["index"], 2), 0),   # a six-plane network, variant 2
        lambda: nets["lord"].forward_packed(rec.packed("lord", rows["index"], 3), 2),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises((ValueError, pkg.DdzError)):
            fn()
            raise AssertionError(f"case {i} was accepted")
    # a role without a ring
    env = pkg.BatchedEnv(8, seed=1, device=DEV)
    env.reset()
    env.legal_slab()
    one = glue.TrainLoop(env, {"lord": nets["lord"], "down": None, "up": None}, 3, capacity=64)
    for fn in (lambda: one.rec.sample_packed("up", 4, 3, at_least=1), lambda: one.rec.packed("down", rows["index"], 3),
               lambda: one.rec.sample_packed("lord", 4, 3)):                            # ... and no host-known count yet
        with pytest.raises(ValueError):
            fn()
    # the library's own answers on device pointers: an unknown variant / planes, a short workspace; n = 0 succeeds
    Lm = importlib.import_module("doudizhu-rl_amd._lib")
    L = Lm.lib()
    p = lambda t: C.c_void_p(t.data_ptr())                                              # noqa: E731
    p5 = lambda ts: (C.c_void_p * 5)(*[t.data_ptr() for t in ts])                       # noqa: E731
    src = Lm.QSrc()
    src.kind, src.planes, src.face, src.action = 0, 6, face.data_ptr(), actions.data_ptr()
    h = torch.empty((4, sc.WIDTH), device=DEV)
    gw, gb = [torch.empty_like(x) for x in w], [torch.empty_like(x) for x in b]
    nbytes = L.ddz_q_stage_bwd_ws_bytes(4, 6)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert L.ddz_q_stage_bwd(0, C.byref(src), 4, p(gh), sc.WIDTH, p(arg), p5(gw), p5(gb), p(ws), nbytes - 1, None) == -1
    assert L.ddz_q_stage_bwd(0, C.byref(src), 4, p(gh), sc.WIDTH, None, p5(gw), p5(gb), p(ws), nbytes, None) == -1
    assert L.ddz_q_stage_fwd(0, C.byref(src), 4, p5(w), p5(b), p(h), 3840, None, None) == -1
    assert L.ddz_q_stage_fwd(0, C.byref(src), 0, p5(w), p5(b), p(h), sc.WIDTH, None, None) == 0
    assert L.ddz_q_stage_bwd(0, C.byref(src), 0, p(gh), sc.WIDTH, p(arg), p5(gw), p5(gb), p(ws), 0, None) == 0
    src.planes = 5
    assert L.ddz_q_stage_fwd(0, C.byref(src), 4, p5(w), p5(b), p(h), sc.WIDTH, None, None) == -1
    src.kind, src.variant = 1, 4
    assert L.ddz_q_stage_fwd(0, C.byref(src), 4, p5(w), p5(b), p(h), sc.WIDTH, None, None) == -1
    torch.cuda.synchronize()
    # an empty batch through the Python layer, both sources
    for source in ({"face": face[:0], "actions": actions[:0]}, {**rows, "index": rows["index"][:0]}):
        h0, a0 = pkg.q_stage_fwd(w, b, **source)
        assert h0.shape == (0, sc.WIDTH) and a0.shape == (0, 3840)
        g0 = pkg.q_stage_bwd(gh[:0], a0, w, **source)
        assert all(not bool(t.any()) for t in g0[0] + g0[1])


def test_stage_function_honours_needs_input_grad(glue):
    case = sc.exact_case(7, 19)
    st = sc.statement(case)
    net = sc.load(glue.QNet(7), case).to(DEV)
    face, actions, gh = _dev([case.face, case.actions, case.gh])
    net.conv2.weight.requires_grad_(False)
    net.conv_shunzi.bias.requires_grad_(False)
    convs = (net.conv1, net.conv2, net.conv3, net.conv4, net.conv_shunzi)
    params = [p for cv in convs for p in (cv.weight, cv.bias)]
    h = glue.Stage.apply({"face": face, "actions": actions}, *params)
    assert torch.equal(h.cpu().double(), st.h)
    h.backward(gh)
    assert net.conv2.weight.grad is None and net.conv_shunzi.bias.grad is None
    for k, cv in enumerate(convs):
        if cv.weight.grad is not None:
            assert torch.equal(cv.weight.grad.cpu().double(), st.gw[k])
        if cv.bias.grad is not None:
            assert torch.equal(cv.bias.grad.cpu().double(), st.gb[k])
    net.eval()
    with torch.no_grad():
        q = net.forward_stage(face, actions)                       # the no-grad pass: q_stage_fwd without arg
    assert not q.requires_grad and q.shape == (19, 1)
    q_grad = net.forward_stage(face, actions)                      # ... and the pass through Stage: the same values
    assert q_grad.requires_grad and torch.equal(q_grad.detach(), q)
    with pytest.raises(ValueError):
        glue.Stage.apply({"face": face.clone().requires_grad_(), "actions": actions}, *params)


# ---- 11. train(fused="packed") --------------------------------------------------------------------------------------------------
def test_train_packed(glue):
    torch.manual_seed(0)
    nets = {"lord": glue.QNet(6), "down": glue.QNet(6), "up": None}
    before = {r: (copy.deepcopy(nets[r].conv1.weight.detach()), copy.deepcopy(nets[r].conv_shunzi.weight.detach())) for r in ("lord", "down")}
    res = glue.train(3, nets, 20, tables=64, seed=1, check_every=4, capacity=512, fused="packed", batch_size=32, device=DEV)
    assert res["episodes"] >= 20 and res["lord"] + res["down"] + res["up"] == res["episodes"]
    assert set(res["loss"]) == {"lord", "down"}
    for role, v in res["loss"].items():
        assert v is not None and math.isfinite(v), role
        assert not torch.equal(nets[role].conv1.weight.detach().cpu(), before[role][0])
        assert not torch.equal(nets[role].conv_shunzi.weight.detach().cpu(), before[role][1])
