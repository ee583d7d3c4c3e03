"""Operands and an fp64 statement for the learner's first layer (include/ddz_env.h: ddz_q_first_fwd / ddz_q_first_bwd), shared by
tests/test_first_layer_cpu.py and tests/test_gpu_first_layer.py.  numpy / CPU torch only; written from the header's expressions,
not from doudizhu-rl_amd/dqn_glue.py.

  exact_case   a dyadic recipe: every product and every partial sum of any order is a multiple of 1 / 64 far below 2^24 / 64, so
               fp32 in ANY summation order equals fp64 -- forward, arg-max and all eight gradients, bit for bit.
  random_case  standard-normal parameters and gy, uniform [0, 1) faces and actions (the probability planes are not 0 / 1).
  forward64 / statement    the expressions in fp64 with what the derivable bounds need: sum |terms| and the rows routed to each element.
"""
import types

import numpy as np
import torch

PLANES = (4, 6, 7, 9)
H = 256


def _case(face, actions, weights, biases, gy):
    return types.SimpleNamespace(face=face, actions=actions, weights=weights, biases=biases, gy=gy, n=face.shape[0],
                                 planes=face.shape[1])


def exact_case(planes, n, seed=0):
    """conv weights integers in -8..8 over 8, biases integers in -16..16 over 8, faces / actions 0 / 1, gy integers in -32..32
    over 8; channels o % 8 == k (k = 0..3): b_k += 64, conv k + 1 wins there; channels o % 8 == 4: zero weights and b = 0.5 in
    all four convs, a four-way tie.  fp32 tensors."""
    g = torch.Generator().manual_seed(1000 * planes + seed)
    C = planes + 1
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)   # noqa: E731
    weights = [ri(-8, 8, H, C, 1, k) / 8 for k in range(1, 5)]
    biases = [ri(-16, 16, H) / 8 for _ in range(4)]
    o = torch.arange(H)
    for k in range(4):
        biases[k][o % 8 == k] += 64.0
        weights[k][o % 8 == 4] = 0.0
        biases[k][o % 8 == 4] = 0.5
    face = ri(0, 1, n, planes, 15, 4)
    actions = ri(0, 1, n, 15, 4)
    gy = ri(-32, 32, n, 15 * H) / 8
    return _case(face, actions, weights, biases, gy)


def one_hot_gy(case, n_i, o, r, value=2.5):
    """the case with gy zero except for one (n, o, r)"""
    gy = torch.zeros_like(case.gy)
    gy[n_i, o * 15 + r] = value
    return _case(case.face, case.actions, case.weights, case.biases, gy)


def random_case(planes, n, seed=0):
    g = torch.Generator().manual_seed(2000 * planes + seed)
    C = planes + 1
    weights = [torch.randn((H, C, 1, k), generator=g) for k in range(1, 5)]
    biases = [torch.randn(H, generator=g) for _ in range(4)]
    face = torch.rand((n, planes, 15, 4), generator=g)
    actions = torch.rand((n, 15, 4), generator=g)
    gy = torch.randn((n, 15 * H), generator=g)
    return _case(face, actions, weights, biases, gy)


def load(net, case):
    """the case's parameters into a QNet's conv1..conv4 (in place)"""
    with torch.no_grad():
        for k, cv in enumerate((net.conv1, net.conv2, net.conv3, net.conv4)):
            cv.weight.copy_(case.weights[k])
            cv.bias.copy_(case.biases[k])
    return net


def forward_terms(planes):
    """additions + 1 of the longest forward chain: the bias and the 4 C products of conv4"""
    return 4 * (planes + 1) + 1


def forward64(case):
    """the forward expressions in fp64: s [n,256,15,4], y / arg [n,3840] (arg = the LOWEST k that attains the max; numpy.argmax
    returns the first), abs_max [n,3840] = the largest sum |terms| of the four chains, margin [n,3840] = the largest minus the
    second largest s_k; xk[k - 1] = conv k's input rows [(n, r), (c, j < k)]"""
    n, C = case.n, case.planes + 1
    x = torch.cat((case.face, case.actions.unsqueeze(1)), dim=1).double().permute(0, 2, 1, 3)   # [n,15,C,4]
    xk = [x[..., :k].reshape(n * 15, C * k) for k in range(1, 5)]
    s = torch.zeros((n, 15, H, 4), dtype=torch.float64)
    sa = torch.zeros_like(s)
    for k in range(1, 5):
        w, b = case.weights[k - 1].double().reshape(H, C * k), case.biases[k - 1].double()
        s[..., k - 1] = (xk[k - 1] @ w.t() + b).view(n, 15, H)
        sa[..., k - 1] = (xk[k - 1].abs() @ w.abs().t() + b.abs()).view(n, 15, H)
    s, sa = s.permute(0, 2, 1, 3), sa.permute(0, 2, 1, 3)                                       # [n,256,15,4]
    own = torch.from_numpy(np.argmax(s.numpy(), axis=-1))                                       # first occurrence of the maximum
    y = s.max(dim=-1).values
    second = s.masked_fill(torch.nn.functional.one_hot(own, 4).bool(), -np.inf).max(dim=-1).values
    return types.SimpleNamespace(n=n, C=C, xk=xk, s=s, y=y.reshape(n, -1), arg=own.reshape(n, -1).to(torch.uint8),
                                 abs_max=sa.max(dim=-1).values.reshape(n, -1), margin=(y - second).reshape(n, -1))


def head64(fwd, n):
    """forward64 of the first n samples of the case, cut from the whole case's"""
    return types.SimpleNamespace(n=n, C=fwd.C, xk=[x[: n * 15] for x in fwd.xk], s=fwd.s[:n], y=fwd.y[:n], arg=fwd.arg[:n],
                                 abs_max=fwd.abs_max[:n], margin=fwd.margin[:n])


def statement(case, arg=None, fwd=None):
    """forward64(case) (or `fwd`, when the caller has it) and -- routed by `arg` (default: the statement's own) -- gw[k] / gb[k] in
    the parameters' shapes, gw_abs / gb_abs = the same sums of |gy x| / |gy|, rows[k] [256] = the (n, r) routed to conv k + 1 per
    channel.  A new object: `fwd` is not changed."""
    fwd = forward64(case) if fwd is None else fwd
    n, C = case.n, fwd.C
    assert fwd.n == n
    out = types.SimpleNamespace(**vars(fwd))
    route = (fwd.arg if arg is None else arg).reshape(n, H, 15)
    gy = case.gy.double().reshape(n, H, 15)
    out.gw, out.gb, out.gw_abs, out.gb_abs, out.rows = [], [], [], [], []
    for k in range(1, 5):
        m = route == k - 1
        g = (gy * m).permute(0, 2, 1).reshape(n * 15, H)                                        # rows (n, r)
        out.gw.append((g.t() @ fwd.xk[k - 1]).view(H, C, 1, k))
        out.gw_abs.append((g.abs().t() @ fwd.xk[k - 1].abs()).view(H, C, 1, k))
        out.gb.append(g.sum(dim=0))
        out.gb_abs.append(g.abs().sum(dim=0))
        out.rows.append(m.sum(dim=(0, 2)).double())
    return out


def literal_first_layer(net, face, actions):
    """QNet.forward's own lines up to the pool (net.py:87-94): cat, conv1..conv4, cat, pool, view"""
    x = torch.cat((face, actions.unsqueeze(1)), dim=1)
    y = torch.cat([f(x) for f in (net.conv1, net.conv2, net.conv3, net.conv4)], -1)
    return net.pool(y).view(actions.shape[0], -1)
