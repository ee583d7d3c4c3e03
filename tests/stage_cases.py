"""Operands and an fp64 statement for the learner's whole pre-fc1 stage (include/ddz_env.h: ddz_q_stage_fwd / ddz_q_stage_bwd), shared
by tests/test_stage_cpu.py and tests/test_gpu_stage.py.  numpy / CPU torch only; the recipes of tests/first_layer_cases.py with
conv_shunzi's parameters and a gradient gh [n,4864] added; written from the header's expressions, not from
doudizhu-rl_amd/dqn_glue.py.

  exact_case   first_layer_cases.exact_case + ws integers in -8..8 over 8, bs integers in -16..16 over 8, gh's z columns integers in
               -32..32 over 8: with 0 / 1 inputs every product and every partial sum of any order is a multiple of 1 / 64 far below
               2^24 / 64, so fp32 in ANY summation order equals fp64.
  random_case  first_layer_cases.random_case + standard-normal ws, bs and z columns of gh.
  statement    first_layer_cases.statement on the y columns + z, gws, gbs in fp64 with sum |terms| for the bounds.
"""
import types

import torch

import first_layer_cases as flc

PLANES, H = flc.PLANES, flc.H
Y, Z = 15 * H, 4 * H            # 3840 first-layer columns of h, then conv_shunzi's 1024
WIDTH = Y + Z


def _stage(first, ws, bs, gz):
    """a first-layer case + conv_shunzi's parameters + the z columns of gh -> the stage's case (weights / biases: all five convs;
    gy stays the first layer's gradient = the y columns of gh)"""
    c = types.SimpleNamespace(**vars(first))
    c.weights, c.biases = list(first.weights[:4]) + [ws], list(first.biases[:4]) + [bs]
    c.gz = gz
    c.gh = torch.cat((first.gy, gz), dim=1).contiguous()
    return c


def exact_case(planes, n, seed=0):
    first = flc.exact_case(planes, n, seed)
    g = torch.Generator().manual_seed(3000 * planes + seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)   # noqa: E731
    return _stage(first, ri(-8, 8, H, planes + 1, 15, 1) / 8, ri(-16, 16, H) / 8, ri(-32, 32, n, Z) / 8)


def random_case(planes, n, seed=0):
    first = flc.random_case(planes, n, seed)
    g = torch.Generator().manual_seed(4000 * planes + seed)
    return _stage(first, torch.randn((H, planes + 1, 15, 1), generator=g), torch.randn(H, generator=g),
                  torch.randn((n, Z), generator=g))


def head(case, n):
    """the first n samples of a case (the parameters are shared)"""
    c = types.SimpleNamespace(**vars(case))
    c.face, c.actions, c.gy, c.gz, c.gh = (t[:n].contiguous() for t in (case.face, case.actions, case.gy, case.gz, case.gh))
    c.n = n
    return c


def with_gh(case, gh):
    c = types.SimpleNamespace(**vars(case))
    c.gh = gh.contiguous()
    c.gy, c.gz = c.gh[:, :Y].contiguous(), c.gh[:, Y:].contiguous()
    return c


def with_shunzi(case, ws, bs=None):
    c = types.SimpleNamespace(**vars(case))
    c.weights = list(case.weights[:4]) + [ws]
    c.biases = list(case.biases[:4]) + [case.biases[4] if bs is None else bs]
    return c


def first_part(case):
    """the first_layer_cases case inside a stage case"""
    return flc._case(case.face, case.actions, case.weights[:4], case.biases[:4], case.gy)


def load(net, case):
    """the case's parameters into a QNet's five convolutions (in place)"""
    flc.load(net, first_part(case))
    with torch.no_grad():
        net.conv_shunzi.weight.copy_(case.weights[4])
        net.conv_shunzi.bias.copy_(case.biases[4])
    return net


def shunzi_terms(planes):
    """additions + 1 of z's chain: the bias and the 15 C products"""
    return 15 * (planes + 1) + 1


def x64(case):
    """x f64 [n, C, 15, 4]: the planes of face followed by the action plane"""
    return torch.cat((case.face, case.actions.unsqueeze(1)), dim=1).double()


def shunzi64(case):
    """z f64 [n,1024] (column o * 4 + j) and z_abs = sum |terms| of its chain"""
    n, x = case.n, x64(case)
    w, b = case.weights[4].double()[:, :, :, 0], case.biases[4].double()                    # [256,C,15]
    z = torch.einsum("ocr,ncrj->noj", w, x) + b[None, :, None]
    za = torch.einsum("ocr,ncrj->noj", w.abs(), x.abs()) + b.abs()[None, :, None]
    return z.reshape(n, Z), za.reshape(n, Z)


def shunzi_grads64(case):
    """gws [256,C,15,1], gbs [256] from the z columns of gh, and the same sums of |gh x| / |gh|"""
    n, x = case.n, x64(case)
    gz = case.gz.double().reshape(n, H, 4)
    gws = torch.einsum("noj,ncrj->ocr", gz, x).unsqueeze(-1)
    gws_abs = torch.einsum("noj,ncrj->ocr", gz.abs(), x.abs()).unsqueeze(-1)
    return gws, gz.sum(dim=(0, 2)), gws_abs, gz.abs().sum(dim=(0, 2))


def statement(case, arg=None, fwd=None):
    """first_layer_cases.statement of the y part (gw / gb / ... lists of four, routed by `arg`, default the statement's own) with
    conv_shunzi's appended as the fifth entry of gw / gb / gw_abs / gb_abs, and h / h_abs [n,4864] = (y, z) / their sum |terms|"""
    st = flc.statement(first_part(case), arg=arg, fwd=fwd)
    st.z, st.z_abs = shunzi64(case)
    st.h, st.h_abs = torch.cat((st.y, st.z), dim=1), torch.cat((st.abs_max, st.z_abs), dim=1)
    gws, gbs, gws_abs, gbs_abs = shunzi_grads64(case)
    st.gw, st.gb = st.gw + [gws], st.gb + [gbs]
    st.gw_abs, st.gb_abs = st.gw_abs + [gws_abs], st.gb_abs + [gbs_abs]
    return st


def literal_stage(net, face, actions):
    """QNet.forward's own lines up to the dropout (net.py:87-97)"""
    x = torch.cat((face, actions.unsqueeze(1)), dim=1)
    y = torch.cat([f(x) for f in (net.conv1, net.conv2, net.conv3, net.conv4)], -1)
    y = net.pool(y).view(actions.shape[0], -1)
    z = net.conv_shunzi(x).view(actions.shape[0], -1)
    return torch.cat([y, z], -1)
