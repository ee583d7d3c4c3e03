"""The ways the weights of a LIVE network change under the objects that act with it (numpy / torch only, any device): the cases of
tests/test_moving_weights_cpu.py and tests/test_gpu_moving_weights.py.

Every front end that plays from a QNet keeps tables derived from the weights alone (dqn_glue.FactorisedQ / RoleQ), cached behind
_versions() -- (id, data_ptr, _version) per parameter.  A move is applied to the SAME network object the front end holds; the
tests then ask whether the long-lived object plays the new weights.

  MOVES   name -> (apply(glue, net, seed), seen): `seen` = whether _versions() reports the move.  Only a write through `.data`
          is not seen (it bumps no version counter and keeps the address): unsupported unless followed by refresh(force=True).
  adam    three mc_step's with torch.optim.Adam(net.parameters(), LEARNING_RATE) -- the optimizer train() builds -- on a fixed
          synthetic batch (s0 / a0 0/1 planes, ret standard normal, seeded)
  sgd     one plain SGD step on the same batch: a different in-place kernel
  perturb p.add_(0.01 * randn_like(p)) under no_grad, as the learner twin tests do
  load    net.load_state_dict(other.state_dict()): train()'s target copy, _compete_net's load
  assign  net.load_state_dict(sd, assign=True): new Parameter objects, versions that may be equal
  swap    two parameters replaced by new nn.Parameter objects
  one_tensor_fc2_bias / one_tensor_conv_shunzi   ONE parameter moves: a version tuple or a refresh that misses a parameter
          (conv_shunzi.weight feeds base's neighbours Mz_f, Z and W2x; fc2.bias feeds b2 alone)
  data_write   p.data.mul_(1.25) on every parameter

The vacuity guard is on the reference alone: assert_moved() takes the literal network's fp64 q (q_reference.literal_q on
copy.deepcopy(net).double()) of the test's rows before and after the move and requires median |dq| > 1e-3 -- 100 x the 1e-5 the
kernels are compared at -- and |q| < 1 on both sides, the range that bound is stated for.  (Adam at 1e-4 moves some rows by 1e-4
and others by 0.3: hence the median.)  The sizes of sgd, one_tensor_* and data_write are chosen so that the guard holds; the
measured medians are in profiles/r26_notes.md."""
import copy

import numpy as np
import torch
import torch.nn as nn

import q_reference as R

MEDIAN_MOVE = 1e-3        # the reference's median |dq| must exceed this
Q_RANGE = 1.0             # and |q_ref| stay below this: the range tests/test_gpu_qnet.py's 1e-5 is stated for
Q_BOUND = 1e-5            # |fp32 factorised q - fp64 literal q|, absolute (tests/test_gpu_qnet.py's own bound)
SGD_LR = 0.005
ONE_TENSOR_BIAS = 0.05    # fc2.bias += this: every q moves by exactly it
ONE_TENSOR_SHUNZI = 0.05  # conv_shunzi.weight += this * randn
DATA_FACTOR = 1.25


def synthetic_batch(net, seed, n=32):
    """{"s0" f32 [n,P,15,4], "a0" f32 [n,15,4] 0/1 planes, "ret" f32 [n] standard normal} on the network's device, from the seed"""
    g = torch.Generator().manual_seed(int(seed))
    dev = next(net.parameters()).device
    s0 = torch.randint(0, 2, (n, net.planes, 15, 4), generator=g).float()
    a0 = torch.randint(0, 2, (n, 15, 4), generator=g).float()
    return {"s0": s0.to(dev), "a0": a0.to(dev), "ret": torch.randn(n, generator=g).to(dev)}


def _other(glue, net, seed):
    torch.manual_seed(1000 + int(seed))
    return glue.QNet(net.planes).to(next(net.parameters()).device)


def _randn_like(p, seed):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(p.shape, generator=g).to(p.device)


def adam(glue, net, seed):
    opt = torch.optim.Adam(net.parameters(), glue.LEARNING_RATE)
    batch = synthetic_batch(net, seed)
    for _ in range(3):
        glue.mc_step(net, opt, batch)


def sgd(glue, net, seed):
    glue.mc_step(net, torch.optim.SGD(net.parameters(), SGD_LR), synthetic_batch(net, seed))


def perturb(glue, net, seed):
    with torch.no_grad():
        for k, p in enumerate(net.parameters()):
            p.add_(0.01 * _randn_like(p, seed * 100 + k))


def load(glue, net, seed):
    net.load_state_dict(_other(glue, net, seed).state_dict())


def assign(glue, net, seed):
    net.load_state_dict(_other(glue, net, seed).state_dict(), assign=True)


def swap(glue, net, seed):
    other = _other(glue, net, seed)
    net.fc1.weight = nn.Parameter(other.fc1.weight.detach().clone())
    net.conv2.weight = nn.Parameter(other.conv2.weight.detach().clone())


def one_tensor_fc2_bias(glue, net, seed):
    with torch.no_grad():
        net.fc2.bias.add_(ONE_TENSOR_BIAS)


def one_tensor_conv_shunzi(glue, net, seed):
    with torch.no_grad():
        net.conv_shunzi.weight.add_(ONE_TENSOR_SHUNZI * _randn_like(net.conv_shunzi.weight, seed))


def data_write(glue, net, seed):
    for p in net.parameters():
        p.data.mul_(DATA_FACTOR)


# name -> (apply, seen by _versions())
MOVES = {
    "adam": (adam, True), "sgd": (sgd, True), "perturb": (perturb, True), "load": (load, True), "assign": (assign, True),
    "swap": (swap, True), "one_tensor_fc2_bias": (one_tensor_fc2_bias, True),
    "one_tensor_conv_shunzi": (one_tensor_conv_shunzi, True), "data_write": (data_write, False),
}
SEEN = [name for name, (_, seen) in MOVES.items() if seen]


def apply(name, glue, net, seed=0):
    """the move on the live network object; the network stays in the mode (train / eval) it was in"""
    MOVES[name][0](glue, net, seed)


def reference_q(net, face, rows):
    """fp64 q of every (face[i], rows[i]) pair by the literal network on the CURRENT weights: a deep copy, so the live network
    and its version counters are not touched"""
    return R.literal_q(copy.deepcopy(net).cpu().double().eval(), face, rows)


def assert_moved(q_before, q_after):
    """the vacuity guard on two reference_q results; returns the median |dq|"""
    q_before, q_after = q_before.double(), q_after.double()
    assert float(q_before.abs().max()) < Q_RANGE and float(q_after.abs().max()) < Q_RANGE, \
        (float(q_before.abs().max()), float(q_after.abs().max()))
    median = float((q_after - q_before).abs().median())
    assert median > MEDIAN_MOVE, median
    return median


def constructed_rows(P, seed, tables=16, per_table=4):
    """tables x per_table rows on random 0/1 faces: (face f32 [T,P,15,4], rows int8 [N,16] count rows -- 0..4 cards of at most
    five ranks, a joker once --, offsets int32 [T+1], table of every row int64 [N])"""
    g = np.random.default_rng(int(seed))
    T, N = int(tables), int(tables) * int(per_table)
    face = torch.from_numpy(g.integers(0, 2, (T, P, 15, 4)).astype(np.float32))
    rows = np.zeros((N, 16), dtype=np.int8)
    for i in range(N):
        for r in g.choice(15, size=int(g.integers(1, 6)), replace=False):
            rows[i, r] = 1 if r >= 13 else int(g.integers(1, 5))
    offsets = torch.arange(0, N + 1, per_table, dtype=torch.int32)
    return face, torch.from_numpy(rows), offsets, torch.arange(N) // per_table
