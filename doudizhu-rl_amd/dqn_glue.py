"""Batched transition assembly for the DQN loop of the reference.

The reference closes the transition of role X when X's next observation appears, or at the
terminal ply (game.py:109-167):
  * X acts in state s0 with action a0 (game.py:95-104);
  * the next time X is to move, feedback(X, done=False) stores (s0, a0, 0, s1 = face now,
    a1 = greedy action now, False) (game.py:109-127, called from :131-133, :146-148, :158-160);
  * when any role empties its hand every role with a pending (s0, a0) gets
    (s0, a0, +/-reward_dict[role], s1 = face after the terminal ply, a1 = zeros[15,4], True)
    (game.py:113-123, :134-141, :149-155, :161-167): winners +reward, losers -reward; lord and
    farmers are opposite sides, the two farmers win and lose together; the calls come in play
    order starting behind the winner (lord wins: down, up, lord; down wins: up, lord, down; up
    wins: lord, down, up).
Here that bookkeeping is done for T tables at once with tensor ops (any device).  Pinned by fixture
G11 (tests/golden/gen_game.py: every perceive() call of the reference's own Game.play).

One documented choice: the reference never clears `*_s0 / *_a0` between episodes
(game.py:39-40,132-137; SURVEY.md appendix A "quirks"), so from the second episode of a Game
object on, the first feedback of `down` and of `up` pushes (s0, a0 of the PREVIOUS episode's last
move, 0, s1 = first observation of the new episode, a1, False) -- a transition across a reshuffle;
the lord's stale pair is overwritten unseen.  Default here: pending slots are cleared at the
terminal ply (no such transition); replicate_reference_quirk=True reproduces the reference call
for call (both modes are checked against G11).

Usage per lock-step iteration (all tensors [T, ...]):
    closed = asm.before_step(role, face, chosen_onehot, greedy_onehot)
    ... env.step(auto_reset=False) ...; terminal_face = env.observe(variant)
    ended = asm.after_step(role, done, r, terminal_face); env.reset(mask=done)
Both calls return a dict of the transitions they closed (s0, a0, reward, s1, a1, done,
table, role) ready to append to a replay buffer; within a table the rows are in the reference's
call order.
"""
import torch

REWARD_DICT = {"up": 50.0, "lord": 100.0, "down": 50.0}  # game.py:13-14; role ids 0 up, 1 lord, 2 down


class TransitionAssembler:
    def __init__(self, n_tables, planes, device, reward_dict=None, trained_roles=(True, True, True),
                 replicate_reference_quirk=False):
        """trained_roles: (up, lord, down) -- the roles whose agent keeps training (Game's train_dict, game.py:15-16,
        :95-104,:112): only they open and close transitions.  replicate_reference_quirk: see the module docstring."""
        rd = dict(REWARD_DICT if reward_dict is None else reward_dict)
        self.T, self.P, self.device = int(n_tables), int(planes), torch.device(device)
        self.reward = torch.tensor([rd["up"], rd["lord"], rd["down"]], dtype=torch.float32, device=self.device)
        self.trained = torch.tensor([bool(x) for x in trained_roles], dtype=torch.bool, device=self.device)
        self.quirk = bool(replicate_reference_quirk)
        self.s0 = torch.zeros((self.T, 3, self.P, 15, 4), dtype=torch.float32, device=self.device)
        self.a0 = torch.zeros((self.T, 3, 15, 4), dtype=torch.float32, device=self.device)
        self.pending = torch.zeros((self.T, 3), dtype=torch.bool, device=self.device)
        self.fresh = torch.ones(self.T, dtype=torch.bool, device=self.device)   # no ply of the episode played yet

    @staticmethod
    def _pack(s0, a0, reward, s1, a1, done, table, role):
        return {"s0": s0, "a0": a0, "reward": reward, "s1": s1, "a1": a1, "done": done, "table": table,
                "role": role}

    def before_step(self, role, face, chosen, greedy, active=None):
        """role int[T] actor of each table, face f32[T,P,15,4] its observation, chosen / greedy
        f32[T,15,4] the action it is about to play and the greedy action (a1 of the closing
        transition, game.py:125).  Closes the actor's previous transition, opens a new one.
        active bool[T]: tables that move in this iteration (default all)."""
        role = role.to(self.device).long()
        ar = torch.arange(self.T, device=self.device)
        if active is None:
            active = torch.ones(self.T, dtype=torch.bool, device=self.device)
        active = active.to(self.device).bool()
        act_tr = active & self.trained[role]
        # the first ply of an episode (the lord's) has no feedback in front of it (game.py:129-130): whatever the slot
        # still holds is overwritten unseen
        close = self.pending[ar, role] & act_tr & ~self.fresh
        idx = close.nonzero(as_tuple=True)[0]
        r_idx = role[idx]
        out = self._pack(self.s0[idx, r_idx].clone(), self.a0[idx, r_idx].clone(),
                         torch.zeros(idx.numel(), dtype=torch.float32, device=self.device),
                         face[idx].clone(), greedy[idx].clone(),
                         torch.zeros(idx.numel(), dtype=torch.bool, device=self.device), idx, r_idx)
        act = act_tr.nonzero(as_tuple=True)[0]
        self.s0[act, role[act]] = face[act]
        self.a0[act, role[act]] = chosen[act]
        self.pending[act, role[act]] = True
        self.fresh &= ~active
        return out

    def after_step(self, role, done, r, terminal_face):
        """role int[T] the actor that just moved, done u8[T], r i8[T] (-1 lord won, +1 farmers
        won; rule_play.py:14), terminal_face f32[T,P,15,4] = env.observe() after the ply.
        Closes every pending transition of the finished tables."""
        done = done.to(self.device).bool()
        role = role.to(self.device).long()
        t_idx, r_idx = (self.pending & done[:, None]).nonzero(as_tuple=True)
        # the reference's call order: play order (lord, down, up) starting behind the winner = the actor of this ply
        order = torch.argsort(t_idx * 3 + (r_idx - role[t_idx] - 1) % 3)
        t_idx, r_idx = t_idx[order], r_idx[order]
        lord_won = (r.to(self.device)[t_idx] < 0)
        is_lord = r_idx == 1
        sign = torch.where(lord_won == is_lord, 1.0, -1.0)
        out = self._pack(self.s0[t_idx, r_idx].clone(), self.a0[t_idx, r_idx].clone(),
                         sign * self.reward[r_idx], terminal_face[t_idx].clone(),
                         torch.zeros((t_idx.numel(), 15, 4), dtype=torch.float32, device=self.device),
                         torch.ones(t_idx.numel(), dtype=torch.bool, device=self.device), t_idx, r_idx)
        if not self.quirk:
            self.pending[done] = False
        self.fresh |= done
        return out


class ReturnAssembler:
    """Return spec v1 (include/ddz_env.h: ddz_mc_before / ddz_mc_after) in plain torch ops on any device: the host
    statement the device recorder (ReturnRecorder, csrc/ddz_returns.h) is tested against.  A table keeps an episode log of at
    most log_cap decisions (state row u8 [176], action id, role, the role's decision ordinal), a decision counter per role and
    a cumulative `lost` counter; when the table finishes, log entry (role k, ordinal j) becomes the target
        ret = (+reward[k] if k's side won else -reward[k]) * gamma^togo,   togo = c[k] - 1 - j,
    by togo f32 multiplications (not pow: the device gives the same bits).  With gamma = 1 that is the Deep Monte Carlo target;
    with the reference's gamma it is what y_i = r_i + (1 - done_i) * gamma * y_{i+1} gives along the role's own transitions."""

    def __init__(self, n_tables, log_cap, device="cpu", reward_dict=None, trained_roles=(True, True, True), gamma=1.0):
        rd = dict(REWARD_DICT if reward_dict is None else reward_dict)
        self.T, self.L, self.device = int(n_tables), int(log_cap), torch.device(device)
        if not 1 <= self.L <= 255:
            raise ValueError("log_cap must be in 1 .. 255")
        dev = self.device
        self.reward = torch.tensor([float(rd.get(k) or 0.0) for k in ("up", "lord", "down")], dtype=torch.float32, device=dev)
        self.trained = torch.tensor([bool(x) for x in trained_roles], dtype=torch.bool, device=dev)
        self.gamma = torch.tensor(float(gamma), dtype=torch.float32, device=dev)
        self.rows = torch.zeros((self.T, self.L, 176), dtype=torch.uint8, device=dev)
        self.act = torch.zeros((self.T, self.L), dtype=torch.int32, device=dev)
        self.who = torch.zeros((self.T, self.L, 2), dtype=torch.int64, device=dev)     # {role, ordinal}
        self.n = torch.zeros(self.T, dtype=torch.int64, device=dev)
        self.c = torch.zeros((self.T, 3), dtype=torch.int64, device=dev)               # (u8 on the device: saturates at 255)
        self.lost = torch.zeros(self.T, dtype=torch.int64, device=dev)                 # (u32 on the device: saturates)

    def before(self, role, rows, chosen, active=None):
        """role int [T] the actor of each table (its state row's role byte), rows u8 [T,176] the state rows now, chosen int32 [T]
        the action ids about to be played, active bool [T] (None: all).  Appends to the logs; returns nothing."""
        dev = self.device
        role = role.to(dev).long()
        ok = role <= 2
        if active is not None:
            ok = ok & active.to(dev).bool()
        ok = ok & self.trained[role.clamp(max=2)]
        t = ok.nonzero(as_tuple=True)[0]
        k = role[t]
        room = self.n[t] < self.L
        tr, kr = t[room], k[room]
        p = self.n[tr]
        self.rows[tr, p] = rows.to(dev).view(self.T, 176)[tr]
        self.act[tr, p] = chosen.to(dev).to(torch.int32)[tr]
        self.who[tr, p, 0], self.who[tr, p, 1] = kr, self.c[tr, kr]
        self.n[tr] += 1
        self.lost[t[~room]] = (self.lost[t[~room]] + 1).clamp(max=2 ** 32 - 1)
        self.c[t, k] = (self.c[t, k] + 1).clamp(max=255)

    def after(self, done, r):
        """done u8 [T], r i8 [T] as the step wrote them (r < 0: the lord won).  Returns the emits of the call in emit order
        (ascending table, then ascending log position): {"s0" u8 [m,176], "a0" int32 [m], "ret" f32 [m], "table" int64 [m],
        "togo" int64 [m], "role" int64 [m]}; the logs and decision counters of the finished tables are empty afterwards."""
        dev = self.device
        done = done.to(dev).bool()
        live = torch.arange(self.L, device=dev)[None, :] < self.n[:, None]
        t, p = (live & done[:, None]).nonzero(as_tuple=True)
        k, j = self.who[t, p, 0], self.who[t, p, 1]
        togo = self.c[t, k] - 1 - j
        lord_won = r.to(dev)[t] < 0
        ret = torch.where(lord_won == (k == 1), self.reward[k], -self.reward[k])
        for i in range(int(togo.max()) if togo.numel() else 0):
            ret = torch.where(togo > i, ret * self.gamma, ret)
        out = {"s0": self.rows[t, p].clone(), "a0": self.act[t, p].clone(), "ret": ret, "table": t, "togo": togo, "role": k}
        self.n[done] = 0
        self.c[done] = 0
        return out


class TeacherAssembler:
    """Teacher spec v1 (include/ddz_env.h: ddz_teach) on the host, as plain Python loops over the tables and the
    moves of their lists: the statement the device pass (TeacherRecorder, csrc/ddz_teach.h) is tested against.  Move j of table
    t's list becomes the target
        ret = reward[k] * ((2 num - p) / p),   p = (den - unknown) * scale,   k = the table's role,
    where the table is selected and den - unknown >= min_den: +reward[k] for a move that always wins, -reward[k] for one that
    never does.  (2 num - p) and p are converted to f32 (round to nearest), divided in f32 and multiplied by the f32 reward."""

    def __init__(self, reward_dict=None, trained_roles=(True, True, True)):
        rd = dict(REWARD_DICT if reward_dict is None else reward_dict)
        self.reward = torch.tensor([float(rd.get(k) or 0.0) for k in ("up", "lord", "down")], dtype=torch.float32)
        self.trained = [bool(x) for x in trained_roles]
        if len(self.trained) != 3:
            raise ValueError("trained_roles: (up, lord, down)")

    def label(self, rows, counts, ids, num, den=None, den_const=None, unknown=None, scale=1, min_den=1, active=None):
        """rows u8 [T,176] the state rows, counts int [T], ids / num / den / unknown int [T, stride] (den None: den_const for
        every entry; unknown None: nothing subtracted), active bool [T] (None: all).  Returns the emits of the call in emit
        order (ascending table, then ascending j; a ring takes those of its role in this order): {"s0" u8 [m,176], "a0" int32
        [m], "ret" f32 [m], "table" int64 [m], "togo" int64 [m] (zeros), "role" int64 [m]}."""
        scale, min_den = int(scale), int(min_den)
        if not 1 <= scale <= 1024 or min_den < 1:
            raise ValueError("scale must be in [1, 1024] and min_den at least 1")
        if den is None and (den_const is None or int(den_const) < 1):
            raise ValueError("den_const must be at least 1 where no den array is given")
        rows = rows.cpu().view(-1, 176)
        T = rows.shape[0]
        counts = counts.cpu().view(T).tolist()
        table = lambda x: None if x is None else x.cpu().view(T, -1).tolist()   # noqa: E731
        ids, num, den, unknown = table(ids), table(num), table(den), table(unknown)
        stride = len(num[0])
        act = None if active is None else active.cpu().view(T).tolist()
        role_byte = rows[:, 10 * 16].tolist()
        ts, js, ks, top, bottom = [], [], [], [], []
        for t in range(T):
            k = role_byte[t]
            if k > 2 or (act is not None and not act[t]) or not self.trained[k] or counts[t] <= 0:
                continue
            for j in range(min(counts[t], stride)):
                d = (den[t][j] if den is not None else int(den_const)) - (unknown[t][j] if unknown is not None else 0)
                if d < min_den:
                    continue
                p = d * scale
                ts.append(t), js.append(j), ks.append(k), top.append(2 * num[t][j] - p), bottom.append(p)
        t, k = torch.tensor(ts, dtype=torch.int64), torch.tensor(ks, dtype=torch.int64)
        value = torch.tensor(top, dtype=torch.int64).to(torch.float32) / torch.tensor(bottom, dtype=torch.int64).to(torch.float32)
        return {"s0": rows[t].clone(), "a0": torch.tensor([ids[a][b] for a, b in zip(ts, js)], dtype=torch.int32),
                "ret": self.reward[k] * value, "table": t, "togo": torch.zeros_like(t), "role": k}


def td_target(transitions, q_next, gamma=0.95):
    """y = r + (1 - done) * gamma * Q_target(s1, a1)  (dqn.py:40-41, config.py:8 GAMMA)."""
    return transitions["reward"] + (~transitions["done"]).float() * gamma * q_next.view(-1)


# ------------------------------------------------------------------------------------------------
# The ragged Q forward of the reference's DQN (net.py:81-102, dqn.py:50-71, game.py:95-104) for T tables at once.
#
# The reference evaluates Q(face, action) for EVERY legal action of a state by repeating `face` A times and
# concatenating the action as one more input plane (net.py:87-90): sum_A rows x (C x 15 x 4) inputs per iteration.
# Here the first layer is evaluated factorised.  Its five convolutions are linear in their input and look at ONE
# rank (conv1..4: a (1,k) window, stride 4, on a width-4 input -> one column per rank, net.py:141-144) or ONE
# thermometer slot (conv_shunzi (15,1), net.py:146), and an action plane is a thermometer of its count vector
# (envi.py:139-146), so for a rank r that an action takes `cnt` cards of:
#     maxpool_k conv_k(face + action)[c, r] = max_k ( S_k[t, r, c] + A_k[cnt, c] )          =: Y[t, r, cnt, c]
# with S = the face part (one GEMM per table, NOT per legal row) and A a 5 x 4 x 256 table of the action-plane
# weights -- the same for every rank, and cnt = 0 for every rank the action does not touch.  fc1 is linear, so its
# pre-activation is a sum over the 15 ranks of U[r, t, cnt_r, :] = fc1_r @ Y[t, r, cnt_r, :] (+ the conv_shunzi
# branch, linear end to end, folded in: a per-table vector and a per-(rank, count) vector).  Per iteration:
#     tables(face)  -> U [15, 5, T, 256]   dense, fixed shapes, plain torch GEMMs (hipBLASLt) -- no ragged dimension
#     per legal row -> q = fc2(relu(sum_r U[r, cnt_r, t] + Z[r, cnt_r]))   a gather-sum + a 256-dot per row
# The loop evaluates the same sum over the NEEDED rows only (FactorisedQ.needed -> ddz_q_slab_needed, over the slab lists:
# no CSR, no host sync, no padded rows); q_csr is the sum over CSR rows with plain torch ops (the training path, ragged_q).
import contextlib  # noqa: E402

import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

_CONV_CH = 256
_FC_TILE = None
# face planes -> face variant of the shared-rows form (FACE_PLANES' values are distinct): EnvCooperationSimplify (direct-addressed
# row finder), EnvComplicated and EnvCooperation (hashed row finder)
SHARED_VARIANT = {6: 3, 7: 1, 9: 2}


def fc_tile():
    """rows per tile of the engine's fc1 kernel (ddz_q_fc1_tile_rows, csrc/ddz_qnet.h FC_M): the rank segments of the needed
    rows start at multiples of it"""
    global _FC_TILE
    if _FC_TILE is None:
        from . import _lib
        _FC_TILE = int(_lib.lib().ddz_q_fc1_tile_rows())
    return _FC_TILE


def row_capacities(T, variant, tile=None):
    """(cap, scap) for T tables, per network slot: the capacity of the needed rows D (a move takes at most what the actor holds:
    <= 20 T rows) and of the shared rows (<= 15 T distinct (rank, column) pairs, and the 4,134,375 direct-addressed keys of face
    variant 3), each with the padding of fifteen tile-aligned rank segments and rounded to the tile: neither can overflow."""
    tile = fc_tile() if tile is None else tile
    padded = lambda rows: (rows + 15 * tile + tile - 1) // tile * tile   # noqa: E731
    return padded(20 * T), padded(min(15 * T, 4134375) if variant == 3 else 15 * T)


def _run_stage(name, fn):
    fn()


def _beside(w, fork, two):
    """The fork of the Q forward's side stream: a context whose launches go to w["side"], behind all the current stream holds so
    far (event w[fork]: recorded on the current stream, the side stream waits) and beside what it issues next; _join ends it.
    By events: no host synchronisation, capturable in a hipGraph.  two=False: no context at all -- everything on the current
    stream."""
    if not two:
        return contextlib.nullcontext()
    side = w["side"]
    w[fork].record(torch.cuda.current_stream(side.device))
    side.wait_event(w[fork])
    return torch.cuda.stream(side)


def _join(w, two):
    """the current stream waits for what _beside put on the side stream"""
    if two:
        w["join"].record(w["side"])
        torch.cuda.current_stream(w["side"].device).wait_event(w["join"])


def first_layer_torch(net, face, actions):
    """The first layer of QNet.forward -- cat, conv1..conv4, cat, max-pool -- as the expressions of ddz_q_first_fwd /
    ddz_q_first_bwd (include/ddz_env.h) in plain differentiable torch ops, any device: with x = the planes of face [n,P,15,4]
    followed by actions [n,15,4],
        s_k = b_k[o] + sum_{c, j < k} w_k[o][c][0][j] * x[n][c][r][j],   y[n][o * 15 + r] = max_k s_k   -> f32 [n,3840]
    torch.max(dim) returns the FIRST index of a tie and routes the whole gradient there: max_pool2d's rule.  The statement the
    two kernels are tested against; QNet.forward_fused on CPU tensors."""
    n = actions.shape[0]
    x = torch.cat((face, actions.unsqueeze(1)), dim=1).permute(0, 2, 1, 3)                  # [n,15,C,4]
    s = []
    for k, cv in enumerate((net.conv1, net.conv2, net.conv3, net.conv4), start=1):
        w = cv.weight[:, :, 0, :]                                                         # [256,C,k]
        s.append(x[..., :k].reshape(n * 15, -1) @ w.reshape(_CONV_CH, -1).t() + cv.bias)  # [n * 15, 256]
    y = torch.stack(s, dim=-1).max(dim=-1).values                                         # the (1,4) pool: lowest k on a tie
    return y.view(n, 15, _CONV_CH).permute(0, 2, 1).reshape(n, _CONV_CH * 15)


class FirstLayer(torch.autograd.Function):
    """first_layer_torch on the device by the engine's two kernels (csrc/ddz_qtrain.h): FirstLayer.apply(face, actions, w1, b1,
    w2, b2, w3, b3, w4, b4) -> y f32 [n,3840].  The forward keeps the arg-max (one byte per value) for the backward, which
    writes the eight parameter gradients -- deterministic, no atomics -- and hands autograd the ones it asked for.  face and
    actions are data: one that requires grad is a ValueError.  With no parameter that requires grad no arg-max is written
    (QNet.forward_fused makes the no-grad pass -- the target network's -- the same way, by engine.q_first_fwd itself)."""

    @staticmethod
    def forward(ctx, face, actions, *params):
        from . import engine as E
        if face.requires_grad or actions.requires_grad:
            raise ValueError("FirstLayer has no gradient with respect to face or actions")
        if len(params) != 8:
            raise ValueError("FirstLayer.apply(face, actions, w1, b1, w2, b2, w3, b3, w4, b4)")
        weights, biases = [p.detach() for p in params[0::2]], [p.detach() for p in params[1::2]]
        want = any(ctx.needs_input_grad[2:])
        y, arg = E.q_first_fwd(face, actions, weights, biases, want_arg=want)
        if want:
            ctx.save_for_backward(face, actions, arg, *weights)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from . import engine as E
        face, actions, arg, *weights = ctx.saved_tensors
        gw, gb = E.q_first_bwd(face, actions, gy.contiguous(), arg, weights)
        grads = [None, None]
        for k in range(4):
            grads += [gw[k], gb[k]]
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad))


def stage_torch(net, face, actions):
    """Everything of QNet.forward in front of dropout / fc1 as the expressions of ddz_q_stage_fwd / ddz_q_stage_bwd
    (include/ddz_env.h) in plain differentiable torch ops, any device: first_layer_torch, then conv_shunzi as one matmul over
    the (plane, rank) pairs of every thermometer slot,
        z[n][o * 4 + j] = bs[o] + sum_{c, r} ws[o][c][r][0] * x[n][c][r][j],
    then net.py:97's cat -> h f32 [n,4864].  The statement the stage's kernels are tested against; QNet.forward_stage on CPU
    tensors."""
    n = actions.shape[0]
    y = first_layer_torch(net, face, actions)
    x = torch.cat((face, actions.unsqueeze(1)), dim=1)                                        # [n,C,15,4]
    w = net.conv_shunzi.weight[:, :, :, 0].reshape(_CONV_CH, -1)                              # [256, C * 15]
    z = x.reshape(n, -1, 4).permute(0, 2, 1).reshape(n * 4, -1) @ w.t() + net.conv_shunzi.bias   # [n * 4, 256]
    return torch.cat((y, z.view(n, 4, _CONV_CH).permute(0, 2, 1).reshape(n, _CONV_CH * 4)), dim=1)


class Stage(torch.autograd.Function):
    """stage_torch on the device by the engine's kernels (csrc/ddz_qtrain.h): Stage.apply(source, w1, b1, w2, b2, w3, b3, w4, b4,
    ws, bs) -> h f32 [n,4864], `source` the keyword operands of engine.q_stage_source -- {"face", "actions"} or {"states", "ids",
    "index", "table", "variant"} (packed replay rows: no face is built).  FirstLayer's rules: the forward keeps the arg-max for
    the backward, which writes the ten parameter gradients -- deterministic, no atomics -- and hands autograd the ones it asked
    for; the source is data (a tensor of it that requires grad is a ValueError); with no parameter that requires grad no arg-max
    is written and nothing is saved."""

    @staticmethod
    def forward(ctx, source, *params):
        from . import engine as E
        if any(torch.is_tensor(v) and v.requires_grad for v in source.values()):
            raise ValueError("Stage has no gradient with respect to its source")
        if len(params) != 10:
            raise ValueError("Stage.apply(source, w1, b1, w2, b2, w3, b3, w4, b4, ws, bs)")
        weights, biases = [p.detach() for p in params[0::2]], [p.detach() for p in params[1::2]]
        want = any(ctx.needs_input_grad[1:])
        h, arg = E.q_stage_fwd(weights, biases, want_arg=want, **source)
        if want:
            ctx.keys = [k for k, v in source.items() if torch.is_tensor(v)]
            ctx.rest = {k: v for k, v in source.items() if not torch.is_tensor(v)}
            ctx.save_for_backward(arg, *weights, *[source[k] for k in ctx.keys])
        return h

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gh):
        from . import engine as E
        arg, *rest = ctx.saved_tensors
        weights, data = rest[:5], rest[5:]
        gw, gb = E.q_stage_bwd(gh.contiguous(), arg, weights, **dict(zip(ctx.keys, data)), **ctx.rest)
        grads = [None]
        for k in range(5):
            grads += [gw[k], gb[k]]
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad))


class PackedBatch:
    """A replay batch that stays packed (TransitionRecorder.sample_packed): a role's ring views s0 / s1 u8 [capacity,176],
    a0 / a1 int32 [capacity], reward f32 [capacity], done u8 [capacity], the drawn entries index int64 [n] (inside the ring), the
    action table int8 [n_actions,16] and the face variant.  QNet.forward_packed reads the state rows and action ids directly;
    td_step gathers reward and done, nothing else."""
    __slots__ = ("s0", "s1", "a0", "a1", "reward", "done", "index", "table", "variant")

    def __init__(self, s0, s1, a0, a1, reward, done, index, table, variant):
        from .engine import FACE_PLANES
        if int(variant) not in range(len(FACE_PLANES)):
            raise ValueError("variant must be a face variant 0..3")
        self.s0, self.s1, self.a0, self.a1, self.reward, self.done = s0, s1, a0, a1, reward, done
        self.index, self.table, self.variant = index, table, int(variant)

    @property
    def n(self):
        return int(self.index.numel())


class ReturnBatch(PackedBatch):
    """A batch of return targets that stays packed (ReturnRecorder.sample_packed): side 0 of a PackedBatch -- the ring views s0
    u8 [capacity,176] and a0 int32 [capacity], the drawn entries, the action table, the variant -- with ret f32 [capacity] and
    togo u8 [capacity] in place of a second side: s1, a1, reward and done are None, and QNet.forward_packed(batch, 1) is a
    ValueError."""
    __slots__ = ("ret", "togo")

    def __init__(self, s0, a0, ret, togo, index, table, variant):
        super().__init__(s0, None, a0, None, None, None, index, table, variant)
        self.ret, self.togo = ret, togo


class QNet(nn.Module):
    """The reference's Q-network family (net.py:66-150: NetComplicated 5 input planes, NetMoreComplicated 8,
    NetCooperation 10, NetCooperationSimplify 7), same parameter names and shapes (state_dict-compatible); forward is
    the literal evaluation of net.py:81-102.  `planes` = planes of `face` (4 / 7 / 9 / 6); + 1 for the action."""

    def __init__(self, planes=6):
        super().__init__()
        c = int(planes) + 1
        self.planes = int(planes)
        self.conv1 = nn.Conv2d(c, _CONV_CH, (1, 1), (1, 4))
        self.conv2 = nn.Conv2d(c, _CONV_CH, (1, 2), (1, 4))
        self.conv3 = nn.Conv2d(c, _CONV_CH, (1, 3), (1, 4))
        self.conv4 = nn.Conv2d(c, _CONV_CH, (1, 4), (1, 4))
        self.conv_shunzi = nn.Conv2d(c, _CONV_CH, (15, 1), 1)
        self.pool = nn.MaxPool2d((1, 4))
        self.drop = nn.Dropout(0.5)
        self.fc1 = nn.Linear(_CONV_CH * (15 + 4), 256)
        self.fc2 = nn.Linear(256, 1)

    def forward(self, face, actions):
        """face [P,15,4] or [n,P,15,4], actions [n,15,4] -> Q [n,1]  (net.py:81-102)"""
        if face.dim() == 3:
            face = face.unsqueeze(0).repeat((actions.shape[0], 1, 1, 1))
        x = torch.cat((face, actions.unsqueeze(1)), dim=1)
        y = torch.cat([f(x) for f in (self.conv1, self.conv2, self.conv3, self.conv4)], -1)
        y = self.pool(y).view(actions.shape[0], -1)
        z = self.conv_shunzi(x).view(actions.shape[0], -1)
        h = self.drop(torch.cat([y, z], -1))
        return self.fc2(F.relu(self.fc1(h)))

    def forward_fused(self, face, actions):
        """forward with the cat / conv1..4 / cat / pool chain as ONE stage that never materialises the [n,256,15,4] pre-pool tensor
        -- FirstLayer (the engine's kernels) on device tensors, first_layer_torch on CPU tensors; conv_shunzi, dropout, fc1, relu
        and fc2 are the same modules in the same order (one RNG state gives the literal's dropout mask).  No gradient of face /
        actions."""
        if face.dim() == 3:
            face = face.unsqueeze(0).repeat((actions.shape[0], 1, 1, 1))
        params = [p for cv in (self.conv1, self.conv2, self.conv3, self.conv4) for p in (cv.weight, cv.bias)]
        if face.is_cuda and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            y = FirstLayer.apply(face.contiguous(), actions.contiguous(), *params)
        elif face.is_cuda:                                   # a no-grad pass: no arg-max is written, nothing is kept
            from .engine import q_first_fwd
            y = q_first_fwd(face.contiguous(), actions.contiguous(), [p.detach() for p in params[0::2]],
                            [p.detach() for p in params[1::2]], want_arg=False)[0]
        else:
            y = first_layer_torch(self, face, actions)
        z = self.conv_shunzi(torch.cat((face, actions.unsqueeze(1)), dim=1)).view(actions.shape[0], -1)
        h = self.drop(torch.cat([y, z], -1))
        return self.fc2(F.relu(self.fc1(h)))


    def _conv_params(self):
        return [p for cv in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv_shunzi) for p in (cv.weight, cv.bias)]

    def _stage(self, **source):
        """h [n,4864] by the engine's stage kernels: through Stage when a convolution parameter wants a gradient, else the no-grad
        pass (no arg-max is written, nothing is kept)"""
        params = self._conv_params()
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return Stage.apply(source, *params)
        from .engine import q_stage_fwd
        return q_stage_fwd([p.detach() for p in params[0::2]], [p.detach() for p in params[1::2]], want_arg=False, **source)[0]

    def forward_stage(self, face, actions):
        """forward with everything in front of dropout -- cat, conv1..4, cat, pool, conv_shunzi, the views, the cat -- as ONE stage
        that writes h [n,4864] whole: Stage (the engine's kernels: two launches, no library convolution) on device tensors,
        stage_torch on CPU tensors; dropout, fc1, relu and fc2 are the same modules in the same order (one RNG state gives the
        literal's dropout mask).  No gradient of face / actions."""
        if face.dim() == 3:
            face = face.unsqueeze(0).repeat((actions.shape[0], 1, 1, 1))
        h = self._stage(face=face.contiguous(), actions=actions.contiguous()) if face.is_cuda else stage_torch(self, face, actions)
        return self.fc2(F.relu(self.fc1(self.drop(h))))

    def forward_packed(self, batch, side):
        """forward_stage on side 0 (s0, a0) or 1 (s1, a1) of a PackedBatch, the stage reading the ring's state rows and action
        ids itself: no face, no thermometer and no library convolution.  Bit for bit forward_stage on what
        TransitionRecorder.decode gives for the same index."""
        from .engine import FACE_PLANES
        if side not in (0, 1):
            raise ValueError("side: 0 = (s0, a0), 1 = (s1, a1)")
        if not isinstance(batch, PackedBatch):
            raise ValueError("forward_packed takes a PackedBatch (TransitionRecorder.sample_packed)")
        if FACE_PLANES[batch.variant] != self.planes:
            raise ValueError(f"the network takes {self.planes} planes, face variant {batch.variant} has {FACE_PLANES[batch.variant]}")
        states, ids = (batch.s0, batch.a0) if side == 0 else (batch.s1, batch.a1)
        if states is None:
            raise ValueError("a batch of return targets (ReturnBatch) has no side 1")
        h = self._stage(states=states, ids=ids, index=batch.index, table=batch.table, variant=batch.variant)
        return self.fc2(F.relu(self.fc1(self.drop(h))))


class FactorisedQ:
    """Inference form of a QNet: the weight-only tables of the factorisation above, cached until the weights change
    (refresh() is called automatically, by every eager call, when a parameter's version counter moved).  Eval semantics (no
    dropout).
    Fixed storage: every derived table (TABLES) is allocated once per object and device and WRITTEN IN PLACE by every later
    refresh(); the workspaces of _ws are allocated once per (device, T) and survive a refresh.  A hipGraph that captured an
    acting pass therefore reads, at every replay, the tables of the last refresh() -- the weights of that moment, defined
    values in live memory -- and after a learner step the caller runs refresh() eagerly (no Python runs at replay) and replays.
    A network moved to another device gets new tables there: not under a live graph.
    What refresh() cannot see: _versions() compares (id, address, version counter) per parameter, which an optimizer step, any
    in-place write under no_grad, load_state_dict (assign=True too) and a swapped Parameter all move; a write through `.data`
    (p.data.mul_()) moves none of them and is unsupported unless followed by refresh(force=True)."""
    # the derived tables: what a captured pass holds addresses of (Wd is a view of W2; W2_jok a list of two)
    TABLES = ("Wf", "bias_f", "A", "Mz_f", "Z", "base", "W2", "W2x", "W2_main", "w2", "b2")

    def __init__(self, net, chunk_tables=16384):
        self.net, self.chunk = net, int(chunk_tables)
        self.two_streams = True        # needed(shared="all"): the D chain on a side stream beside the H0 chain
        self.P = net.planes
        self.H, self.H1 = _CONV_CH, net.fc1.out_features
        self._ver = None
        self._dev = None
        self._ws = {}
        self.refresh()

    def _versions(self):
        # (id and storage address too: load_state_dict(assign=True) / a swapped Parameter can carry an equal version; a write
        # through p.data moves nothing here: refresh(force=True) is the caller's part then)
        return tuple((id(p), p.data_ptr(), p._version) for p in self.net.parameters()) + (next(self.net.parameters()).device,)

    def _allocate(self, dev):
        """the derived tables' storage on dev, made once: refresh() writes into it"""
        P, H, H1 = self.P, self.H, self.H1
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)   # noqa: E731
        self.Wf, self.bias_f, self.A = z(P * 4, 4 * H), z(4 * H), z(5, 4, H)
        self.Mz_f, self.Z, self.base = z(P * 60, H1), z(15, 5, H1), z(H1)
        self.W2, self.W2x = z(15, H, H1), z(15, H + (4 * P + 15) // 16 * 16, H1)
        self.Wd = self.W2.view(15 * H, H1)                             # the dense GEMM's right operand: K = 15 * 256, rank-major
        self.W2_main, self.W2_jok = z(65, H, H1), [z(2, H, H1), z(2, H, H1)]
        self.w2, self.b2 = z(H), z(1)
        self._dev = dev

    @torch.no_grad()
    def refresh(self, force=False):
        """Recompute the derived tables from the current weights, into their fixed storage, when a parameter moved (_versions)
        or when forced; returns whether it did.  Raises RuntimeError while the current stream is capturing: a refresh is no
        part of an iteration, and one must not be baked into a graph unnoticed (_Loop.capture refreshes before it begins)."""
        now = self._versions()
        if not force and now == self._ver:
            return False
        n, P, H, H1 = self.net, self.P, self.H, self.H1
        dev = n.fc1.weight.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the network's weights moved (or refresh(force=True)) while the stream is capturing: call "
                               "refresh() before the capture begins")
        if dev != self._dev:
            self._allocate(dev)
        C = P + 1
        convs = (n.conv1, n.conv2, n.conv3, n.conv4)
        Wf = self.Wf.view(P, 4, 4, H)                                  # [plane, slot j, conv k, channel] (slots j > k stay 0)
        A = self.A                                                     # [count, conv k, channel] (count 0 stays 0)
        for k, cv in enumerate(convs):
            w = cv.weight[:, :, 0, :]                                  # [H, C, k+1]
            Wf[:, : k + 1, k, :] = w[:, :P, :].permute(1, 2, 0)
            for cnt in range(1, 5):
                A[cnt, k] = w[:, C - 1, : min(k + 1, cnt)].sum(dim=1)
        torch.cat([cv.bias for cv in convs], out=self.bias_f)
        W1 = n.fc1.weight
        W1y = W1[:, : 15 * H].reshape(H1, H, 15)                       # input index c * 15 + r (net.py:94 view)
        W1z = W1[:, 15 * H:].reshape(H1, H, 4)                         # input index c * 4 + w  (net.py:96)
        Ws = n.conv_shunzi.weight[:, :, :, 0]                          # [H, C, 15]
        Mz = torch.einsum("ocw,cpr->prwo", W1z, Ws)                    # [C, 15, 4, H1]: conv_shunzi then fc1, composed
        self.Mz_f.copy_(Mz[:P].reshape(P * 60, H1))                    # face part: one GEMM per table
        self.Z[:, 1:] = Mz[C - 1].cumsum(dim=1)                        # action part per (rank, count): weights only
        self.base.copy_(n.fc1.bias + torch.einsum("ocw,c->o", W1z, n.conv_shunzi.bias))
        W2 = self.W2.copy_(W1y.permute(2, 1, 0))                       # [r, c, o]: fc1 per rank
        # fc1 per rank with the table term's rows appended (the shared-rows form, csrc/ddz_qnet.h section 5): a shared row
        # carries its 4 P column values behind its 256 first-layer values, so [fc1_r ; Mz[:, r] ; 0] (K = 256 + ceil16(4 P):
        # 288 for P = 6 / 7, 304 for P = 9) gives Y x fc1_r + column x Mz_r in one product (the padding rows stay 0)
        self.W2x[:, :H] = W2
        self.W2x[:, H: H + 4 * P] = Mz[:P].permute(1, 0, 2, 3).reshape(15, P * 4, H1)
        # one GEMM batch per (rank, count): ranks 3..2 have counts 0..4 (65 batches), the two jokers counts 0..1
        self.W2_main.view(13, 5, H, H1).copy_(W2[:13, None].expand(13, 5, H, H1))
        for k, r in enumerate((13, 14)):
            self.W2_jok[k].copy_(W2[r, None].expand(2, H, H1))
        self.w2.copy_(n.fc2.weight[0])
        self.b2.copy_(n.fc2.bias)
        self._ver = now
        return True

    def _workspace(self, Tc, dev, fused):
        key = (Tc, dev, fused)
        if key not in self._ws:
            if len(self._ws) > 3:
                self._ws.clear()
            Y = torch.zeros((15, 5, Tc, self.H), dtype=torch.float32, device=dev)
            S = tmp = None
            if not fused:
                S = torch.empty((15 * Tc, 4, self.H), dtype=torch.float32, device=dev)
                tmp = torch.empty((15 * Tc, 4, self.H), dtype=torch.float32, device=dev)
            self._ws[key] = (Y, S, tmp)
        return self._ws[key]

    @torch.no_grad()
    def tables(self, face, out=None, fused=None):
        """face f32 [T,P,15,4] -> U f32 [15,5,T,H1]: fc1's pre-activation contribution of rank r when the action takes
        cnt cards of it (the per-table terms -- fc1 bias, the face part of conv_shunzi -- ride on rank 0; counts 2..4 of
        the two joker ranks are never written: pass a zero-initialised `out`).  Fixed shapes, no host sync; tables are
        processed in chunks to bound the workspace.
        fused (default: on a GPU): Y = max-pooled first layer per (rank, count, table) comes from the engine's
        ddz_q_features in one pass over `face`; fused=False is the same stage in plain torch ops (the statement the
        kernel is tested against; it reads and writes the [T,15,4,256] conv output ten times)."""
        if self._ver != self._versions():
            self.refresh()
        T, P, H, H1 = face.shape[0], self.P, self.H, self.H1
        if tuple(face.shape[1:]) != (P, 15, 4):
            raise ValueError(f"face must be [T,{P},15,4]")
        if fused is None:
            fused = face.is_cuda
        U = out if out is not None else torch.zeros((15, 5, T, H1), dtype=torch.float32, device=face.device)
        if tuple(U.shape) != (15, 5, T, H1) or not U.is_contiguous():
            raise ValueError("out must be a contiguous [15,5,T,256] tensor")
        U75 = U.view(75, T, H1)
        for t0 in range(0, T, self.chunk):
            t1 = min(T, t0 + self.chunk)
            Tc = t1 - t0
            f = face[t0:t1]
            Y, S, tmp = self._workspace(Tc, face.device, fused)
            if fused:
                from .engine import q_features
                q_features(f.contiguous(), self.Wf, self.bias_f, self.A, Y)
            else:
                X = f.permute(2, 0, 1, 3).reshape(15 * Tc, P * 4)      # rank-major rows: (r, t) x (plane, slot)
                torch.addmm(self.bias_f, X, self.Wf, out=S.view(15 * Tc, 4 * H))
                for cnt in range(5):
                    torch.add(S, self.A[cnt], out=tmp)
                    Y[:, cnt] = tmp.amax(dim=1).view(15, Tc, H)        # max over the four convs = the (1,4) max-pool
            Y75 = Y.view(75, Tc, H)
            torch.bmm(Y75[:65], self.W2_main, out=U75[:65, t0:t1])     # ranks 3..2, counts 0..4
            for k, r in enumerate((13, 14)):                           # the jokers: counts 0, 1
                torch.bmm(Y75[5 * r: 5 * r + 2], self.W2_jok[k], out=U75[5 * r: 5 * r + 2, t0:t1])
            U[0, :, t0:t1] += torch.addmm(self.base, f.reshape(Tc, P * 60), self.Mz_f)
        return U

    def _needed_workspace(self, dev, T, shared):
        """needed()'s buffers for T tables, the tiers the form takes all made before its first launch: the needed rows (every form),
        the shared rows (shared), the shared D rows with the side stream and its events ("all"), y0 (the dense form only: 1 GB at
        65,536 tables)."""
        from . import engine as E
        P, H, H1 = self.P, self.H, self.H1
        w = self._ws.setdefault(("needed", dev, T), {})
        cap, scap = row_capacities(T, SHARED_VARIANT.get(P))
        z = lambda *shape, dt=torch.float32, fill=0: torch.full(shape, fill, dtype=dt, device=dev)   # noqa: E731
        if "cap" not in w:
            w.update({"cap": cap, "y0": None, "dy": z(cap, H), "d": z(cap, H1), "h0": z(T, H1),
                      "row_index": z(T, 64, dt=torch.int32, fill=-1), "seg": z(40, dt=torch.int32), "row_cnt": z(cap, dt=torch.uint8),
                      "scratch": z(E.q_need_scratch_bytes(T), dt=torch.uint8)})
        if shared and "srows" not in w:
            v = SHARED_VARIANT[P]
            sws = E.q_shared_ws_bytes() if v == 3 else E.q_shared_hash_ws_bytes(T)
            w.update({"svariant": v, "scap": scap, "sws": z(sws, dt=torch.uint8), "srows": z(T, 16, dt=torch.int32, fill=-1),
                      "srep": z(scap, dt=torch.int32, fill=-1), "sseg": z(40, dt=torch.int32),
                      "ys": z(scap, E.shared_row_width(P)), "g": z(scap, H1),
                      "y0": None})                                           # (a dense call's y0 is not needed in this form)
        if shared == "all" and "dws" not in w:
            w.update({"dws": z(E.q_shared_need_ws_bytes(w["scap"]), dt=torch.uint8), "row_index2": z(T, 64, dt=torch.int32, fill=-1),
                      "drep": z(w["cap"], dt=torch.int32, fill=-1), "dseg": z(40, dt=torch.int32), "drow_cnt": z(w["cap"], dt=torch.uint8),
                      "side": torch.cuda.Stream(dev), "fork0": torch.cuda.Event(), "fork": torch.cuda.Event(),
                      "join": torch.cuda.Event()})
        if not shared and w["y0"] is None:
            w["y0"] = z(T, 15 * H)
        return w

    # ---- needed form: H0 per table from ONE dense GEMM + D only for the (rank, count) rows some legal move uses ----
    @torch.no_grad()
    def needed(self, env, face, gemm="torch", shared=False, hook=None):
        """face f32 [T,P,15,4] of env's CURRENT states (its slab lists are read on the device) -> NeededU: h0 f32 [T,256],
        d f32 [rows,256], row_index int32 [T,64], seg int32 [40] (device).  Nothing crosses to the host; every launch is
        graph-capturable.  The rows GEMM (D = dY x fc1[rank], segment sizes in device memory) is always the engine's fp32
        MFMA kernel (ddz_q_fc1_rows: a library GEMM would need the sizes on the host).  The dense GEMM (a plain
        [T, 3840] x [3840, 256] product) is torch.addmm = hipBLASLt by default (gemm="torch": 148 TFLOP/s in the loop), or
        the same MFMA kernel (gemm="mfma", ddz_q_fc1_dense: 125 TFLOP/s; six geometries measured, tools/fc1_probe.py).
        shared=True / "all" (faces of EnvCooperationSimplify, P = 6; EnvCooperation, P = 9; EnvComplicated, P = 7 -- the face
        variant follows from P -- and `face` MUST be env's own face of that variant of its current states: the rows are keyed
        from env's state, not from `face`): the SHARED-ROWS form (csrc/ddz_qnet.h sections 5-6) -- no dense GEMM: one row per
        distinct (rank, face column) of the batch (3.6 % of the 15 T columns at 65,536 tables for P = 6; the rows are found by
        direct addressing for P = 6, by a hashed table for P = 7 / 9, section 5b), first layer + ONE k_fc1 rows product over
        those (K = 256 + ceil16(4 P): the table term rides in it), H0[t] = base + the fifteen rows of table t.
        True: the needed rows D stay per table (their first layer skips the ranks no legal move touches); "all" (PolicyLoop's
        default): D as well once per distinct (shared row, count) -- the returned row_index is then the remapped one -- and the
        D chain runs on a side stream beside the H0 chain (self.two_streams; fork / join by events, no host synchronisation).
        Exact per call from the current weights and states (nothing is cached between calls); same values up to fp32 summation
        order in H0 (tests: 1e-5; D and q bit for bit between True and "all").
        hook(name, fn): every stage is issued as hook(stage name, the callable that launches it) -- PolicyLoop.profile's timer; the
        call then keeps every stage on the current stream (events around work of another stream time nothing), same values.
        The result aliases this object's workspace: consume it before the next call."""
        from . import engine as E
        if self._ver != self._versions():
            self.refresh()
        T, P = face.shape[0], self.P
        if shared and P not in SHARED_VARIANT:
            raise ValueError("shared=True keys the columns of the faces of EnvComplicated, EnvCooperation and EnvCooperationSimplify "
                             "(face variants 1 / 2 / 3: 7 / 9 / 6 planes) only")
        if tuple(face.shape[1:]) != (P, 15, 4) or T != env.T or not face.is_cuda:
            raise ValueError(f"face must be a device tensor [T,{P},15,4] of the environment's tables")
        if not shared and gemm not in ("mfma", "torch"):
            raise ValueError("gemm must be 'mfma' or 'torch'")
        w = self._needed_workspace(face.device, T, shared)
        run = hook or _run_stage
        all_ = shared == "all"
        two = all_ and self.two_streams and hook is None
        Wf, bf, A = self.Wf, self.bias_f, self.A
        # the needed rows: per table, or ("all") one D row per distinct (shared row, count) (section 6) -- row_index remapped
        ri, sg, rc = (w["row_index2"], w["dseg"], w["drow_cnt"]) if all_ else (w["row_index"], w["seg"], w["row_cnt"])
        with _beside(w, "fork0", two):                                   # the need sets beside the shared rows
            run("need", lambda: env.q_need(w["cap"], w["scratch"], w["row_index"], w["seg"], w["row_cnt"]))
        if shared:
            run("shared_rows", lambda: env.q_shared_rows(w["sws"], w["scap"], w["srows"], w["srep"], w["sseg"], variant=w["svariant"]))
        else:
            run("features", lambda: E.q_features_needed(face, Wf, bf, A, ri, w["y0"], w["dy"]))
            run("table_term", lambda: torch.addmm(self.base, face.view(T, P * 60), self.Mz_f, out=w["h0"]))   # (K = 60 P: small)
            run("fc1_dense", (lambda: E.q_fc1_dense(w["y0"], self.Wd, w["h0"])) if gemm == "mfma" else
                (lambda: w["h0"].addmm_(w["y0"], self.Wd)))
        # The H0 chain (first layer of the rows -> G -> gather) and the D chain (D rows -> dY -> D) share only their inputs: both
        # GEMMs are a few hundred tiles -- one or two rounds over the 256 CUs, the launch as long as its last round -- and the
        # bookkeeping kernels are latency-bound, so the D chain runs on a SIDE STREAM beside the H0 chain.
        with _beside(w, "fork", two):
            if all_:
                run("shared_need", lambda: env.q_shared_need(w["row_index"], w["srows"], w["sseg"], w["scap"], w["dws"], w["cap"], ri,
                                                             w["drep"], sg, rc))
                run("features", lambda: E.q_features_drows(face, Wf, bf, A, w["srep"], w["drep"], sg, w["dy"]))
            elif shared:
                run("features", lambda: E.q_features_needed(face, Wf, bf, A, ri, None, w["dy"]))
            run("fc1_rows", lambda: E.q_fc1_rows(w["dy"], sg, rc, self.W2, self.Z, w["d"]))   # D = dY x fc1[rank] + Z[rank][count]
        if shared:
            # G[row] = Y[row] x fc1[rank] + column x Mz[rank] (the table term is linear in the face: folded into the rows -- the
            # column rides behind Y in the row, Mz[rank] behind fc1[rank] in the operand: one K = 288 / 304 product)
            run("features_shared", lambda: E.q_features_rows(face, Wf, bf, w["srep"], w["sseg"], w["ys"]))
            run("fc1_shared", lambda: E.q_fc1_rows_k(w["ys"], w["sseg"], self.W2x, w["g"]))
            run("gather_h0", lambda: E.q_gather_h0(w["g"], w["srows"], w["h0"], base=self.base))   # H0[t] = base + sum_r G[row(t, r)]
        _join(w, two)
        return NeededU(w["h0"], w["d"], ri, sg)

    @staticmethod
    def need_sets(rows, offsets, T):
        """bool [T,15,4]: [t, r, c - 1] <=> some move of table t's CSR list takes exactly c cards of rank r (a joker exists
        once: only c = 1)."""
        N = rows.shape[0]
        pos = torch.arange(N, device=rows.device, dtype=offsets.dtype)
        seg = torch.searchsorted(offsets[1:].contiguous(), pos, right=True).clamp_(max=T - 1).long()
        valid = pos < offsets[T]
        cnt = rows[:, :15].long().clamp(0, 4)
        cnt[:, 13:] = cnt[:, 13:].clamp(max=1)
        hit = (cnt[:, :, None] == torch.arange(1, 5, device=rows.device)[None, None, :]) & valid[:, None, None]   # [N,15,4]
        need = torch.zeros((T, 15, 4), dtype=torch.int32, device=rows.device)
        need.index_add_(0, seg, hit.to(torch.int32))
        return need > 0

    @torch.no_grad()
    def needed_torch(self, face, rows, offsets):
        """The same in plain torch from CSR lists (any device): the statement the engine's needed-rows kernels are tested
        against -- same row layout (rank segments from multiples of fc_tile(), inside a segment table-major then count), so
        row_index and seg compare exactly."""
        if self._ver != self._versions():
            self.refresh()
        T, P, H, H1 = face.shape[0], self.P, self.H, self.H1
        dev = face.device
        FC_TILE = fc_tile()
        need = self.need_sets(rows, offsets, T)                         # [T,15,4]
        per_rank = need.permute(1, 0, 2).reshape(15, T * 4)             # rank-major; inside a rank (t, c) order
        n_r = per_rank.sum(1)
        seg = torch.zeros(40, dtype=torch.int32, device=dev)
        row = 0
        starts = []
        for r in range(15):
            starts.append(row)
            seg[r], seg[16 + r] = row, row // FC_TILE
            row += (int(n_r[r]) + FC_TILE - 1) // FC_TILE * FC_TILE
        seg[15], seg[31], seg[32] = row, row // FC_TILE, int(n_r.sum())
        excl = per_rank.long().cumsum(1) - per_rank.long()
        idx = torch.where(per_rank, excl + torch.tensor(starts, device=dev)[:, None], -1).view(15, T, 4).permute(1, 0, 2)
        row_index = torch.full((T, 64), -1, dtype=torch.int32, device=dev)
        row_index[:, :52] = idx[:, :13].reshape(T, 52).to(torch.int32)
        row_index[:, 52], row_index[:, 53] = idx[:, 13, 0].to(torch.int32), idx[:, 14, 0].to(torch.int32)
        Y = self._first_layer_torch(face)                               # [15,5,T,H]
        y0 = Y[:, 0].permute(1, 0, 2).reshape(T, 15 * H).contiguous()
        dy = torch.zeros((max(row, FC_TILE), H), dtype=torch.float32, device=dev)
        d = torch.zeros((max(row, FC_TILE), H1), dtype=torch.float32, device=dev)
        for r in range(15):
            for c in range(1, 5 if r < 13 else 2):
                dst = idx[:, r, c - 1]
                m = dst >= 0
                dy[dst[m]] = Y[r, c][m] - Y[r, 0][m]
            d[starts[r]: starts[r] + int(n_r[r])] = dy[starts[r]: starts[r] + int(n_r[r])] @ self.W2[r]
            for c in range(1, 5 if r < 13 else 2):                      # the action plane's own term rides on the row
                dst = idx[:, r, c - 1]
                d[dst[dst >= 0]] += self.Z[r, c]
        h0 = torch.addmm(self.base, face.reshape(T, P * 60), self.Mz_f) + y0 @ self.Wd
        nu = NeededU(h0, d, row_index, seg)
        nu.y0, nu.dy = y0, dy
        return nu

    @torch.no_grad()
    def q_csr_needed(self, nu, rows, offsets):
        """q of every CSR row from a NeededU (plain torch; the statement ddz_q_slab_needed is tested against)."""
        T = nu.row_index.shape[0]
        N = rows.shape[0]
        pos = torch.arange(N, device=rows.device, dtype=offsets.dtype)
        seg = torch.searchsorted(offsets[1:].contiguous(), pos, right=True).clamp_(max=T - 1).long()
        cnt = rows[:, :15].long().clamp_(0, 4)
        cnt[:, 13:] = cnt[:, 13:].clamp(max=1)
        r = torch.arange(15, device=rows.device)
        col = torch.where(r[None, :] < 13, 4 * r[None, :] + cnt - 1, 52 + (r[None, :] - 13)).clamp(min=0)
        prow = nu.row_index.long()[seg[:, None], col]                   # [N,15]
        use = (cnt > 0) & (prow >= 0)
        dsum = (nu.d[prow.clamp(min=0)] * use[:, :, None]).sum(1)    # (Z[r][cnt] is part of the row)
        h = nu.h0[seg] + dsum
        return F.relu(h) @ self.w2 + self.b2

    def _first_layer_torch(self, face):
        T, P, H = face.shape[0], self.P, self.H
        X = face.permute(2, 0, 1, 3).reshape(15 * T, P * 4)
        S = torch.addmm(self.bias_f, X, self.Wf).view(15 * T, 4, H)
        return torch.stack([(S + self.A[cnt]).amax(dim=1).view(15, T, H) for cnt in range(5)], dim=1)

    @torch.no_grad()
    def q_csr(self, U, rows, offsets):
        """The per-row stage with plain torch ops over CSR lists (the training path, ragged_q; the tests' reference for
        the needed form): U from tables(), rows int8 [N,16] count rows (ddz_legal / ddz_slab_to_csr; rows beyond
        offsets[T] are padding and get some table's value), offsets int32 [T+1] -> q f32 [N].  No host sync: N is the
        buffer size."""
        T = U.shape[2]
        N = rows.shape[0]
        pos = torch.arange(N, device=rows.device, dtype=offsets.dtype)
        seg = torch.searchsorted(offsets[1:].contiguous(), pos, right=True).clamp_(max=T - 1).long()
        cnt = rows[:, :15].long().clamp_(0, 4)
        cnt[:, 13:] = cnt[:, 13:].clamp(max=1)                            # a joker exists once
        rc = torch.arange(15, device=rows.device)[None, :] * 5 + cnt      # [N,15]: (rank, count)
        h = F.embedding_bag(rc * T + seg[:, None], U.view(-1, self.H1), mode="sum")
        h = h + F.embedding_bag(rc, self.Z.view(-1, self.H1), mode="sum")
        return F.relu(h) @ self.w2 + self.b2

    @torch.no_grad()
    def q_slab(self, env, nu, out=None):
        """The per-row stage over the engine's slab lists (ddz_q_slab_needed) from needed()'s NeededU: q f32 [T, stride],
        entries beyond counts[t] untouched.  Feeds env.policy_step_slab / select_slab."""
        return env.q_slab_needed(nu.h0, nu.d, nu.row_index, self.w2, self.b2, out=out)


class NeededU:
    """FactorisedQ.needed's result: h0 f32 [T,256] (fc1's pre-activation of the pass: every count 0), d f32 [rows,256] (what a
    needed (rank, count >= 1) adds to it, the action plane's weights-only term Z[rank][count] included), row_index int32
    [T,64], seg int32 [40] (device: segment starts, rows in use)."""
    __slots__ = ("h0", "d", "row_index", "seg", "y0", "dy")

    def __init__(self, h0, d, row_index, seg):
        self.h0, self.d, self.row_index, self.seg = h0, d, row_index, seg
        self.y0 = self.dy = None


def ragged_q(net, face, rows, offsets):
    """Q(face_t, action) for every legal row of every table (dqn.py:56,67: policy_net(face, actions) for all tables at
    once): face f32 [T,P,15,4], rows int8 [N,16] + offsets int32 [T+1] in CSR order -> q f32 [N].  The factorised
    tables are cached on the network object and rebuilt when its weights change."""
    fq = getattr(net, "_ddz_factorised", None)
    if fq is None:
        fq = net._ddz_factorised = FactorisedQ(net)
    return fq.q_csr(fq.tables(face), rows, offsets)


class _Loop:
    """run(n) and capture(n) of a loop that has step(), refresh(), env and no host synchronisation in an iteration"""

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def capture(self, n=1):
        """n lock-step iterations as ONE hipGraph (the loop has no host synchronisation and no size-dependent shape):
        returns the torch.cuda.CUDAGraph; every .replay() runs the n iterations on the state the previous ones left (states,
        faces, choices, q values: bit for bit what n eager step() calls give -- tests/test_gpu_qnet.py).  Call step() a few
        times first (workspaces allocated, libraries warm).  An iteration is ~30 short launches: the replay removes the host's
        share of the gaps between them.
        The weights: the graph holds the addresses of the derived tables (FactorisedQ / RoleQ: fixed storage, written in place),
        not their values, and no Python runs at replay.  capture() refreshes them before it begins; weights that move WHILE the
        stream captures raise (RuntimeError from refresh()).  After a learner step -- an optimizer step, load_state_dict -- call
        loop.refresh() eagerly, then replay: the graph reads the current tables.  Without that call it plays the weights of the
        last refresh(): defined values, never freed memory.  A write through `.data` needs refresh(force=True); moving the
        network to another device reallocates the tables and is not allowed under a live graph."""
        dev = self.env.device
        self.refresh()
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self.run(n)
        torch.cuda.current_stream(dev).wait_stream(s)
        return g


class PolicyLoop(_Loop):
    """game.py:95-104 for T tables with a Q-network on every seat, one lock-step iteration per step(), no per-table work on
    the host:
        face -> Q of every legal move of every table (slab layout) -> ddz_policy_step_slab (epsilon-greedy arg-max + apply +
        next lists + next face, ONE launch).
    The Q values come from FactorisedQ.needed -- the rows legal moves use, found on the device; the per-rank rows GEMM on
    the engine's fp32 MFMA kernel (segment sizes stay in device memory), the plain dense GEMM by hipBLASLt (gemm="mfma":
    by the same MFMA kernel); nothing crosses to the host, every launch is graph-capturable."""

    def __init__(self, env, net, face_variant=3, epsilon=0.0, auto_reset=True, gemm="torch", shared=None):
        from .engine import FACE_PLANES
        if FACE_PLANES[face_variant] != net.planes:
            raise ValueError("the network's input planes do not match the face variant")
        self.env, self.fq = env, FactorisedQ(net)
        self.variant, self.epsilon, self.auto_reset = int(face_variant), float(epsilon), bool(auto_reset)
        self.gemm = gemm
        # shared rows (FactorisedQ.needed(shared=True)): allowed for face variants 1, 2 and 3, whose columns ddz_q_shared_rows /
        # ddz_q_shared_rows_hashed key from the environment's state; the default for variant 3 (EnvCooperationSimplify) only
        # (True: H0 from shared rows; "all": the needed rows D shared as well -- variant 3's default)
        self.shared = ("all" if int(face_variant) == 3 else False) if shared is None else \
            ("all" if shared == "all" else bool(shared))
        if self.shared and int(face_variant) not in (1, 2, 3):
            raise ValueError("shared rows need face variant 1, 2 or 3")
        T = env.T
        self.face = env.observe(self.variant)
        self.q = torch.zeros((T, env.slab_stride), dtype=torch.float32, device=env.device)
        self.choice = torch.empty(T, dtype=torch.int32, device=env.device)
        if not env._slab_fresh:
            env.legal_slab()

    def describe(self):
        if self.shared:
            finder = ("ddz_q_shared_rows (one row per DISTINCT (rank, face column) of the batch, direct-addressed, on the device)"
                      if self.variant == 3 else
                      "ddz_q_shared_rows_hashed (one row per DISTINCT (rank, face column) of the batch, found in a hashed table "
                      "with one open-addressed region per rank, on the device)")
            return ("ddz_q_need (the (rank, count) rows the legal moves use) + " + finder + " -> ddz_q_features_rows (first layer "
                    "of the shared rows) + "
                    "ddz_q_features_needed (dY of the needed rows) -> ddz_q_fc1_rows twice (G = Y x fc1[rank] over the shared rows, "
                    "D = dY x fc1[rank] over the needed rows: k_fc1, segment tables in device memory) -> H0 = table term + "
                    "ddz_q_gather_h0 (the fifteen shared rows of every table; no dense K = 3840 GEMM) -> ddz_q_slab_needed -> "
                    "ddz_policy_step_slab(greedy, face): every legal action of every table gets its exact Q value each iteration "
                    "from the current weights; nothing is kept between iterations, nothing crosses to the host")
        return ("ddz_q_need (the (rank, count) rows the legal moves use, on the device) -> ddz_q_features_needed (first "
                "layer: y0 per table + dY per needed row) -> H0 = tab + y0 x Wd (K = 3840: "
                + ("torch.addmm / hipBLASLt" if self.gemm == "torch" else "ddz_q_fc1_dense, the fp32 MFMA kernel k_fc1")
                + ") + ddz_q_fc1_rows (D = dY x fc1[rank], k_fc1 with the segment table in device memory)"
                + " -> ddz_q_slab_needed -> ddz_policy_step_slab(greedy, face): every legal action of every table gets its Q "
                "value each iteration; nothing crosses to the host")

    def refresh(self, force=False):
        """FactorisedQ.refresh: the derived tables brought up to date in place (eager steps do it themselves; a captured graph
        needs it after every learner step -- _Loop.capture); returns whether anything was recomputed"""
        return self.fq.refresh(force)

    def q_values(self):
        """q [T, stride] of the current lists (valid in [:, :counts[t]])"""
        return self.fq.q_slab(self.env, self.fq.needed(self.env, self.face, gemm=self.gemm, shared=self.shared), out=self.q)

    def step(self, traj=None):
        q = self.q_values()
        done, r, illegal, _ = self.env.policy_step_slab(q, self.epsilon, face_variant=self.variant, face_out=self.face,
                                                        choice_out=self.choice, auto_reset=self.auto_reset, traj=traj)
        return done, r, illegal

    def profile(self, n=10):
        """Per-stage device time of n iterations: FactorisedQ.needed itself, issued through its stage hook with HIP events on the
        launching stream around every stage, then the row stage and the step; with each stage's algorithmic FLOP or bytes:
        {stage: {"us", "kernel", "flop" | "bytes", "note"}}.  Synchronises."""
        from .engine import shared_row_width
        env, fq, T, P, H = self.env, self.fq, self.env.T, self.fq.P, self.fq.H
        shared, all_ = bool(self.shared), self.shared == "all"
        ev = {}
        rows_needed = rows_padded = moves = rows_shared = rows_shared_padded = rows_private = 0

        def timed(name, fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.setdefault(name, []).append((a, b))

        self.q_values()                                                   # (workspace exists)
        w = fq._ws[("needed", self.face.device, T)]
        for _ in range(int(n)):
            nu = fq.needed(env, self.face, gemm=self.gemm, shared=self.shared, hook=timed)
            timed("row_stage", lambda: fq.q_slab(env, nu, out=self.q))
            seg = nu.seg.cpu()
            rows_needed += int(seg[32]); rows_padded += int(seg[15]); moves += int(env.counts.sum())
            if shared:
                sseg = w["sseg"].cpu()
                rows_shared += int(sseg[32]); rows_shared_padded += int(sseg[15])
            if all_:
                rows_private += int(w["seg"].cpu()[32])
            timed("env_step", lambda: env.policy_step_slab(self.q, self.epsilon, face_variant=self.variant, face_out=self.face,
                                                           choice_out=self.choice, auto_reset=self.auto_reset))
        torch.cuda.synchronize(env.device)
        rn, rp, mv = rows_needed / n, rows_padded / n, moves / n
        rs, rsp, priv = rows_shared / n, rows_shared_padded / n, rows_private / n
        K = shared_row_width(P)
        region = 2048
        while region < 2 * T:                                              # the hashed finder's region per rank (ddz_qnet.h 5b)
            region *= 2
        nslot = 15 * region
        distinct = f"one row per distinct (rank, face column): {rs:.0f} of the {15 * T} columns ({rs / (15 * T):.3f}); "
        nd = "" if shared else "needed "
        # one description per stage, in the order of the report; the stages that ran select theirs
        stages = {
            "need": {"kernel": "k_q_need_mask + k_q_need_scan + k_q_need_assign", "bytes": mv * 16 + T * (8 + 8 + 256),
                     "note": "list rows read, need sets written and read, row_index written"},
            "shared_rows": ({"kernel": "memset + k_qs_mark + k_qs_count + k_qs_seg + k_qs_assign + k_qs_rows",
                             "bytes": T * 176 + 3 * 4134375 * 4 + T * 16 * 4 * 3 + rs * 8,
                             "note": distinct + "state read, the 16.5-MB slot table cleared / counted / assigned, rows [T,16] written"}
                            if self.variant == 3 else
                            {"kernel": f"memset + k_qs_hmark<{self.variant}> + k_qs_count + k_qs_seg + k_qs_assign + k_qs_rows",
                             "bytes": T * 176 + nslot * (12 + 4 + 4) + T * 16 * 4 * 3 + rs * 8,
                             "note": distinct + f"state read, the hashed table ({nslot} slots, {nslot * 12 / 1e6:.1f} MB) cleared / probed / "
                                     "counted / assigned, rows [T,16] written"}),
            "features_shared": {"kernel": f"k_q_feat_rows<{P}>", "bytes": rs * (P * 16 + K * 4),
                                "note": f"first layer (count 0) of the shared rows + the table term of their columns (linear in the "
                                        f"face: folded into the rows -- no [T, {60 * P}] x [{60 * P}, 256] GEMM per iteration)"},
            "fc1_shared": {"kernel": "k_fc1<true>", "flop": 2.0 * rs * K * H,
                           "note": f"G = [Y | column] x [fc1[rank] ; Mz[rank]] (K = {K}) over the {rs:.0f} shared rows ({rsp:.0f} with the padding of the fifteen "
                                   f"segments) -- the dense form of the same term is 2 x {T} x 3840 x 256 = {2.0 * T * 15 * H * H / 1e9:.0f} GFLOP"},
            "gather_h0": {"kernel": "k_qs_gather", "bytes": T * (64 + 2 * H * 4) + rs * H * 4,
                          "note": f"H0 read and written, rows [T,16] read, every row of G once ({rs * H * 4 / 1e6:.0f} MB: the fifteen "
                                  f"1-KB reads per table -- {T * 15 * H * 4 / 1e9:.2f} GB -- are served by L2 / MALL)"},
            "shared_need": {"kernel": "memset + k_qd_mark + k_qd_count + k_qd_seg + k_qd_assign + k_qd_remap",
                            "bytes": T * 64 * 4 * 3 + T * 64 + rs * 16 * 3 + rn * 5, "needed_triples": priv,
                            "note": f"one D row per distinct (shared row, count) some table needs: {rn:.0f} rows for the "
                                    f"{priv:.0f} needed (table, rank, count) triples ({priv / T:.2f} per table)"},
            "features": ({"kernel": f"k_q_feat_drows<{P}>", "bytes": rn * (P * 16 + H * 4 + 8), "note": "dY of the shared D rows"}
                         if all_ else
                         {"kernel": f"k_q_feat_needed<{P}> (y0 = null)", "bytes": T * P * 240 + rn * H * 4 + T * 256,
                          "note": "face + row_index read, dY [needed rows, 256] written; ranks no legal move touches are skipped"}
                         if shared else
                         {"kernel": f"k_q_feat_needed<{P}>", "bytes": T * P * 240 + T * 15 * H * 4 + rn * H * 4 + T * 256,
                          "note": "face + row_index read, y0 [T, 3840] + dY [needed rows, 256] written"}),
            "table_term": {"kernel": "torch.addmm (hipBLASLt)", "flop": 2.0 * T * P * 60 * H,
                           "note": "fc1 bias + the face part of conv_shunzi: [T, 60 P] x [60 P, 256]"},
            "fc1_dense": {"kernel": "k_fc1<false>" if self.gemm == "mfma" else "torch.addmm (hipBLASLt)",
                          "flop": 2.0 * T * 15 * H * H, "note": "H0 += y0 [T, 3840] x Wd [3840, 256]"},
            "fc1_rows": {"kernel": "k_fc1<true>", "flop": 2.0 * rn * H * H,
                         "note": f"D = dY x fc1[rank]: {rn:.0f} {nd}rows per iteration ({rn / T:.2f} per table), {rp:.0f} computed "
                                 f"with the padding of the fifteen tile-aligned {'' if shared else '(256-row) '}segments; FLOP of the {nd}rows"},
            "row_stage": {"kernel": "k_q_slab_needed", "bytes": T * H * 4 + rn * H * 4 + mv * 20,
                          "note": f"H0 + the {nd}D rows + the list rows read, q written"},
            "env_step": {"kernel": "k_slab<4,true>", "bytes": T * (2 * 176 + P * 240 + 8) + mv * 24,
                         "note": "arg-max over q, apply, new lists, new face"},
        }
        us = {k: sum(a.elapsed_time(b) for a, b in v) * 1e3 / len(v) for k, v in ev.items()}
        return {k: {"us": us[k], **d} for k, d in stages.items() if k in us}

    def variants(self, timed_loop, sync):
        """env steps/s of the other forms of the same loop on the same environment (bench.py): H0 from the dense K = 3840
        GEMM over every table, by hipBLASLt and by k_fc1."""
        out = {}
        T = self.env.T
        other = "mfma" if self.gemm == "torch" else "torch"
        forms = [("needed_dense_gemm_by_" + ("k_fc1" if other == "mfma" else "hipblaslt"), {"gemm": other, "shared": False})]
        if self.shared:   # the dense form of H0 (round 4's first form: one K = 3840 GEMM over every table)
            forms.insert(0, ("needed_dense_gemm_by_" + ("hipblaslt" if self.gemm == "torch" else "k_fc1"),
                             {"gemm": self.gemm, "shared": False}))
        for name, kw in forms:
            loop = PolicyLoop(self.env, self.fq.net, face_variant=self.variant, epsilon=self.epsilon, **kw)
            loop.run(2)
            dt, reps = timed_loop(lambda: loop.run(5), sync, min_s=0.2, max_reps=64)
            out[name + "_env_steps_per_s"] = T * 5 * reps / dt
            del loop
        return out


ROLE_ORDER = ("up", "lord", "down")      # the engine's role ids 0, 1, 2


def role_slots(nets, face_variant):
    """{"lord" | "down" | "up": QNet | None} (missing keys: None) -> (slot networks, net_of_role [3] in role order up, lord, down:
    a slot or -1 = the rule agent).  Equal network objects share one slot; slots are numbered in role order.  Raises ValueError
    for an unknown role, a map without a network, face variant 0 or one the shared rows do not key, and planes that differ
    between the networks or from the variant.  Pure Python: no device is touched."""
    from .engine import FACE_PLANES
    unknown = set(nets) - set(ROLE_ORDER)
    if unknown:
        raise ValueError(f"unknown role(s) {sorted(unknown)}: the roles are lord, down and up")
    v = int(face_variant)
    if v not in (1, 2, 3):
        raise ValueError("per-role networks need face variant 1, 2 or 3 (the faces the shared rows key; variant 0 has none)")
    slots, net_of_role = [], []
    for role in ROLE_ORDER:
        net = nets.get(role)
        if net is None:
            net_of_role.append(-1)
            continue
        for s, other in enumerate(slots):
            if other is net:
                net_of_role.append(s)
                break
        else:
            net_of_role.append(len(slots))
            slots.append(net)
    if not slots:
        raise ValueError("the role map has no network (an all-rule game is BatchedEnv.step_auto(0b111))")
    if len({int(n.planes) for n in slots}) != 1:
        raise ValueError("the networks' input planes differ: all roles share one face variant")
    if int(slots[0].planes) != FACE_PLANES[v]:
        raise ValueError(f"the networks take {slots[0].planes} planes, face variant {v} has {FACE_PLANES[v]}")
    return slots, net_of_role


class RoleQ:
    """The multi-network counterpart of FactorisedQ's shared-rows form (needed(shared="all")): one network per role, or the rule
    agent (Game, game.py:11-43).  One pass over the tables whose actor has a network: the shared rows keyed by (network slot,
    rank, column) (csrc/ddz_qnet.h section 7), the per-slot GEMMs on the slot's weights, H0 / D / q of a table from its own
    network -- bit for bit what FactorisedQ(net of the table's role).needed(env, face, shared="all") + q_slab give.  Tables played
    by the rule agent take no part (their q entries are left alone).  The stacked weight tables (STACKED: slot s holds the
    table of network s) follow FactorisedQ's contract: allocated once per object and device, the slots of the networks whose
    parameter versions moved rewritten in place by refresh() -- every eager needed() calls it; a captured pass plays the tables
    of the last refresh() until the caller refreshes eagerly; a write through `.data` needs refresh(force=True)."""
    STACKED = ("Wf", "bias_f", "A", "W2x", "W2", "Z", "base", "w2", "b2")

    def __init__(self, nets, face_variant):
        self.nets, self.net_of_role = role_slots(nets, face_variant)
        self.variant, self.N = int(face_variant), len(self.nets)
        self.fqs = [FactorisedQ(n) for n in self.nets]
        self.P = self.fqs[0].P
        self._ws = {}
        self._ver = self._dev = None
        self.refresh()

    def _versions(self):
        return tuple(fq._versions() for fq in self.fqs)

    @torch.no_grad()
    def refresh(self, force=False):
        """Bring the slots of the networks whose weights moved (every slot when forced) up to date, in place; returns whether
        anything was recomputed.  Raises RuntimeError while the current stream is capturing, as FactorisedQ.refresh."""
        now = self._versions()
        if not force and now == self._ver:
            return False
        dev = self.fqs[0].net.fc1.weight.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a network's weights moved (or refresh(force=True)) while the stream is capturing: call "
                               "refresh() before the capture begins")
        for fq in self.fqs:
            fq.refresh(force)
        stale = [force or self._ver is None or self._ver[s] != now[s] for s in range(self.N)]
        if dev != self._dev:                                            # (one device for all: the kernels take one)
            for name in self.STACKED:
                t = getattr(self.fqs[0], name)
                shape = (self.N,) if name == "b2" else (self.N,) + tuple(t.shape)
                setattr(self, name, torch.zeros(shape, dtype=torch.float32, device=dev))
            self._dev, stale = dev, [True] * self.N
        for s, fq in enumerate(self.fqs):
            if stale[s]:
                for name in self.STACKED:
                    getattr(self, name)[s: s + 1].copy_(getattr(fq, name).view((1,) + tuple(getattr(self, name).shape[1:])))
        self._ver = now
        return True

    def _workspace(self, env, face):
        from . import engine as E
        T, dev, N, H = env.T, face.device, self.N, _CONV_CH
        key = (dev, T)
        if key not in self._ws:
            self._ws.clear()
            cap, scap = row_capacities(T, self.variant)                            # per slot
            z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
            self._ws[key] = {
                "cap": cap, "scap": scap,
                "scratch": z(E.q_need_scratch_bytes(T), dt=torch.uint8), "row_index": z(T, 64, dt=torch.int32),
                "seg": z(40, dt=torch.int32), "row_cnt": z(cap, dt=torch.uint8),
                "sws": z(E.q_roles_ws_bytes(T, self.variant, N), dt=torch.uint8), "srows": z(T, 16, dt=torch.int32),
                "srep": z(N * scap, dt=torch.int32), "sseg": z(N, 40, dt=torch.int32), "slot": z(T, dt=torch.int8),
                "ys": z(N * scap, E.shared_row_width(self.P)), "g": z(N * scap, H), "h0": z(T, H),
                "dws": z(E.q_roles_need_ws_bytes(scap, N), dt=torch.uint8), "row_index2": z(T, 64, dt=torch.int32),
                "drep": z(N * cap, dt=torch.int32), "dseg": z(N, 40, dt=torch.int32), "drow_cnt": z(N * cap, dt=torch.uint8),
                "dy": z(N * cap, H), "d": z(N * cap, H),
                "side": torch.cuda.Stream(dev), "fork0": torch.cuda.Event(), "fork": torch.cuda.Event(), "join": torch.cuda.Event()}
        return self._ws[key]

    @torch.no_grad()
    def needed(self, env, face):
        """face f32 [T,P,15,4]: env's own face of the variant of its CURRENT states -> RolesU (h0, d, row_index, seg, slot; device,
        aliases this object's workspace).  As FactorisedQ.needed(shared="all"): the need sets and the D chain on a side stream
        beside the finder and the H0 chain (fork / join by events), nothing crosses to the host, every launch is capturable."""
        from . import engine as E
        if self._ver != self._versions():
            self.refresh()
        T, P, N = face.shape[0], self.P, self.N
        if tuple(face.shape[1:]) != (P, 15, 4) or T != env.T or not face.is_cuda:
            raise ValueError(f"face must be a device tensor [T,{P},15,4] of the environment's tables")
        w = self._workspace(env, face)
        with _beside(w, "fork0", True):
            env.q_need(w["cap"], w["scratch"], w["row_index"], w["seg"], w["row_cnt"])
        env.q_roles_rows(self.variant, self.net_of_role, N, w["sws"], w["scap"], w["srows"], w["srep"], w["sseg"], w["slot"])
        with _beside(w, "fork", True):
            env.q_roles_need(N, w["row_index"], w["srows"], w["sseg"], w["scap"], w["dws"], w["cap"], w["row_index2"], w["drep"],
                             w["dseg"], w["drow_cnt"])
            E.q_roles_features_drows(face, N, self.Wf, self.bias_f, self.A, w["srep"], w["scap"], w["drep"], w["dseg"], w["dy"], w["cap"])
            E.q_roles_fc1_rows(N, w["dy"], w["dseg"], w["drow_cnt"], self.W2, self.Z, w["d"], w["cap"])
        E.q_roles_features_rows(face, N, self.Wf, self.bias_f, w["srep"], w["sseg"], w["ys"], w["scap"])
        E.q_roles_fc1_rows_k(N, w["ys"], w["sseg"], self.W2x, w["g"], w["scap"])
        E.q_roles_gather_h0(N, w["g"], w["srows"], w["slot"], self.base, w["h0"])   # H0[t] = base[slot] + sum_r G[row(t, r)]
        _join(w, True)
        return RolesU(w["h0"], w["d"], w["row_index2"], w["dseg"], w["slot"])

    @torch.no_grad()
    def q_slab(self, env, nu, out):
        """ddz_q_roles_slab: q f32 [T, stride] of every legal move of every network table (rule tables' entries left alone)."""
        return env.q_roles_slab(self.N, nu.slot, nu.h0, nu.d, nu.row_index, self.w2, self.b2, out)


class RolesU:
    """RoleQ.needed's result: NeededU's fields (seg: int32 [N,40] of the D rows, one block per slot) + slot int8 [T] (-1: rule)."""
    __slots__ = ("h0", "d", "row_index", "seg", "slot")

    def __init__(self, h0, d, row_index, seg, slot):
        self.h0, self.d, self.row_index, self.seg, self.slot = h0, d, row_index, seg, slot


class SeatLoop(_Loop):
    """game.py:95-106 for T tables with a network or the rule agent per role, one lock-step iteration per step():
        act():   RoleQ's pass over the network tables -> greedy choice (ddz_select_slab) and, with epsilon per role, the
                 epsilon-greedy choice (trained roles explore, game.py:95-104) -> the rule agent's move for the roles mapped to
                 None (auto_choose) -> one action id per table
        apply(): one step of every table (step_slab(STEP_IDS), re-deal of finished tables) and the next face.
    Between act() and apply() a training driver reads face (the face the network tables chose on), choice / greedy (indices
    into the slab lists; valid for network tables, slot >= 0) and ids (what every table plays): TransitionAssembler.before_step
    takes them.  Nothing crosses to the host; capture(n) records n iterations as one graph."""

    def __init__(self, env, nets, face_variant, epsilon=0.0, auto_reset=True):
        self.rq = RoleQ(nets, face_variant)
        eps = self._eps_arg(epsilon)
        self.env, self.variant, self.auto_reset = env, int(face_variant), bool(auto_reset)
        nr = self.rq.net_of_role
        self.eps = [e if nr[k] >= 0 else 0.0 for k, e in enumerate(eps)]
        self.auto_roles = sum(1 << k for k in range(3) if nr[k] < 0)
        T, dev = env.T, env.device
        self.face = env.observe(self.variant)
        self.q = torch.full((T, env.slab_stride), float("nan"), dtype=torch.float32, device=dev)
        self.greedy = torch.empty(T, dtype=torch.int32, device=dev)
        self.choice = self.greedy if not any(self.eps) else torch.empty(T, dtype=torch.int32, device=dev)
        self._eps_of_role = torch.tensor(self.eps, dtype=torch.float32, device=dev)
        self._auto = torch.empty(T, dtype=torch.int32, device=dev)
        self.ids = torch.empty(T, dtype=torch.int32, device=dev)
        self.slot = None
        if not env._slab_fresh:
            env.legal_slab()

    @staticmethod
    def _eps_arg(epsilon):
        """a float for every role, or {"lord" | "down" | "up": float}, in role order"""
        if not isinstance(epsilon, dict):
            return [float(epsilon)] * 3
        bad = set(epsilon) - set(ROLE_ORDER)
        if bad:
            raise ValueError(f"unknown role(s) {sorted(bad)} in epsilon")
        return [float(epsilon.get(r, 0.0)) for r in ROLE_ORDER]

    def refresh(self, force=False):
        """RoleQ.refresh: the stacked tables of the networks that moved brought up to date in place (eager steps do it
        themselves; a captured graph needs it after every learner step -- _Loop.capture); returns whether anything was
        recomputed"""
        return self.rq.refresh(force)

    def q_values(self):
        """q [T, stride] of the current lists for the network tables (valid in [t, :counts[t]] where slot[t] >= 0)"""
        nu = self.rq.needed(self.env, self.face)
        self.slot = nu.slot
        return self.rq.q_slab(self.env, nu, self.q)

    def act(self):
        env = self.env
        q = self.q_values()
        env.select_slab(q, 0.0, out=self.greedy)
        if self.choice is not self.greedy:
            self.choice.copy_(self.greedy)
            role_eps = self._eps_of_role[env.role.long()]
            for e in sorted(set(e for e in self.eps if e > 0)):
                self.choice.copy_(torch.where(role_eps == e, env.select_slab(q, e), self.choice))
        net_ids = env.slab_ids().gather(1, self.choice.clamp(min=0).long()[:, None])[:, 0]
        if self.auto_roles:
            env.auto_choose(self.auto_roles, out=self._auto)
            self.ids.copy_(torch.where(self.slot >= 0, net_ids, self._auto))
        else:
            self.ids.copy_(net_ids)
        return self.ids

    def set_epsilon(self, epsilon):
        """new exploration rates (a float for every network role, or {"lord" | "down" | "up": float}) for the next act(); a host
        value, as in __init__: a captured graph keeps the rates it was captured with"""
        eps = self._eps_arg(epsilon)
        nr = self.rq.net_of_role
        self.eps = [e if nr[k] >= 0 else 0.0 for k, e in enumerate(eps)]
        self._eps_of_role.copy_(torch.tensor(self.eps, dtype=torch.float32))
        if any(self.eps) and self.choice is self.greedy:
            self.choice = torch.empty(self.env.T, dtype=torch.int32, device=self.env.device)
        elif not any(self.eps):
            self.choice = self.greedy

    def apply(self, traj=None):
        from .engine import STEP_IDS
        done, r, illegal = self.env.step_slab(self.ids, STEP_IDS, auto_reset=self.auto_reset, traj=traj)
        self.env.observe(self.variant, out=self.face)
        return done, r, illegal

    def step(self, traj=None):
        self.act()
        return self.apply(traj)



class QLeaf:
    """A leaf evaluator for engine.GuidedSearch.run (search spec v3): the value of a leaf is its actor's best Q.  The leaf rows
    are imported into a scratch BatchedEnv of one table per item (made once; anew when a later search has another item count,
    device or rule set), q of every legal move comes from the
    shared-rows pass keyed by network slot (SeatLoop.q_values: the leaves of a search are near-duplicates, which is where
    that pass is at its best), and ddz_guided_values turns the maximum into 1024ths: p = qmax / reward[role] is the expected
    outcome in [-1, 1] for the actor's side, value = rint((p + 1) * 512) clamped.  nets: {"lord" | "down" | "up": QNet | None};
    leaves whose actor has no network are left to `fallback` (another evaluator, e.g. engine.PlayoutLeaf), which is called
    first; without one every role needs a network.  A search with a `priors` field (BatchedEnv.guided_puct, search spec v5)
    also gets the weight of every move of a leaf from the same q slab (ddz_puct_priors): w_j = rint(255 * exp((q_j - qmax) /
    (reward[role] * tau))), the best move 255; tau: the temperature, in units of the role's reward."""

    def __init__(self, nets, face_variant, reward_dict=None, fallback=None, tau=1.0):
        if not float(tau) > 0.0:
            raise ValueError("tau must be positive")
        self.inv_tau = 1.0 / float(tau)
        _, self.net_of_role = role_slots(nets, face_variant)
        if fallback is None and min(self.net_of_role) < 0:
            missing = [r for r, s in zip(ROLE_ORDER, self.net_of_role) if s < 0]
            raise ValueError(f"no network for {missing} and no fallback evaluator for their leaves")
        rd = dict(REWARD_DICT if reward_dict is None else reward_dict)
        self.inv_reward = [1.0 / float(rd[r]) for r in ROLE_ORDER]
        self.net_roles = sum(1 << k for k in range(3) if self.net_of_role[k] >= 0)
        self.nets, self.variant, self.fallback = nets, int(face_variant), fallback
        self.loop = None

    def scratch(self, search):
        from .engine import BatchedEnv
        if (self.loop is None or self.loop.env.T != search.n_items or self.loop.env.device != search.env.device
                or self.loop.env.native_joker_kickers != search.env.native_joker_kickers):
            env = BatchedEnv(search.n_items, seed=search.env.seed, device=search.env.device,
                             native_joker_kickers=search.env.native_joker_kickers)
            self.loop = SeatLoop(env, self.nets, self.variant, auto_reset=False)
        return self.loop

    def refresh(self, force=False):
        """SeatLoop.refresh of the scratch loop (False before the first search made it: a new loop is built from the current
        weights).  An eager run refreshes itself at every leaf pass; a captured search needs the call after a learner step."""
        return False if self.loop is None else self.loop.refresh(force)

    def q_values(self, search):
        """q f32 [n_items, stride] of the leaves' lists (valid where the leaf's actor has a network) and the scratch env"""
        loop = self.scratch(search)
        env = loop.env
        env.state_import(search.leaves)
        env.legal_slab()
        env.observe(self.variant, out=loop.face)
        return loop.q_values(), env

    def __call__(self, search):
        from .engine import guided_values, puct_priors
        if self.fallback is not None:
            self.fallback(search)
        q, env = self.q_values(search)
        if getattr(search, "priors", None) is not None:
            puct_priors(search.leaves, env.counts, q, self.inv_reward, inv_tau=self.inv_tau, net_roles=self.net_roles, out=search.priors)
        return guided_values(search.leaves, env.counts, q, self.inv_reward, net_roles=self.net_roles, out=search.values)


def _compete_net(x, face_variant, device, cache):
    """a compete() role entry: None, a QNet, or the path of a reference state dict (loaded weights_only)"""
    if x is None or isinstance(x, nn.Module):
        return x
    from . import metrics
    from .engine import FACE_PLANES
    path = str(x)
    if path not in cache:
        sd = metrics.load_state_dict(abspath=path)
        net = QNet(int(sd["conv1.weight"].shape[1]) - 1 if "conv1.weight" in sd else FACE_PLANES[int(face_variant)])
        net.load_state_dict(sd)
        cache[path] = net.to(device).eval()
    return cache[path]


@torch.no_grad()
def compete(face_variant, nets, total, tables=4096, seed=0, book=None, device="cuda:0", check_every=8):
    """Game.compete (game.py:240-290) on the batched engine: greedy networks (QNet, or the path of a reference state dict) and the
    rule agent (None) per role, lock-step iterations over `tables` tables until at least `total` episodes have finished (checked
    every `check_every` iterations: one host sync each).  Returns {"lord", "down", "up": wins, "episodes", "iterations"} from
    BatchedEnv.stats() deltas (the wins sum to the episodes); with `book` (metrics.WinRateBook) the same stats feed it."""
    from .engine import BatchedEnv
    cache = {}
    nets = {r: _compete_net(v, face_variant, device, cache) for r, v in nets.items()}
    env = BatchedEnv(int(tables), seed=int(seed), device=device)
    env.reset()
    env.legal_slab()
    if all(v is None for v in nets.values()) and not (set(nets) - set(ROLE_ORDER)):
        step = lambda: env.step_auto(0b111, slab=True)     # noqa: E731   (the rule agent on every seat)
    else:
        step = SeatLoop(env, nets, face_variant, 0.0).step
    s0 = env.stats()
    if book is not None:
        book.update(s0)
    it = 0
    while True:
        for _ in range(int(check_every)):
            step()
        it += int(check_every)
        s1 = env.stats()
        if s1["episodes"] - s0["episodes"] >= int(total):
            break
    if book is not None:
        book.update(s1)
    env.close()
    return {"lord": s1["lord_wins"] - s0["lord_wins"], "down": s1["down_wins"] - s0["down_wins"],
            "up": s1["up_wins"] - s0["up_wins"], "episodes": s1["episodes"] - s0["episodes"], "iterations": it}


class Replay:
    """Ring buffer of transitions on the device (dqn.py:11,22-23: deque(maxlen=REPLAY_SIZE) of tuples)."""

    def __init__(self, size, planes, device):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
        self.s0, self.a0, self.s1, self.a1 = z(size, planes, 15, 4), z(size, 15, 4), z(size, planes, 15, 4), z(size, 15, 4)
        self.r, self.done = z(size), torch.zeros(size, dtype=torch.bool, device=device)
        self.size, self.n, self.head = size, 0, 0

    def push(self, tr):
        k = tr["reward"].numel()
        if k == 0:
            return
        if k > self.size:
            tr = {key: v[-self.size:] for key, v in tr.items()}
            k = self.size
        idx = (self.head + torch.arange(k, device=self.r.device)) % self.size
        self.s0[idx], self.a0[idx], self.s1[idx], self.a1[idx] = tr["s0"], tr["a0"], tr["s1"], tr["a1"]
        self.r[idx], self.done[idx] = tr["reward"], tr["done"]
        self.head = (self.head + k) % self.size
        self.n = min(self.size, self.n + k)

    def sample(self, k):
        idx = torch.randint(0, self.n, (k,), device=self.r.device)
        return {"s0": self.s0[idx], "a0": self.a0[idx], "s1": self.s1[idx], "a1": self.a1[idx],
                "reward": self.r[idx], "done": self.done[idx]}


EPSILON_HIGH, EPSILON_LOW, DECAY = 0.5, 0.01, int((8000 * (2 / 3)) / 5)   # config.py:9-13


def epsilon_schedule(episode, high=EPSILON_HIGH, low=EPSILON_LOW, decay=DECAY):
    """DQNFirst.update_epsilon (dqn.py:73-76): low + (high - low) * exp(-episode / decay)."""
    import math
    return low + (high - low) * math.exp(-1.0 * episode / decay)


def td_step(policy, target, optimizer, batch, gamma=0.95, fused=False):
    """One perceive() update (dqn.py:33-48): y = r + (1 - done) * gamma * Q_target(s1, a1), MSE against
    Q_policy(s0, a0), one optimizer step.  Returns the loss (a tensor: no host sync).  fused: True -- both passes through
    QNet.forward_fused (the first layer by the engine's forward / backward kernels) -- or "stage" -- through QNet.forward_stage
    (everything in front of dropout by the engine's kernels) -- instead of the literal forward.  A PackedBatch as `batch`
    (TransitionRecorder.sample_packed) runs both passes through QNet.forward_packed, whatever `fused` says: two stage launches
    per pass, no face, no library convolution; the reward and done gathers are the only other reads of the ring."""
    if isinstance(batch, PackedBatch):
        q_next = lambda: target.forward_packed(batch, 1)      # noqa: E731
        q_now = lambda: policy.forward_packed(batch, 0)       # noqa: E731
        tr = {"reward": batch.reward[batch.index], "done": batch.done[batch.index].bool()}
    else:
        if isinstance(fused, str):
            if fused != "stage":
                raise ValueError('fused: False, True or "stage"')
            q_target, q_policy = target.forward_stage, policy.forward_stage
        else:                                                  # (any other value by its truth, as before)
            q_target, q_policy = (target.forward_fused, policy.forward_fused) if fused else (target, policy)
        q_next = lambda: q_target(batch["s1"], batch["a1"])   # noqa: E731
        q_now = lambda: q_policy(batch["s0"], batch["a0"])    # noqa: E731
        tr = batch
    with torch.no_grad():
        y = td_target(tr, q_next(), gamma)
    loss = F.mse_loss(q_now().view(-1), y)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach()


def mc_step(policy, optimizer, batch, fused=False):
    """One update onto Monte-Carlo return targets: MSE of Q_policy(s0, a0) against the batch's `ret` (ReturnRecorder.sample /
    ReturnAssembler), one optimizer step -- td_step without the target pass.  Returns the loss (a tensor: no host sync).  fused
    as in td_step: False the literal forward, True QNet.forward_fused, "stage" QNet.forward_stage; a ReturnBatch
    (ReturnRecorder.sample_packed) goes through QNet.forward_packed whatever `fused` says."""
    if isinstance(batch, ReturnBatch):
        q, ret = policy.forward_packed(batch, 0), batch.ret[batch.index]
    else:
        if isinstance(fused, str):
            if fused != "stage":
                raise ValueError('fused: False, True or "stage"')
            q_policy = policy.forward_stage
        else:
            q_policy = policy.forward_fused if fused else policy
        q, ret = q_policy(batch["s0"], batch["a0"]), batch["ret"]
    loss = F.mse_loss(q.view(-1), ret)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach()


# ------------------------------------------------------------------------------------------------
# The same bookkeeping on the device (csrc/ddz_replay.h): TransitionAssembler + one Replay per role as three launches per call,
# transitions kept packed (two 176-byte state rows, two action ids, reward, done, table) and decoded into faces / thermometers
# when a batch is drawn.  TransitionAssembler and Replay above stay as the statement the recorder is tested against.
REPLAY_SIZE, BATCH_SIZE, GAMMA, UPDATE_TARGET_EVERY, LEARNING_RATE = 20000, 256, 0.95, 20, 1e-4   # config.py:8-14, dqn.py:19


def _role_id(role):
    if isinstance(role, str):
        if role not in ROLE_ORDER:
            raise ValueError("role must be up / lord / down (or its id 0 / 1 / 2)")
        return ROLE_ORDER.index(role)
    if int(role) not in (0, 1, 2):
        raise ValueError("role must be up / lord / down (or its id 0 / 1 / 2)")
    return int(role)


class _Recorder:
    """What every recorder of env's tables shares, whatever its rings hold: the device, the rewards and trained roles in role
    order, the action table, a ring per trained role, the host-known counts, the draws.  A recorder adds its workspace `ws`,
    decode / packed of its entries and around_step(loop, ids, step): what a TrainLoop does with it around step() -> its result."""
    target_network = False     # whether its batches are learnt against a target network (td_step) or alone (mc_step)

    def _setup(self, env, capacity, reward_dict, trained_roles):
        from . import engine as E
        self.device = E._require_gpu(env.device)          # (DdzError without a GPU, as BatchedEnv)
        rd = dict(REWARD_DICT if reward_dict is None else reward_dict)
        self.env, self.T, self.capacity = env, int(env.T), int(capacity)
        if self.capacity <= 0:
            raise ValueError("capacity must be positive")
        self.reward = [float(rd.get(r) or 0.0) for r in ROLE_ORDER]
        self.trained = tuple(bool(x) for x in trained_roles)
        if len(self.trained) != 3:
            raise ValueError("trained_roles: (up, lord, down)")
        self.trained_mask = sum(1 << k for k in range(3) if self.trained[k])
        self._rows = E.action_table(self.device, env.native_joker_kickers)   # [n_actions, 16] int8: id -> count row
        self.known = [0, 0, 0]                                               # host-known lower bounds of the counts (note_counts)

    def _make_rings(self, nbytes, off, fields):
        """one zero-filled ring of nbytes per trained role (None for the others) and, per ring, views of its count and of its
        fields ((name, dtype, elements per entry), ...) at the offsets `off`"""
        cap = self.capacity
        self.rings = [torch.zeros(nbytes, dtype=torch.uint8, device=self.device) if t else None for t in self.trained]

        def views(ring):
            out = {"count": ring[off["count"]: off["count"] + 8].view(torch.int64)}
            for name, dt, width in fields:
                size = torch.empty((), dtype=dt).element_size() * width * cap
                v = ring[off[name]: off[name] + size].view(dt)
                out[name] = v.view(cap, width) if width > 1 else v
            return out
        self.fields = [None if r is None else views(r) for r in self.rings]

    @property
    def ws_bytes_per_table(self):
        return self.ws.numel() / self.T

    def _ring(self, role):
        f = self.fields[_role_id(role)]
        if f is None:
            raise ValueError(f"role {role!r} is not trained: it has no ring")
        return f

    def _index(self, index):
        """ring entries as an int64 [n] device tensor, clamped into the ring"""
        return index.to(device=self.device, dtype=torch.int64).clamp(0, self.capacity - 1).contiguous()

    def count(self, role):
        """transitions ever written into the role's ring: a 0-dim int64 DEVICE tensor (a view: it moves with the recorder)"""
        return self._ring(role)["count"][0]

    def note_counts(self):
        """ONE host sync: reads the three counts into `known` (the host-known minimum sample() checks); returns them"""
        c = torch.stack([f["count"][0] if f is not None else torch.zeros((), dtype=torch.int64, device=self.device)
                         for f in self.fields]).tolist()
        self.known = [int(x) for x in c]
        return self.known

    def draw(self, role, k, at_least=None):
        """int64 [k] device tensor: k entries drawn uniformly (with replacement, as Replay.sample) from the role's
        min(count, capacity) live entries, ON THE DEVICE from the device count: no .item().  Whether the ring holds anything is
        the caller's knowledge: at_least (default: known[role], which note_counts() refreshes at the caller's own sync points)
        is a host-known lower bound of the count, and 0 is an argument error."""
        rid = _role_id(role)
        f = self._ring(role)
        lo = self.known[rid] if at_least is None else int(at_least)
        if lo <= 0:
            raise ValueError("sample() needs a host-known positive lower bound of the ring's count (note_counts(), or at_least=)")
        n = f["count"][0].clamp(min=1, max=self.capacity)
        return (torch.rand(int(k), dtype=torch.float64, device=self.device) * n.double()).long().minimum(n - 1)

    def sample(self, role, k, variant, at_least=None):
        """decode() of draw(role, k, at_least): the batch as faces and thermometers"""
        return self.decode(role, self.draw(role, k, at_least), variant)

    def sample_packed(self, role, k, variant, at_least=None):
        """packed() of draw(role, k, at_least): the batch sample() would decode for the same RNG state, left packed"""
        return self.packed(role, self.draw(role, k, at_least), variant)


class TransitionRecorder(_Recorder):
    """TransitionAssembler + one Replay per role (dqn.py:14) on the device, for env's tables: before() / after() around the
    step of a lock-step iteration (ddz_tr_before / ddz_tr_after: same semantics as before_step / after_step, the `fresh` rule,
    trained_roles, the active mask and replicate_reference_quirk included), nothing on the host, capturable.  A role's ring
    holds `capacity` packed transitions (369 bytes each: any face variant is rebuilt from them, bit for bit, by decode());
    the transition with sequence number s is entry s % capacity, in the order Replay.push would have stored the same calls
    (per call: ascending table).  trained_roles: (up, lord, down); only they get a ring."""
    target_network = True

    def __init__(self, env, capacity, reward_dict=None, trained_roles=(True, True, True), replicate_reference_quirk=False):
        from . import engine as E
        self._setup(env, capacity, reward_dict, trained_roles)
        self.quirk = bool(replicate_reference_quirk)
        self.ws = torch.zeros(E.tr_ws_bytes(self.T), dtype=torch.uint8, device=self.device)
        self._make_rings(E.tr_ring_bytes(self.capacity), E.tr_ring_layout(self.capacity),
                         (("s0", torch.uint8, 176), ("s1", torch.uint8, 176), ("a0", torch.int32, 1), ("a1", torch.int32, 1),
                          ("reward", torch.float32, 1), ("table", torch.int32, 1), ("done", torch.uint8, 1)))

    def before(self, chosen_ids, greedy_ids, active=None):
        """before the step: chosen_ids / greedy_ids int32 [T] canonical ids of what every table plays and of its greedy action
        (a1 of the closing transition), active u8 / bool [T] the tables that move by a network (None: all)"""
        self.env.tr_before(self.ws, self.rings, self.capacity, chosen_ids, greedy_ids, active, self.trained_mask)

    def after(self, done, r):
        """after step(auto_reset=False), before the re-deal: done u8 [T], r i8 [T] as the step returned them"""
        self.env.tr_after(self.ws, self.rings, self.capacity, done, r, self.reward, self.quirk)

    def around_step(self, loop, ids, step):
        """the greedy ids of the network tables gathered into loop._greedy_ids, before(), the step, after()"""
        loop._greedy_ids.copy_(self.env.slab_ids().gather(1, loop.seat.greedy.clamp(min=0).long()[:, None])[:, 0])
        loop._active.copy_(loop.seat.slot >= 0)
        self.before(ids, loop._greedy_ids, loop._active)
        done, r, illegal = step()
        self.after(done, r)
        return done, r, illegal

    def decode(self, role, index, variant):
        """the dict Replay.sample returns -- s0, s1 f32 [n,P,15,4], a0, a1 f32 [n,15,4], reward f32 [n], done bool [n] -- of
        the ring entries index (int64 [n] device tensor; clamped into the ring) in the faces of `variant`.  No host sync."""
        from . import engine as E
        f, index = self._ring(role), self._index(index)
        na = self._rows.shape[0]
        thermo = lambda ids: E.rows_to_onehot(self._rows[ids[index].clamp(0, na - 1).long()])   # noqa: E731
        return {"s0": E.observe_states(f["s0"], index, variant), "a0": thermo(f["a0"]),
                "s1": E.observe_states(f["s1"], index, variant), "a1": thermo(f["a1"]),
                "reward": f["reward"][index], "done": f["done"][index].bool()}

    def packed(self, role, index, variant):
        """the PackedBatch of the ring entries index (int64 [n] device tensor; clamped into the ring as decode does): views of the
        ring, nothing decoded, nothing copied but the index.  No host sync."""
        f = self._ring(role)
        return PackedBatch(f["s0"], f["s1"], f["a0"], f["a1"], f["reward"], f["done"], self._index(index), self._rows, variant)


MAX_DECISIONS_PER_ROLE = 54   # the longest game has 162 plies and the three roles take turns: a role acts at most 162 / 3 times


class _ReturnRings(_Recorder):
    """a recorder whose rings hold return entries (csrc/ddz_returns.h's McRing): mc_step takes its batches"""
    RING_FIELDS = (("s0", torch.uint8, 176), ("a0", torch.int32, 1), ("ret", torch.float32, 1), ("table", torch.int32, 1),
                   ("togo", torch.uint8, 1))

    def decode(self, role, index, variant):
        """{"s0" f32 [n,P,15,4], "a0" f32 [n,15,4], "ret" f32 [n], "togo" u8 [n]} of the ring entries index (int64 [n] device
        tensor; clamped into the ring) in the faces of `variant`.  No host sync."""
        from . import engine as E
        f, index = self._ring(role), self._index(index)
        ids = f["a0"][index].clamp(0, self._rows.shape[0] - 1).long()
        return {"s0": E.observe_states(f["s0"], index, variant), "a0": E.rows_to_onehot(self._rows[ids]),
                "ret": f["ret"][index], "togo": f["togo"][index]}

    def packed(self, role, index, variant):
        """the ReturnBatch of the ring entries index (int64 [n] device tensor; clamped into the ring as decode does): views of the
        ring, nothing decoded, nothing copied but the index.  No host sync."""
        f = self._ring(role)
        return ReturnBatch(f["s0"], f["a0"], f["ret"], f["togo"], self._index(index), self._rows, variant)


class ReturnRecorder(_ReturnRings):
    """ReturnAssembler + one ring per trained role on the device (csrc/ddz_returns.h, return spec v1), for env's tables: before() /
    after() around the step of a lock-step iteration (ddz_mc_before / ddz_mc_after), nothing on the host, capturable.  A ring
    entry is (state row, action id, ret = +/-reward[role] * gamma^togo, table, togo): 189 bytes, about half a transition;
    count / note_counts / draw / sample / sample_packed are every recorder's.  log_cap: log entries per table (1..255);
    None = MAX_DECISIONS_PER_ROLE per trained role, which no game overflows.  The workspace is about 182 bytes per log entry:
    121 MB at 4,096 tables with three trained roles, 1.9 GB at 65,536.  A log that does overflow loses the later decisions
    (workspace counter `lost`), never the discount of the logged ones."""

    def __init__(self, env, capacity, reward_dict=None, trained_roles=(True, True, True), gamma=1.0, log_cap=None):
        from . import engine as E
        self._setup(env, capacity, reward_dict, trained_roles)
        self.gamma = float(gamma)
        self.log_cap = int(log_cap) if log_cap is not None else MAX_DECISIONS_PER_ROLE * max(1, sum(self.trained))
        T, L = self.T, self.log_cap
        self.ws = torch.zeros(E.mc_ws_bytes(T, L), dtype=torch.uint8, device=self.device)
        self._cnt = self.ws[E.mc_ws_layout(T, L)["cnt"]:][:T * 4].view(T, 4)         # {n, c[3]} per table: what clear() zeroes
        self._make_rings(E.mc_ring_bytes(self.capacity), E.mc_ring_layout(self.capacity), self.RING_FIELDS)

    def before(self, chosen_ids, active=None):
        """before the step: chosen_ids int32 [T] canonical ids of what every table plays, active u8 / bool [T] the tables that
        move by a network (None: all)"""
        self.env.mc_before(self.ws, self.log_cap, chosen_ids, active, self.trained_mask)

    def after(self, done, r):
        """after step(auto_reset=False), before the re-deal: done u8 [T], r i8 [T] as the step returned them"""
        self.env.mc_after(self.ws, self.log_cap, self.rings, self.capacity, done, r, self.reward, self.gamma)

    def around_step(self, loop, ids, step):
        """before() on the network tables, the step, after(): no greedy id is gathered, since no a1 is recorded"""
        loop._active.copy_(loop.seat.slot >= 0)
        self.before(ids, loop._active)
        done, r, illegal = step()
        self.after(done, r)
        return done, r, illegal

    def clear(self, mask=None):
        """forget the logs (entries and decision counters; `lost` stays) of the tables of mask (bool / u8 [T]; None: all) that the
        caller re-deals itself before they finish.  No host sync."""
        if mask is None:
            self._cnt.zero_()
        else:
            self._cnt.masked_fill_(mask.to(device=self.device).bool().view(self.T, 1), 0)


class TeacherRecorder(_ReturnRings):
    """TeacherAssembler + one return ring per trained role on the device (csrc/ddz_teach.h, teacher spec v1), for env's tables:
    label(stats) turns the root statistics of one evaluator run (engine.Teacher.evaluate) into ring entries (state row, action
    id, ret = reward[role] * (2 wins / visits - 1), table, togo 0) -- one per move of every selected table whose denominator
    reaches min_den, not only the move that is played.  Nothing on the host, capturable.  The rings are ReturnRecorder's
    (189 bytes an entry), and count / note_counts / draw / sample / sample_packed / decode / packed are its own: mc_step takes
    the batches unchanged.  One call at many tables emits more than a small ring holds (a list has 1 to 497 moves): the ring
    then takes the last `capacity` emits of the call, as both other recorders do."""

    def __init__(self, env, capacity, reward_dict=None, trained_roles=(True, True, True), min_den=1):
        from . import engine as E
        self._setup(env, capacity, reward_dict, trained_roles)
        self.min_den = int(min_den)
        if self.min_den < 1:
            raise ValueError("min_den must be at least 1")
        self.ws = torch.zeros(E.teach_ws_bytes(self.T), dtype=torch.uint8, device=self.device)     # (per-call scratch)
        self._make_rings(E.mc_ring_bytes(self.capacity), E.mc_ring_layout(self.capacity), self.RING_FIELDS)

    def before(self, *args, **kwargs):
        raise TypeError("a TeacherRecorder has no before / after pair around the step: label(stats) is its one call")

    after = before

    def label(self, stats, active=None):
        """on the states the evaluator ran on (before the step): stats = Teacher.evaluate(env)'s TeacherStats, active u8 / bool
        [T] the tables to label (None: all).  Only roles that are trained here AND that the evaluator took are labelled."""
        env = self.env
        env._need_ids("TeacherRecorder.label")
        env.teach(self.ws, self.rings, self.capacity, stats.num, stats.den, stats.den_const, stats.unknown, stats.scale,
                  self.min_den, active, self.trained_mask & stats.roles, self.reward, counts=stats.counts, ids=env.ids,
                  stride=env.slab_stride)

    def around_step(self, loop, ids, step):
        """every label_every-th iteration: evaluate, label() of the network tables, act="teacher": its moves into ids; the step"""
        if loop._it % loop.label_every == 0:
            env = self.env
            loop._active.copy_(loop.seat.slot >= 0)
            stats = loop.teacher.evaluate(env)
            self.label(stats, loop._active)
            if loop.act == "teacher":
                move = loop.teacher.choose(env, stats, out=loop._teacher_ids)
                labelled = loop._active.bool() & loop._trained_of_role[env.role.clamp(max=2).long()] & (env.role <= 2)
                ids.copy_(torch.where(labelled & (move >= 0), move, ids))
        loop._it += 1
        return step()


class TrainLoop(_Loop):
    """One iteration of Game.train's inner loop (game.py:90-167) for T tables, nothing on the host: SeatLoop.act() ->
    recorder.before on the network tables -> step_slab(STEP_IDS, no auto-reset) -> recorder.after -> re-deal of the finished
    tables -> the next lists and faces.  nets / epsilon as SeatLoop's; train_dict {"lord" | "down" | "up": bool} (default:
    every role with a network trains): a network role that does not train plays greedy and records nothing (game.py:95-104).
    capture(n) records n iterations as one graph at the epsilon of the moment and on the derived tables' fixed storage: after
    every learner step call refresh(), then replay (_Loop.capture; without it the graph plays the weights of the last
    refresh).  targets: "td" -- the recorder is a
    TransitionRecorder (one-step targets, td_step) -- or "mc" -- a ReturnRecorder(gamma, log_cap) (the episode's return,
    mc_step): no greedy id is gathered, since no a1 is recorded.
    targets="teacher" (teacher spec v1): the recorder is a TeacherRecorder(min_den) and every label_every-th
    iteration runs SeatLoop.act() -> stats = teacher.evaluate(env) -> rec.label(stats, active = the network tables) -- a target
    for EVERY legal move of every network table of a trained role -- and, with act="teacher" (expert iteration), the ids of
    the labelled tables are replaced by teacher.choose(env, stats) where it is >= 0 (the same statistics: no second search);
    then the step, the re-deal, the lists and the faces as in the other modes.  No before / after pair, no greedy-id gather,
    no target network; batches go to mc_step.  teacher: an engine.Teacher; whether it reads the opponents' hands (hidden) is
    the caller's choice -- open-hand labels are legitimate for training, not for serving.  One label() at many tables emits
    more than a small ring holds; the ring then takes the last `capacity` emits of the call, as both other recorders do.
    capture(n) records the n iterations with their labelling pattern unrolled, so n must be a multiple of label_every."""

    def __init__(self, env, nets, face_variant, capacity=REPLAY_SIZE, epsilon=0.0, train_dict=None, reward_dict=None,
                 replicate_reference_quirk=False, targets="td", gamma=None, log_cap=None, teacher=None, label_every=1, min_den=1,
                 act="net"):
        _teacher_args(targets, teacher, label_every, min_den, act)
        self.teacher, self.label_every, self.act, self._it = teacher, int(label_every), act, 0
        self.seat = SeatLoop(env, nets, face_variant, 0.0, auto_reset=False)
        nr = self.seat.rq.net_of_role
        td = {r: True for r in ROLE_ORDER} if train_dict is None else train_dict
        bad = set(td) - set(ROLE_ORDER)
        if bad:
            raise ValueError(f"unknown role(s) {sorted(bad)} in train_dict")
        self.trained = tuple(nr[k] >= 0 and bool(td.get(r)) for k, r in enumerate(ROLE_ORDER))
        self.env, self.variant, self.targets = env, int(face_variant), targets
        if targets == "teacher":
            self.rec = TeacherRecorder(env, capacity, reward_dict, self.trained, min_den)
            self._trained_of_role = torch.tensor(self.trained, dtype=torch.bool, device=env.device)
            self._teacher_ids = torch.empty(env.T, dtype=torch.int32, device=env.device)
        elif targets == "mc":
            self.rec = ReturnRecorder(env, capacity, reward_dict, self.trained, 1.0 if gamma is None else gamma, log_cap)
        else:
            self.rec = TransitionRecorder(env, capacity, reward_dict, self.trained, replicate_reference_quirk)
            self._greedy_ids = torch.empty(env.T, dtype=torch.int32, device=env.device)
        self.set_epsilon(epsilon)
        self._active = torch.empty(env.T, dtype=torch.uint8, device=env.device)

    def set_epsilon(self, epsilon):
        """exploration of the TRAINED roles (a float, or a dict per role)"""
        eps = dict(epsilon) if isinstance(epsilon, dict) else {r: float(epsilon) for r in ROLE_ORDER}
        self.seat.set_epsilon({r: (e if self.trained[ROLE_ORDER.index(r)] else 0.0) for r, e in eps.items()})

    @property
    def face(self):
        return self.seat.face

    def refresh(self, force=False):
        """SeatLoop.refresh of the acting loop: with a captured graph, the call between a learner step (td_step / mc_step on the
        networks this loop holds) and the next replay -- _Loop.capture; eager step() calls refresh themselves"""
        return self.seat.refresh(force)

    def step(self):
        from .engine import STEP_IDS
        env = self.env
        ids = self.seat.act()
        done, r, illegal = self.rec.around_step(self, ids, lambda: env.step_slab(ids, STEP_IDS, auto_reset=False))
        env.reset(mask=done)
        env.legal_slab()
        env.observe(self.variant, out=self.seat.face)
        return done, r, illegal

    def capture(self, n=1):
        """n iterations as ONE hipGraph, as PolicyLoop.capture (call step() a few times first).  targets="teacher": the
        labelling pattern of the n iterations is part of the graph, so n is a multiple of label_every."""
        if self.targets == "teacher" and int(n) % self.label_every:
            raise ValueError("capture(n) unrolls the labelling pattern: n must be a multiple of label_every")
        return super().capture(n)


def _teacher_args(targets, teacher, label_every, min_den, act):
    """targets and the arguments of targets="teacher" (TrainLoop, train), checked before anything touches the device"""
    from .engine import Teacher
    if targets not in ("td", "mc", "teacher"):
        raise ValueError('targets: "td", "mc" or "teacher"')
    if act not in ("net", "teacher"):
        raise ValueError('act: "net" or "teacher"')
    if targets != "teacher":
        if teacher is not None or act != "net":
            raise ValueError('teacher= and act="teacher" go with targets="teacher"')
        return
    if not isinstance(teacher, Teacher):
        raise ValueError('targets="teacher" needs teacher=engine.Teacher(kind, ...)')
    if int(label_every) < 1 or int(min_den) < 1:
        raise ValueError("label_every and min_den must be at least 1")


def train(face_variant, nets, episodes, train_dict=None, reward_dict=None, tables=4096, seed=0, log_every=100,
          model_every=1000, book=None, model_dir=None, win_dir=None, device="cuda:0", check_every=8, capacity=REPLAY_SIZE,
          begin=None, log=None, fused=False, batch_size=BATCH_SIZE, targets="td", gamma=None, teacher=None, label_every=1,
          min_den=1, act="net"):
    """Game.train (game.py:183-238) on the batched engine, the counterpart of compete(): nets {"lord" | "down" | "up": QNet |
    None (the rule agent)}, train_dict which network roles keep training (default: all of them), reward_dict as REWARD_DICT.
    Lock-step iterations of TrainLoop over `tables` tables until `episodes` episodes have finished; every iteration each
    trained role whose ring holds batch_size entries (default BATCH_SIZE, the reference's 256) takes one td_step(fused=fused) on
    a batch of that size sampled on the device (dqn.py:24-48: Adam 1e-4, a target network per role); fused="packed" leaves the
    batch packed (sample_packed: the stage's kernels read the ring, no face is built).  The host looks at the
    device every `check_every` iterations only (env.stats() and the ring counts: the one sync): there it moves epsilon (epsilon_schedule of the episodes so far), copies policy -> target
    every UPDATE_TARGET_EVERY episodes (dqn.py:73-80), writes the log line every log_every and the checkpoints
    <begin>_<role>_<episode> every model_every episodes (game.py:209-232; metrics.checkpoint_name / save_state_dict under
    model_dir, the win rates under win_dir) -- `episode` being the multiple of the interval that was crossed, since the tables
    finish episodes in bulk.  The policy networks learn in train() mode (dropout on, dqn.py:41), the targets are evaluated
    without dropout.  Returns {"lord", "down", "up": wins, "episodes", "iterations", "loss": {role: last loss | None},
    "checkpoints": [paths]}.  targets="mc": the roles learn from Monte-Carlo return targets instead (ReturnRecorder, one mc_step
    per ready role and iteration, gamma None = 1.0 = Deep Monte Carlo): no target network exists and none is copied; everything
    else, the returned keys included, is the same.  targets="teacher": the roles learn from the root statistics of a search
    (TrainLoop(targets="teacher", teacher=engine.Teacher(...), label_every, min_den, act): a target for every legal move of the
    labelled tables; act="teacher" also plays the teacher's move there), again one mc_step per ready role and iteration and no
    target network; the same returned keys."""
    import copy
    import time
    from . import metrics
    from .engine import BatchedEnv
    batch_size = int(batch_size)
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    if isinstance(fused, str) and fused not in ("stage", "packed"):
        raise ValueError('fused: False, True, "stage" or "packed"')
    _teacher_args(targets, teacher, label_every, min_den, act)
    nets = {r: v for r, v in nets.items()}
    for r, v in nets.items():
        if v is not None:
            nets[r] = v.to(device)
    env = BatchedEnv(int(tables), seed=int(seed), device=device)
    env.reset()
    env.legal_slab()
    loop = TrainLoop(env, nets, face_variant, capacity=capacity, epsilon=epsilon_schedule(0), train_dict=train_dict,
                     reward_dict=reward_dict, targets=targets, gamma=gamma, teacher=teacher, label_every=label_every,
                     min_den=min_den, act=act)
    mc = not loop.rec.target_network                                 # (return rings and mc_step, no target network)
    roles = [r for k, r in enumerate(ROLE_ORDER) if loop.trained[k]]
    if not roles:
        env.close()
        raise ValueError("No agent need train.")                     # game.py:184-188
    policy = {r: nets[r] for r in roles}
    target, opt = {}, {}
    for r in roles:                                                  # (roles that share a network object share the learner)
        same = [o for o in target if policy[o] is policy[r]]
        target[r] = None if mc else target[same[0]] if same else copy.deepcopy(policy[r]).eval()
        opt[r] = opt[same[0]] if same else torch.optim.Adam(policy[r].parameters(), LEARNING_RATE)
        policy[r].train()
    book = book if book is not None else metrics.WinRateBook(begin)
    begin = begin or book.begin
    s0 = env.stats()
    book.update(s0)
    loss = {r: None for r in roles}
    paths, it, eps_done, eps_logged, t_log = [], 0, 0, 0, time.time()
    ready = {r: False for r in roles}
    while True:
        for _ in range(int(check_every)):
            loop.step()
            for r in roles:
                if ready[r]:
                    packed = isinstance(fused, str) and fused == "packed"
                    batch = (loop.rec.sample_packed if packed else loop.rec.sample)(r, batch_size, face_variant)
                    if mc:
                        loss[r] = mc_step(policy[r], opt[r], batch, fused=False if packed else fused)
                    else:
                        loss[r] = td_step(policy[r], target[r], opt[r], batch, GAMMA, fused=fused)
        it += int(check_every)
        s1 = env.stats()                                             # the host sync of the interval
        known = loop.rec.note_counts()
        for r in roles:
            ready[r] = known[ROLE_ORDER.index(r)] >= batch_size
        book.update(s1)
        prev, eps_done = eps_done, s1["episodes"] - s0["episodes"]
        for r in roles:
            if loss[r] is not None:
                book.add_loss(r, float(loss[r]))
        if not mc and eps_done // UPDATE_TARGET_EVERY > prev // UPDATE_TARGET_EVERY:
            for r in roles:
                target[r].load_state_dict(policy[r].state_dict())
        if eps_done // int(log_every) > prev // int(log_every):
            msg = book.log_message(eps_done - eps_logged, time.time() - t_log)
            eps_logged = eps_done
            if log is not None:
                log(msg)
            book.close_interval(win_dir)
            t_log = time.time()
        if model_dir is not None and eps_done // int(model_every) > prev // int(model_every):
            mark = eps_done // int(model_every) * int(model_every)
            for r in metrics.ROLES:
                if nets.get(r) is not None:
                    paths.append(metrics.save_state_dict(nets[r], model_dir, metrics.checkpoint_name(begin, r, mark)))
        if eps_done >= int(episodes):
            break
        loop.set_epsilon(epsilon_schedule(eps_done))
    for r in roles:
        policy[r].eval()
    env.close()
    out = {"lord": s1["lord_wins"] - s0["lord_wins"], "down": s1["down_wins"] - s0["down_wins"],
           "up": s1["up_wins"] - s0["up_wins"], "episodes": eps_done, "iterations": it,
           "loss": {r: (None if v is None else float(v)) for r, v in loss.items()}, "checkpoints": paths}
    return out
