"""BatchedEnv: T independent Doudizhu tables advanced in lock-step on one MI355X.

Host-side mirror of the reference's env adapter (envi.py:16-161) re-cut as batched verbs.
PyTorch owns every buffer (state, scratch, CSR list, outputs); the HIP library
(csrc/, C ABI include/ddz_env.h) is handed raw device pointers and the current stream.
Nothing here computes game logic on the CPU, and nothing falls back to it.
"""
import collections
import ctypes as C

import torch

from . import _lib
from ._lib import DdzError, check

ROW = 16
NFIELDS = 11
TRAJ_BYTES = 32
NUM_ACTIONS = 13527
STEP_RANDOM, STEP_CHOICE, STEP_ROWS, STEP_IDS = 0, 1, 2, 3
FACE_PLANES = (4, 7, 9, 6)  # Env, EnvComplicated, EnvCooperation, EnvCooperationSimplify
F_HAND0, F_HIST0, F_RECENT0, F_TAKEN, F_META = 0, 3, 6, 9, 10
# bytes of the meta row (include/ddz_env.h): role to move, done, winner's role (META_NO_WINNER: none), dealt
META_ROLE, META_DONE, META_WINNER, META_DEALT = 0, 1, 2, 6
META_NO_WINNER = 0xFF
# the bits of the status word (include/ddz_env.h, DDZ_ST_*)
(STATUS_MISMATCH, STATUS_CAPACITY, STATUS_BAD_LAST, STATUS_AUTO_WAIT, STATUS_AUTO_DEPTH, STATUS_Q_NO_ROW, STATUS_DOMAIN,
 STATUS_CFR_CAPACITY, STATUS_SOLVE_DEPTH) = (1 << k for k in range(9))
# a 20-card hand never has more than this many legal moves (tests/test_rules_bounds.py);
# the default row capacity is T * MAX_LEGAL_PER_TABLE so the CSR list cannot overflow.
MAX_LEGAL_PER_TABLE = 512
CSR_STAGING_BYTES = 16 << 30  # default staging budget of rollout_random_csr (slabs of a batch of iterations)


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise DdzError("no MI355X visible (torch.cuda.is_available() is False): the engine has "
                       "no CPU fallback")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DdzError(f"device must be a cuda (ROCm) device, got {dev}")
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _chk(x, name, dtype, dev, shape=None, numel=None, at_least=None, where="on the same device", why="", pinned=False,
         none_ok=False):
    """The one test of a caller's buffer before its address reaches the library: `x` has `dtype`, lives on `dev` (pinned: or in
    pinned host memory, which the device reads and writes), is contiguous, and has exactly `shape`, exactly `numel` elements or
    `at_least` that many (none of the three: a byte workspace whose size travels with its address, for the library to test)
    -> x, or ValueError.  none_ok: None passes as None.  why: what the message cannot show otherwise."""
    if x is None and none_ok:
        return None
    if (x is None or x.dtype != dtype or not x.is_contiguous()
            or (x.device != dev and not (pinned and x.device.type == "cpu" and x.is_pinned()))
            or (shape is not None and tuple(x.shape) != tuple(shape)) or (numel is not None and x.numel() != numel)
            or (at_least is not None and x.numel() < at_least)):
        size = list(shape) if shape is not None else [numel] if numel is not None else f"[>= {at_least or 0}]"
        raise ValueError(f"{name} must be a contiguous {dtype} {size} tensor {where}{why}")
    return x


def _roles_mask(roles, hidden=True, name="roles"):
    roles = int(roles)
    if not 0 <= roles <= 7:
        raise ValueError(f"{name} is a mask of the role bits 0 (up), 1 (lord), 2 (down)")
    if not hidden and roles != 0b111:
        raise ValueError(f"{name} needs hidden=True (the open form takes every running table)")
    return roles


def _salt(salt):
    return int(salt) & 0xFFFFFFFF


def _reward3(reward):
    if len(reward) != 3:
        raise ValueError("reward: three floats in role order up, lord, down")
    return (C.c_float * 3)(*[float(x) for x in reward])


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
    """the caller's current HIP stream on `device` as a raw pointer (every launch of the library goes there)"""
    if _raw_stream is not None and device.index is not None:
        return C.c_void_p(_raw_stream(device.index))      # (~0.3 us; torch.cuda.current_stream() builds a Stream object: ~4 us)
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class BatchedEnv:
    """T tables; table t is global table `table_id_base + t` (keys the RNG)."""

    def __init__(self, n_tables, seed=0, device="cuda:0", table_id_base=0, row_capacity=None,
                 want_ids=True, native_joker_kickers=False, host_mirror=False, _debug_tables_per_wave=None,
                 _debug_slab_coop=None, _debug_slab_work_list=None, _debug_auto_teams=None):
        # native_joker_kickers: the optional rule set with the 24 extra rows the reference's native
        # get_moves is known to emit (server/mcts/get_moves.py:22-34); default off = exactly card.py
        self.native_joker_kickers = bool(native_joker_kickers)
        self.lib = _lib.lib(jk=self.native_joker_kickers)
        self.device = _require_gpu(device)
        self.T = int(n_tables)
        if self.T <= 0:
            raise ValueError("n_tables must be positive")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.table_id_base = int(table_id_base)
        self.cap = int(row_capacity) if row_capacity is not None else self.T * MAX_LEGAL_PER_TABLE
        if self.cap > 0x7FFFFFFF:
            raise ValueError("row capacity must be indexable with int32")
        d = self.device
        # host_mirror (the N = 1 `Env` view): the state rows and the list sizes live in PINNED HOST memory -- the kernels
        # read and write them over the host link (a few hundred bytes per launch), the host reads them after one stream
        # synchronisation with no copy at all.  Latency trade for one table; never for a batch.
        self.host_mirror = bool(host_mirror)
        if self.host_mirror:
            self.state = torch.zeros(self.lib.ddz_state_bytes(self.T), dtype=torch.uint8).pin_memory()
        else:
            self.state = torch.zeros(self.lib.ddz_state_bytes(self.T), dtype=torch.uint8, device=d)
        self.scratch = torch.zeros(self.lib.ddz_scratch_bytes(self.T), dtype=torch.uint8, device=d)
        self.offsets = torch.zeros(self.T + 1, dtype=torch.int32, device=d)
        self.rows = torch.zeros((self.cap, ROW), dtype=torch.int8, device=d)
        self.ids = torch.zeros(self.cap, dtype=torch.int32, device=d) if want_ids else None
        if self.host_mirror:
            self.counts = torch.zeros(self.T, dtype=torch.int32).pin_memory()
        else:
            self.counts = torch.zeros(self.T, dtype=torch.int32, device=d)  # slab layout: list sizes
        self.done = torch.zeros(self.T, dtype=torch.uint8, device=d)
        self.reward = torch.zeros(self.T, dtype=torch.int8, device=d)
        self.illegal = torch.zeros(self.T, dtype=torch.uint8, device=d)
        self._stats = torch.zeros(8, dtype=torch.int64, device=d)
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False
        # raw pointers of the persistent buffers, converted once (the host side of a call is ~10 us of ctypes work)
        self._pp = {k: _p(getattr(self, k)) for k in ("counts", "rows", "ids", "done", "reward", "illegal", "offsets")}
        h = C.c_void_p()
        check(self.lib.ddz_create(C.byref(h), self.T, self.seed, self.table_id_base, d.index,
                                  _p(self.state), self.state.numel(), _p(self.scratch),
                                  self.scratch.numel()))
        self._h = h
        if _debug_tables_per_wave is not None or _debug_slab_coop is not None or _debug_slab_work_list is not None:
            # test hook: results never depend on the launch geometry
            check(self.lib.ddz_debug_set_geometry(h, int(_debug_tables_per_wave or 0),
                                                  -1 if _debug_slab_coop is None else int(_debug_slab_coop),
                                                  -1 if _debug_slab_work_list is None else int(bool(_debug_slab_work_list))))
        if _debug_auto_teams is not None:
            # test hook: auto_choose's wavefronts without tables help their workgroup's running searches (default) or not
            check(self.lib.ddz_debug_set_auto_teams(h, int(_debug_auto_teams)))   # 0 off, 1 default, 2 teams without team-first

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ddz_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- views of the packed state ([T,16] int8/uint8, zero-copy) ----
    def field(self, f):
        return self.state.view(self.T, NFIELDS, ROW)[:, f]

    @property
    def role(self):
        return self.field(F_META)[:, 0]

    def hands(self):
        return self.state.view(self.T, NFIELDS, ROW)[:, F_HAND0:F_HAND0 + 3]

    # ---- a caller's buffers: every one passes _chk before its address reaches the library ----
    def _arg(self, x, name, dtype, **size):
        return _chk(x, name, dtype, self.device, where="on the env's device", **size)

    def _traj(self, traj, n_iters=1):
        return self._arg(traj, "traj", torch.uint8, numel=n_iters * self.T * TRAJ_BYTES, none_ok=True)

    def _totals(self, totals):
        return self._arg(totals, "totals", torch.int64, at_least=4, none_ok=True)

    def _ids_out(self, out):
        """int32 [T] to write ids / list indices into, made if None (a host_mirror env also takes pinned host memory)"""
        if out is None:
            return torch.empty(self.T, dtype=torch.int32, device=self.device)
        return self._arg(out, "out", torch.int32, numel=self.T, pinned=self.host_mirror)

    def _slab_counts(self, x, name):
        """int32 [T * stride] of a number per list entry, made if None"""
        if x is None:
            return torch.empty(self.T * self.slab_stride, dtype=torch.int32, device=self.device)
        return self._arg(x, name, torch.int32, numel=self.T * self.slab_stride)

    def _slab_lists(self, what=None):
        """the slab lists are those of the current state: entry [t, j] of a verb's result is read against them.  what
        ("playouts need"): the verb needs the full stride, and says so"""
        if what and self.slab_stride < MAX_LEGAL_PER_TABLE:
            raise ValueError(f"{what} row_capacity >= {MAX_LEGAL_PER_TABLE} * n_tables")
        if not self._slab_fresh:
            self.legal_slab()

    def _workspace(self, attr, need):
        """a byte buffer of at least `need` bytes cached on the env as `attr`: it only grows"""
        if need < 0:
            raise ValueError("no workspace size for these arguments")
        work = getattr(self, attr, None)
        if work is None or work.numel() < need:
            work = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            setattr(self, attr, work)
        return work

    def _need_ids(self, what):
        if self.ids is None:
            raise ValueError(f"{what} needs the action ids of the lists (want_ids=True)")

    # ---- the statistic buffers an env keeps for the choose verbs, PlayoutLeaf and Teacher, by what they hold: the one place they
    # live.  verb: (what its buffers hold, how it takes them back); search() and ismcts() write the same pair
    _KEPT = {"playout": ("playout wins", lambda k: {"wins": k[0]}),
             "search": ("search visits, wins", lambda k: {"visits": k[0], "wins": k[1]}),
             "ismcts": ("search visits, wins", lambda k: {"visits": k[0], "wins": k[1]}),
             "solve": ("solve out", lambda k: {"out": k}),
             "cfr": ("cfr out", lambda k: {"out": k})}

    def _kept(self, key, make=None):
        """the buffers kept under `key` (a tuple of flat tensors), or None; make: what makes them where there are none"""
        kept = self.__dict__.setdefault("_kept_stats", {})
        if make is not None and key not in kept:
            kept[key] = make()
        return kept.get(key)

    def _run_kept(self, verb, *args, **kw):
        """the evaluator `verb` writing into the buffers kept for it (the first run makes them) -> its statistics, each flat"""
        key, give = self._KEPT[verb]
        kept = self.__dict__.setdefault("_kept_stats", {}).get(key)
        if kept is not None:                # (the verb hands back views of what it is given: the kept tuple stays the result)
            getattr(self, verb)(*args, **kw, **give(kept))
            return kept
        got = getattr(self, verb)(*args, **kw)
        self._kept_stats[key] = kept = tuple(x.view(-1) for x in (got if isinstance(got, tuple) else (got,)))
        return kept

    # ---- the choose rules: statistics of the current slab lists -> one canonical action id per table, in `out` ----
    def _choose_out(self, what, out):
        """the int32 [T] a choose verb writes, checked before anything runs"""
        self._need_ids(what)
        return self._ids_out(out)

    def _choose_wins(self, wins, out):
        """the first maximum of wins (ddz_playout_choose)"""
        check(self.lib.ddz_playout_choose(self._h, self._pp["counts"], self._pp["ids"], self.slab_stride, _p(wins), _p(out),
                                          _stream(self.device)))
        return out

    def _choose_ratio(self, visits, wins, out):
        """the first maximum of wins / visits over the visited moves, compared exactly (ddz_search_choose)"""
        check(self.lib.ddz_search_choose(self._h, self._pp["counts"], self._pp["ids"], self.slab_stride, _p(visits), _p(wins), _p(out),
                                         _stream(self.device)))
        return out

    def _choose_solved(self, worlds, wins, unknown, out, value):
        """the solver's rule and the chosen move's `value` (ddz_solve_choose)"""
        check(self.lib.ddz_solve_choose(self._h, self._pp["counts"], self._pp["ids"], self.slab_stride, worlds, _p(wins), _p(unknown),
                                        _p(out), _p(value), _stream(self.device)))
        return out

    def _choose_sigma(self, n, ids, sigma, salt, greedy, out):
        """cfr's rule: sampled from sigma, or its first maximum (ddz_cfr_choose)"""
        check(self.lib.ddz_cfr_choose(self._h, _p(n), _p(ids), _p(sigma), _salt(salt), int(bool(greedy)), _p(out), _stream(self.device)))
        return out

    def _q_slab_arg(self, q):
        if q.dtype != torch.float32 or q.device != self.device or not q.is_contiguous():
            q = q.to(device=self.device, dtype=torch.float32).contiguous()
        if q.numel() != self.T * self.slab_stride:
            raise ValueError("q must be [T, stride]")
        return q

    def _face_out(self, out, variant, name="out"):
        """float32 [T,P,15,4] for the faces of `variant`, made if None"""
        P = FACE_PLANES[variant]
        if out is None:
            return torch.empty((self.T, P, 15, 4), dtype=torch.float32, device=self.device)
        return self._arg(out, name, torch.float32, numel=self.T * P * 60, why=f" ([T,{P},15,4])")

    def _shared_rows_out(self, n_nets, ws, row_capacity, rows, rep, seg):
        """what a shared-row finder writes, n_nets partitions of row_capacity rows"""
        self._arg(ws, "ws", torch.uint8)
        self._arg(rows, "rows", torch.int32, shape=(self.T, 16))
        self._arg(rep, "rep", torch.int32, at_least=n_nets * int(row_capacity))
        self._arg(seg, "seg", torch.int32, at_least=40 * n_nets)

    def _cfr_tensors(self, t, name):
        """the (n, ids, sigma, value) of a cfr() call, handed back as `name`; value: checked by cfr(), which alone writes it"""
        n, ids, sigma, value = t
        why = f" (of {name}: the (n, ids, sigma, value) of an earlier cfr() call)"
        self._arg(n, "n", torch.int32, numel=self.T, why=why)
        self._arg(ids, "ids", torch.int32, numel=self.T * self.CFR_STRIDE, why=why)
        self._arg(sigma, "sigma", torch.float64, numel=self.T * self.CFR_STRIDE, why=why)
        return n, ids, sigma, value

    # ---- verbs ----
    def reset(self, mask=None):
        """Env.reset() + prepare() (envi.py:30-36, game.py:170-171) for masked tables."""
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if mask.numel() != self.T:
                raise ValueError("mask must have one byte per table")
        check(self.lib.ddz_reset(self._h, _p(mask), _stream(self.device)))
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False

    def legal(self):
        """CSR legal-move lists of all tables (envi.py:98-116 valid_actions(tensor=False)).
        Returns (offsets[T+1] i32, rows[cap,16] i8, ids[cap] i32 | None); only the first
        offsets[T] rows are meaningful.  No host sync."""
        check(self.lib.ddz_legal(self._h, _p(self.offsets), _p(self.rows), _p(self.ids), self.cap,
                                 _stream(self.device)))
        self._legal_fresh, self._slab_fresh, self._csr_fresh = True, False, False  # legal() packed CSR rows into the row buffer
        return self.offsets, self.rows, self.ids

    def _need_legal(self):
        if not self._legal_fresh:
            self.legal()

    def step(self, sel=None, mode=STEP_CHOICE, auto_reset=True, traj=None):
        """Apply one action per table (envi.py:63-70 step_manual / :79-85 step_random).
        mode STEP_RANDOM: sel ignored; STEP_CHOICE: sel int32[T] index into each legal
        segment; STEP_ROWS: sel int8[T,16] count rows; STEP_IDS: sel int32[T] canonical action ids
        (-1 = engine RNG for that table), what auto_choose() returns.  Returns (done u8[T], r i8[T],
        illegal u8[T]); r = -1 lord won, +1 farmers won (rule_play.py:14)."""
        self._need_legal()
        self._traj(traj)
        if mode in (STEP_CHOICE, STEP_IDS):
            sel = sel.to(device=self.device, dtype=torch.int32).contiguous()
            if sel.numel() != self.T:
                raise ValueError("choice / ids must have one entry per table")
        elif mode == STEP_ROWS:
            sel = sel.to(device=self.device, dtype=torch.int8).contiguous()
            if tuple(sel.shape) != (self.T, ROW):
                raise ValueError("rows must be [T,16] int8")
        elif mode != STEP_RANDOM:
            raise ValueError("bad step mode")
        check(self.lib.ddz_step(self._h, mode, _p(sel) if mode != STEP_RANDOM else None,
                                _p(self.offsets), _p(self.rows), int(bool(auto_reset)),
                                _p(self.done), _p(self.reward), _p(self.illegal), _p(traj),
                                _stream(self.device)))
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False
        return self.done, self.reward, self.illegal

    def step_onehot(self, actions, auto_reset=True, traj=None):
        """step_manual with the reference's action encoding (envi.py:63-70): actions f32/int
        [T,15,4] thermometers (what valid_actions(tensor=True) rows look like); decoded on the
        device by the row sum of onehot2arr (envi.py:148-157)."""
        a = actions.to(self.device)
        if tuple(a.shape) != (self.T, 15, 4):
            raise ValueError("actions must be [T,15,4]")
        rows = torch.zeros((self.T, ROW), dtype=torch.int8, device=self.device)
        rows[:, :15] = a.sum(dim=2).round().to(torch.int8)
        return self.step(rows, STEP_ROWS, auto_reset, traj)

    def step_random(self, auto_reset=True, traj=None):
        return self.step(None, STEP_RANDOM, auto_reset, traj)

    # ---- rule-based opponent (envi.py:72-77 step_auto) ----
    def auto_choose(self, auto_roles=0b101, out=None, stats=None, _debug_kernel=None):
        """The rule agent's move (RuleBasedModel.choose, rule_based/utils/rule_based_model.py:43-101) for every table
        whose actor's role bit is set in auto_roles (bit 0 up, 1 lord, 2 down; default: both farmers): int32[T]
        canonical action ids, -1 for the other tables (-2 = DDZ_AUTO_INVALID: a state the agent cannot decide, which
        DDZ_STEP_IDS flags illegal -- never a silent random move).  stats: optional int64 [T,2] {combinations, search nodes} of the full
        enumeration; without it the kernel runs an exact branch and bound (same ids, ~3x faster)."""
        out = self._ids_out(out)
        self._arg(stats, "stats", torch.int64, numel=2 * self.T, none_ok=True)
        if _debug_kernel is not None:  # test hook: 1 = the sequential cross-check kernel, 2 = the product kernel
            check(self.lib.ddz_debug_auto_choose_state(self._h, int(_debug_kernel), int(auto_roles), _p(out), _p(stats),
                                                       _stream(self.device)))
        else:
            check(self.lib.ddz_auto_choose_state(self._h, int(auto_roles), _p(out), _p(stats), _stream(self.device)))
        return out

    def step_auto(self, auto_roles=0b101, ids=None, auto_reset=True, traj=None, slab=False):
        """One lock-step iteration in which the roles of auto_roles are played by the rule agent (Env.step_auto,
        envi.py:72-77) and every other table moves by `ids` (int32[T] canonical action ids of a policy; None or -1 =
        engine RNG, i.e. step_random).  game.py:106: `_, done, _ = self.env.step_auto()` for a role without a network."""
        sel = self.auto_choose(auto_roles)
        if ids is not None:
            sel = torch.where(sel >= 0, sel, ids.to(device=self.device, dtype=torch.int32))
        return (self.step_slab if slab else self.step)(sel, STEP_IDS, auto_reset, traj)

    def observe(self, variant=3, out=None):
        """`face` of every table: f32 [T,P,15,4] (envi.py:87-96,165-217)."""
        out = self._face_out(out, variant)
        check(self.lib.ddz_observe(self._h, int(variant), _p(out), _stream(self.device)))
        return out

    # ---- the transition recorder (csrc/ddz_replay.h; dqn_glue.TransitionRecorder) ----
    def _rings_arg(self, rings, ring_bytes, capacity, need=0):
        """the three rings of a recorder verb, one uint8 tensor of ring_bytes(capacity) bytes (or None) per role; bit k of `need`:
        role k must have one -> (their addresses, the bytes of one)"""
        if len(rings) != 3:
            raise ValueError("rings: one tensor (or None) per role, in role order up, lord, down")
        nbytes, why = ring_bytes(capacity), f" ({ring_bytes.__name__}(capacity) bytes)"
        for k, ring in enumerate(rings):
            if ring is not None:
                self._arg(ring, f"rings[{k}]", torch.uint8, numel=nbytes, why=why)
            elif (need >> k) & 1:
                raise ValueError("a trained role needs a ring")
        return (C.c_void_p * 3)(*[None if r is None else r.data_ptr() for r in rings]), nbytes

    def _u8_arg(self, x, name, none_ok=False):
        """uint8 [T]; a bool [T] is converted; none_ok (`active`: None = all tables): None passes as None"""
        return self._arg(x.to(torch.uint8) if x is not None and x.dtype == torch.bool else x, name, torch.uint8, numel=self.T,
                         none_ok=none_ok)

    def tr_before(self, ws, rings, capacity, chosen, greedy, active=None, trained_roles=0b111):
        """ddz_tr_before: close and open transitions on the CURRENT states (call it before the step).  chosen / greedy int32 [T]
        canonical action ids, active u8 / bool [T] or None (all tables), trained_roles: bit r = role r.  No host sync."""
        trained_roles = _roles_mask(trained_roles, name="trained_roles")
        self._arg(ws, "ws", torch.uint8, at_least=tr_ws_bytes(self.T), why=" (tr_ws_bytes(T) bytes)")
        ptrs, nbytes = self._rings_arg(rings, tr_ring_bytes, capacity, trained_roles)
        self._arg(chosen, "chosen", torch.int32, numel=self.T)
        self._arg(greedy, "greedy", torch.int32, numel=self.T)
        active = self._u8_arg(active, "active", none_ok=True)
        check(self.lib.ddz_tr_before(self._h, _p(ws), ws.numel(), ptrs, nbytes, int(capacity), _p(chosen), _p(greedy), _p(active),
                                     trained_roles, _stream(self.device)))

    def tr_after(self, ws, rings, capacity, done, r, reward, replicate_reference_quirk=False):
        """ddz_tr_after: the terminal transitions of the finished tables (call it after step(auto_reset=False), before the
        re-deal).  done u8 [T], r i8 [T] as the step wrote them, reward: three floats in role order up, lord, down."""
        self._arg(ws, "ws", torch.uint8, at_least=tr_ws_bytes(self.T), why=" (tr_ws_bytes(T) bytes)")
        ptrs, nbytes = self._rings_arg(rings, tr_ring_bytes, capacity)
        done, r = self._u8_arg(done, "done"), self._arg(r, "r", torch.int8, numel=self.T)
        check(self.lib.ddz_tr_after(self._h, _p(ws), ws.numel(), ptrs, nbytes, int(capacity), _p(done), _p(r),
                                    _reward3(reward), int(bool(replicate_reference_quirk)), _stream(self.device)))

    # ---- Monte-Carlo return targets (csrc/ddz_returns.h; dqn_glue.ReturnRecorder) ----
    def mc_before(self, ws, log_cap, chosen, active=None, trained_roles=0b111):
        """ddz_mc_before: the episode log of every active table whose actor is a trained role takes (state row now, chosen[t])
        (call it before the step).  chosen int32 [T] canonical action ids, active u8 / bool [T] or None (all tables),
        trained_roles: bit r = role r.  No host sync."""
        trained_roles = _roles_mask(trained_roles, name="trained_roles")
        self._arg(ws, "ws", torch.uint8, at_least=mc_ws_bytes(self.T, log_cap), why=" (mc_ws_bytes(T, log_cap) bytes)")
        self._arg(chosen, "chosen", torch.int32, numel=self.T)
        active = self._u8_arg(active, "active", none_ok=True)
        check(self.lib.ddz_mc_before(self._h, _p(ws), ws.numel(), int(log_cap), _p(chosen), _p(active), trained_roles,
                                     _stream(self.device)))

    def mc_after(self, ws, log_cap, rings, capacity, done, r, reward, gamma=1.0):
        """ddz_mc_after: the logs of the finished tables become ring entries (s0, a0, ret = +/-reward[role] * gamma^togo, table,
        togo) and empty (call it after step(auto_reset=False), before the re-deal).  rings: one uint8 tensor of
        mc_ring_bytes(capacity) bytes (or None: that role's entries are dropped) per role; done u8 [T], r i8 [T] as the step wrote
        them, reward: three floats in role order up, lord, down."""
        self._arg(ws, "ws", torch.uint8, at_least=mc_ws_bytes(self.T, log_cap), why=" (mc_ws_bytes(T, log_cap) bytes)")
        ptrs, nbytes = (None, 0) if rings is None else self._rings_arg(rings, mc_ring_bytes, capacity)   # (None: the library's error)
        done, r = self._u8_arg(done, "done"), self._arg(r, "r", torch.int8, numel=self.T)
        check(self.lib.ddz_mc_after(self._h, _p(ws), ws.numel(), int(log_cap), ptrs, nbytes, int(capacity), _p(done), _p(r),
                                    _reward3(reward), float(gamma), _stream(self.device)))

    # ---- teacher targets (csrc/ddz_teach.h; dqn_glue.TeacherRecorder, Teacher below) ----
    TEACH_REWARD = (50.0, 100.0, 50.0)       # dqn_glue.REWARD_DICT in role order

    def teach(self, ws, rings, capacity, num, den=None, den_const=None, unknown=None, scale=1, min_den=1, active=None,
              trained_roles=0b111, reward=TEACH_REWARD, counts=None, ids=None, stride=None):
        """ddz_teach (teacher spec v1): every move j of every selected table's list whose denominator d = (den[t, j]
        or den_const) - unknown[t, j] is at least min_den becomes an entry (state row, ids[t, j], ret = reward[role] *
        (2 num[t, j] - d scale) / (d scale), table, togo 0) of the role's return ring -- the rings of mc_after, which
        ReturnRecorder.sample / mc_step consume.  num / den / unknown int32 [T * stride] (den None: den_const for every entry;
        unknown None: nothing subtracted), scale 1 or GUIDED_ONE for guided wins, active u8 / bool [T] or None (all tables),
        trained_roles: bit r = role r.  ws: uint8, teach_ws_bytes(T) bytes of per-call scratch (nothing to initialise).
        counts / ids / stride: the lists the statistics belong to (default: the env's own slab lists, which the caller made
        current; stride goes with them).  Three launches on the current stream, nothing on the host: capturable."""
        trained_roles = _roles_mask(trained_roles, name="trained_roles")
        if (counts is None) != (ids is None) or (counts is None and stride is not None):
            raise ValueError("counts, ids and stride describe one list layout: give all of them or none")
        if counts is None:
            self._need_ids("teach")
            counts, ids, stride = self.counts, self.ids, self.slab_stride
        stride = self.slab_stride if stride is None else int(stride)
        if stride < 1 or self.T * stride > 0x7FFFFFFF:
            raise ValueError("stride must be at least 1 and T * stride below 2^31")
        scale, min_den = int(scale), int(min_den)
        if not 1 <= scale <= 1024:
            raise ValueError("scale must be in [1, 1024]")
        if not 1 <= min_den <= 0x7FFFFFFF:
            raise ValueError("min_den must be in [1, 2^31)")
        if den is None and (den_const is None or not 1 <= int(den_const) <= 0x7FFFFFFF):
            raise ValueError("den_const must be in [1, 2^31) where no den array is given")
        n = self.T * stride
        self._arg(counts, "counts", torch.int32, numel=self.T, pinned=self.host_mirror)
        self._arg(ids, "ids", torch.int32, at_least=n)
        self._arg(num, "num", torch.int32, numel=n, why=" ([T * stride])")
        self._arg(den, "den", torch.int32, numel=n, why=" ([T * stride])", none_ok=True)
        self._arg(unknown, "unknown", torch.int32, numel=n, why=" ([T * stride])", none_ok=True)
        self._arg(ws, "ws", torch.uint8, at_least=teach_ws_bytes(self.T), why=" (teach_ws_bytes(T) bytes)")
        ptrs, nbytes = self._rings_arg(rings, mc_ring_bytes, capacity)
        active = self._u8_arg(active, "active", none_ok=True)
        check(self.lib.ddz_teach(self._h, _p(counts), _p(ids), stride, _p(num), _p(den), int(den_const or 0), _p(unknown), scale,
                                 min_den, _p(active), trained_roles, _p(ws), ws.numel(), ptrs, nbytes, int(capacity),
                                 _reward3(reward), _stream(self.device)))

    def select(self, q, epsilon=0.0, out=None):
        """greedy / epsilon-greedy choice per table from per-row values q (f32, CSR order of
        the current legal list; dqn.py:50-71).  Returns int32[T] indices for step(STEP_CHOICE)."""
        if not self._csr_fresh:   # after slab_to_csr() the offsets already describe the current lists: no ddz_legal
            self._need_legal()
        out = self._ids_out(out)
        q = q.to(device=self.device, dtype=torch.float32).contiguous().view(-1)
        check(self.lib.ddz_select(self._h, _p(q), _p(self.offsets), float(epsilon), _p(out),
                                  _stream(self.device)))
        return out

    def select_slab(self, q, epsilon=0.0, out=None):
        """select() for the slab layout: q f32 [T, stride] (entries beyond counts[t] are ignored); returns
        int32[T] indices for step_slab(STEP_CHOICE).  Same greedy / epsilon-greedy rule and RNG as select()."""
        if not self._slab_fresh:
            self.legal_slab()
        out, q = self._ids_out(out), self._q_slab_arg(q)
        check(self.lib.ddz_select_slab(self._h, _p(q), self._pp["counts"], self.slab_stride, float(epsilon), _p(out),
                                       _stream(self.device)))
        return out

    # ---- the needed-rows form of the ragged Q forward (csrc/ddz_qnet.h; dqn_glue.FactorisedQ.needed) ----
    def q_need(self, row_capacity, scratch, row_index, seg, row_cnt):
        """ddz_q_need: which (rank, count >= 1) rows the CURRENT slab lists use, per table, laid out in rank segments:
        writes row_index int32 [T,64], seg int32 [40] and row_cnt uint8 [row_capacity] (device); nothing crosses to the host."""
        if not self._slab_fresh:
            self.legal_slab()
        self._arg(scratch, "scratch", torch.uint8)
        self._arg(row_index, "row_index", torch.int32, shape=(self.T, 64))
        self._arg(seg, "seg", torch.int32, at_least=40)
        self._arg(row_cnt, "row_cnt", torch.uint8, at_least=int(row_capacity))
        check(self.lib.ddz_q_need(self._h, self._pp["counts"], self._pp["rows"], self.slab_stride, int(row_capacity),
                                  _p(scratch), scratch.numel(), _p(row_index), _p(seg), _p(row_cnt), _stream(self.device)))

    def q_shared_rows(self, ws, row_capacity, rows, rep, seg, variant=3):
        """ddz_q_shared_rows: one row per DISTINCT (rank, face column) of the CURRENT states for the faces of `variant`:
        rows int32 [T,16] (row of (t, r)), rep int32 [row_capacity] (row -> instance 16 t + r), seg int32 [40] (rank segments).
        variant 3 (EnvCooperationSimplify): direct-addressed, ws uint8 [q_shared_ws_bytes()]; variants 1 / 2 (EnvComplicated /
        EnvCooperation): ddz_q_shared_rows_hashed, ws uint8 [q_shared_hash_ws_bytes(T)], row_capacity >= 15 T + 15 tiles (any
        other variant: DdzError).  Nothing crosses to the host."""
        self._shared_rows_out(1, ws, row_capacity, rows, rep, seg)
        if int(variant) == 3:
            check(self.lib.ddz_q_shared_rows(self._h, _p(ws), ws.numel(), int(row_capacity), _p(rows), _p(rep), _p(seg),
                                             _stream(self.device)))
        else:
            check(self.lib.ddz_q_shared_rows_hashed(self._h, int(variant), _p(ws), ws.numel(), int(row_capacity), _p(rows), _p(rep),
                                                    _p(seg), _stream(self.device)))

    def _check_q_need(self, n_nets, row_index, rows, sseg, ws, row_capacity, row_index2, drep, dseg, row_cnt):
        """the argument checks of q_shared_need (n_nets None: one partition) and q_roles_need (n_nets slot-major partitions of
        row_capacity rows, a segment table each); returns the number of partitions"""
        N = 1 if n_nets is None else int(n_nets)
        self._arg(row_index, "row_index", torch.int32, shape=(self.T, 64))
        self._arg(rows, "rows", torch.int32, shape=(self.T, 16))
        self._arg(sseg, "sseg", torch.int32, at_least=40 * N)
        self._arg(ws, "ws", torch.uint8)
        self._arg(row_index2, "row_index2", torch.int32, shape=(self.T, 64))
        self._arg(drep, "drep", torch.int32, at_least=N * int(row_capacity))
        self._arg(dseg, "dseg", torch.int32, at_least=40 * N)
        self._arg(row_cnt, "row_cnt", torch.uint8, at_least=N * int(row_capacity))
        return N

    def q_shared_need(self, row_index, rows, sseg, shared_row_capacity, ws, row_capacity, row_index2, drep, dseg, row_cnt):
        """ddz_q_shared_need: one D row per distinct (shared row, count) some table needs: row_index2 int32 [T,64], drep int32
        [row_capacity], dseg int32 [40], row_cnt uint8 [row_capacity] from q_need's row_index and q_shared_rows' rows / sseg."""
        self._check_q_need(None, row_index, rows, sseg, ws, row_capacity, row_index2, drep, dseg, row_cnt)
        check(self.lib.ddz_q_shared_need(self._h, _p(row_index), _p(rows), _p(sseg), int(shared_row_capacity), _p(ws), ws.numel(),
                                         int(row_capacity), _p(row_index2), _p(drep), _p(dseg), _p(row_cnt), _stream(self.device)))

    def _check_q_slab(self, n_nets, h0, d, row_index, w2, b2, out, slot=None):
        """the argument checks of q_slab_needed (n_nets None: one network, and `out` may be None and is then made) and q_roles_slab
        (+ slot), behind a fresh legal_slab(); returns (hidden, out)"""
        self._slab_lists()
        H, N = int(h0.shape[-1]), 1 if n_nets is None else int(n_nets)
        self._arg(h0, "h0", torch.float32, shape=(self.T, H))
        self._arg(d, "d", torch.float32, shape=(d.shape[0], H))
        self._arg(row_index, "row_index", torch.int32, shape=(self.T, 64))
        self._arg(w2, "w2", torch.float32, numel=N * H)
        self._arg(b2, "b2", torch.float32, numel=N)
        if out is None and n_nets is None:
            out = torch.zeros((self.T, self.slab_stride), dtype=torch.float32, device=self.device)
        self._arg(out, "out", torch.float32, numel=self.T * self.slab_stride)
        if n_nets is not None:
            self._arg(slot, "slot", torch.int8, numel=self.T)
        return H, out

    def q_slab_needed(self, h0, d, row_index, w2, b2, out=None):
        """ddz_q_slab_needed: q f32 [T, stride] of every legal move from h0 f32 [T,256], d f32 [rows,256] (with z folded in by
        q_fc1_rows), row_index."""
        H, out = self._check_q_slab(None, h0, d, row_index, w2, b2, out)
        check(self.lib.ddz_q_slab_needed(self._h, _p(h0), _p(d), int(d.shape[0]), _p(row_index), H, _p(w2), _p(b2),
                                         self._pp["counts"], self._pp["rows"], self.slab_stride, _p(out), _stream(self.device)))
        return out

    # ---- per-role networks in one shared-rows forward (csrc/ddz_qnet.h section 7; dqn_glue.RoleQ) ----
    def q_roles_rows(self, variant, net_of_role, n_nets, ws, row_capacity, rows, rep, seg, slot):
        """ddz_q_roles_rows: the shared rows keyed by (network slot, rank, column) for the role map net_of_role (3 ints, role order
        up, lord, down: a slot 0 .. n_nets - 1 or -1 = the rule agent): rows int32 [T,16] (absolute rows; -1 for rule tables), rep
        int32 [n_nets * row_capacity], seg int32 [n_nets, 40] (per slot, relative to its partition of row_capacity rows), slot
        int8 [T] (-1 = rule table).  ws uint8 [q_roles_ws_bytes(T, variant, n_nets)]."""
        N = int(n_nets)
        self._shared_rows_out(N, ws, row_capacity, rows, rep, seg)
        self._arg(slot, "slot", torch.int8, numel=self.T)
        m = (C.c_int32 * 3)(*[int(x) for x in net_of_role])
        check(self.lib.ddz_q_roles_rows(self._h, int(variant), m, N, _p(ws), ws.numel(), int(row_capacity), _p(rows), _p(rep), _p(seg),
                                        _p(slot), _stream(self.device)))

    def q_roles_need(self, n_nets, row_index, rows, sseg, shared_row_capacity, ws, row_capacity, row_index2, drep, dseg, row_cnt):
        """ddz_q_roles_need: q_shared_need over the slots of q_roles_rows (per-slot capacities; rule tables get no D row)."""
        N = self._check_q_need(n_nets, row_index, rows, sseg, ws, row_capacity, row_index2, drep, dseg, row_cnt)
        check(self.lib.ddz_q_roles_need(self._h, N, _p(row_index), _p(rows), _p(sseg), int(shared_row_capacity), _p(ws), ws.numel(),
                                        int(row_capacity), _p(row_index2), _p(drep), _p(dseg), _p(row_cnt), _stream(self.device)))

    def q_roles_slab(self, n_nets, slot, h0, d, row_index, w2, b2, out):
        """ddz_q_roles_slab: q_slab_needed with the weights of each table's slot (w2 f32 [n_nets,256], b2 f32 [n_nets]); every
        entry of a rule table (slot < 0) is left alone."""
        H, out = self._check_q_slab(n_nets, h0, d, row_index, w2, b2, out, slot)
        check(self.lib.ddz_q_roles_slab(self._h, int(n_nets), _p(slot), _p(h0), _p(d), int(d.shape[0]), _p(row_index), H, _p(w2), _p(b2),
                                        self._pp["counts"], self._pp["rows"], self.slab_stride, _p(out), _stream(self.device)))
        return out

    def legal_onehot(self):
        """valid_actions(tensor=True) for all tables: f32 [sum A,15,4] (one host sync)."""
        self._need_legal()
        total = int(self.offsets[-1].item())
        return rows_to_onehot(self.rows[:total])

    # ---- random-policy rollout, slab layout ----
    @property
    def slab_stride(self):
        """rows per table slab when self.rows is used in the slab layout"""
        return self.cap // self.T

    def slab_rows(self):
        """[T, stride, 16] view of the list buffer after rollout_random: table t's legal
        moves are slab_rows()[t, :counts[t]] (ascending canonical id)."""
        st = self.slab_stride
        return self.rows[: self.T * st].view(self.T, st, ROW)

    def slab_ids(self):
        st = self.slab_stride
        return None if self.ids is None else self.ids[: self.T * st].view(self.T, st)

    def legal_mask(self, out=None, unpack=False):
        """get_mask (rule_based/utils/utils.py:45-63) of every table: the legal moves as a dense mask over the
        action space.  Bit-packed int32 [T, 424] (bit id & 31 of word id >> 5; bit 0 = pass), or with
        unpack=True a bool [T, n_actions] tensor (a policy head with one logit per action masks with it)."""
        W = self.lib.ddz_mask_words()
        if out is None:
            out = torch.empty((self.T, W), dtype=torch.int32, device=self.device)
        else:
            self._arg(out, "out", torch.int32, shape=(self.T, W))
        check(self.lib.ddz_legal_mask(self._h, _p(out), _stream(self.device)))
        if not unpack:
            return out
        bits = (out.unsqueeze(-1) >> torch.arange(32, device=self.device, dtype=torch.int32)) & 1
        return bits.view(self.T, W * 32)[:, : self.lib.ddz_num_actions()].bool()

    def legal_slab(self):
        """Legal-move lists of all tables in the slab layout: (counts[T] i32, rows [T,stride,16] i8,
        ids [T,stride] i32 | None); table t's moves are rows[t, :counts[t]] in ascending canonical id.
        No cross-table prefix, so step_slab() can apply the choices AND write the next lists in one launch."""
        if self.slab_stride < MAX_LEGAL_PER_TABLE:
            raise ValueError(f"slab lists need row_capacity >= {MAX_LEGAL_PER_TABLE} * n_tables")
        check(self.lib.ddz_legal_slab(self._h, _p(self.counts), _p(self.rows), _p(self.ids), self.slab_stride,
                                      _stream(self.device)))
        self._legal_fresh = self._csr_fresh = False  # the CSR buffers (offsets) do not describe the row buffer any more
        self._slab_fresh = True
        return self.counts, self.slab_rows(), self.slab_ids()

    def sync(self):
        """hipStreamSynchronize on the current stream (ddz_sync): after it a host_mirror environment's state / counts are
        what the last launch left."""
        check(self.lib.ddz_sync(self.device.index, _stream(self.device)))

    def step_slab(self, sel=None, mode=STEP_CHOICE, auto_reset=True, traj=None):
        """One lock-step iteration in ONE launch: apply `sel` (STEP_CHOICE: int32[T] index into each
        table's slab list; STEP_ROWS: int8[T,16]; STEP_RANDOM: engine RNG) to the lists legal_slab() /
        the previous step_slab() left in the buffers, then overwrite them with the lists of the new
        states (game.py:95-106 + envi.py:98-116).  Returns (done, r, illegal) like step()."""
        self._slab_lists()
        self._traj(traj)
        pinned = sel is not None and sel.device.type == "cpu" and sel.is_pinned()   # (pinned host memory is device-readable)
        if mode in (STEP_CHOICE, STEP_IDS):
            if sel.dtype != torch.int32 or (sel.device != self.device and not pinned) or not sel.is_contiguous():  # (the host
                sel = sel.to(device=self.device, dtype=torch.int32).contiguous()               # side of a call costs ~10 us)
            if sel.numel() != self.T:
                raise ValueError("choice / ids must have one entry per table")
        elif mode == STEP_ROWS:
            if sel.dtype != torch.int8 or (sel.device != self.device and not pinned) or not sel.is_contiguous():
                sel = sel.to(device=self.device, dtype=torch.int8).contiguous()
            if tuple(sel.shape) != (self.T, ROW):
                raise ValueError("rows must be [T,16] int8")
        elif mode != STEP_RANDOM:
            raise ValueError("bad step mode")
        pp = self._pp
        check(self.lib.ddz_step_slab(self._h, mode, _p(sel) if mode != STEP_RANDOM else None, pp["counts"],
                                     pp["rows"], pp["ids"], self.slab_stride, 1 if auto_reset else 0,
                                     pp["done"], pp["reward"], pp["illegal"], _p(traj),
                                     _stream(self.device)))
        self._legal_fresh, self._slab_fresh, self._csr_fresh = False, True, False  # the buffers hold the lists of the new states
        return self.done, self.reward, self.illegal

    def policy_step_slab(self, q, epsilon=0.0, face_variant=None, face_out=None, choice_out=None, auto_reset=True,
                         traj=None):
        """The environment side of one lock-step iteration of a value-based policy in ONE launch: (epsilon-)greedy
        arg-max of q [T, stride] over each table's slab list (= select_slab), apply it (= step_slab), write the new
        lists and, with face_variant, the `face` [T,P,15,4] of the new states (= observe).  Returns (done, r, illegal,
        face | None); bit-identical to the three separate calls."""
        self._slab_lists()
        self._traj(traj)
        self._arg(choice_out, "choice_out", torch.int32, numel=self.T, none_ok=True)
        face = None if face_variant is None else self._face_out(face_out, face_variant, "face_out")
        q = self._q_slab_arg(q)
        pp = self._pp
        check(self.lib.ddz_policy_step_slab(self._h, _p(q), float(epsilon), pp["counts"], pp["rows"], pp["ids"],
                                            self.slab_stride, 1 if auto_reset else 0, pp["done"], pp["reward"],
                                            pp["illegal"], _p(traj), _p(choice_out),
                                            int(face_variant) if face_variant is not None else 0, _p(face),
                                            _stream(self.device)))
        self._legal_fresh, self._slab_fresh, self._csr_fresh = False, True, False
        return self.done, self.reward, self.illegal, face

    def slab_to_csr(self, rows_per_table=64):
        """The slab lists as CSR (offsets int32[T+1], rows int8[cap,16], ids int32[cap] | None) -- the layout legal()
        returns and a ragged NN forward consumes -- by two small launches; list indices are the same in both layouts, so
        select(q_csr) feeds step_slab(CHOICE).  cap = T * rows_per_table rows (mean list: 5.6 rows under a random
        policy; the first lead of a game: ~73): a fuller list raises status bit 1 and is truncated."""
        self._slab_lists()
        cap = self.T * int(rows_per_table)
        if getattr(self, "_csr_cap", 0) != cap:
            self.csr_rows = torch.empty((cap, ROW), dtype=torch.int8, device=self.device)
            self.csr_ids = torch.empty(cap, dtype=torch.int32, device=self.device) if self.ids is not None else None
            self._csr_cap = cap
        check(self.lib.ddz_slab_to_csr(self._h, self._pp["counts"], self._pp["rows"], self._pp["ids"], self.slab_stride,
                                       self._pp["offsets"], _p(self.csr_rows), _p(self.csr_ids), cap, _stream(self.device)))
        self._csr_fresh = True    # select(q_csr) may use self.offsets as they are; the slab lists stay valid for step_slab
        return self.offsets, self.csr_rows, self.csr_ids

    def rollout_random(self, n_iters, traj=None):
        """n_iters lock-step iterations of {legal list, step_random(auto_reset)}
        (game.py:169-181 with envi.py:79-85), one kernel launch each.  The lists of the last
        iteration's *pre-step* states are left in the slab layout (counts, slab_rows())."""
        if self.slab_stride < MAX_LEGAL_PER_TABLE:
            raise ValueError(f"rollout needs row_capacity >= {MAX_LEGAL_PER_TABLE} * n_tables")
        self._traj(traj, n_iters)
        check(self.lib.ddz_rollout_random(self._h, int(n_iters), _p(self.counts), _p(self.rows),
                                          _p(self.ids), self.slab_stride, _p(self._stats), _p(traj),
                                          _stream(self.device)))
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False

    # ---- playout evaluation (flat Monte Carlo: over perfect information, or over sampled hidden hands) ----
    def playout(self, n_playouts, salt=0, chunks=None, wins=None, totals=None, hidden=False, roles=0b111):
        """Win counts of uniformly random playouts for EVERY legal move of every running table (playout spec v1, DESIGN.md 4;
        the reference's Monte-Carlo player, server/mcts/interface.py:15-45, as flat Monte Carlo): wins int32 [T, stride], entry
        [t, j] = how many of the n_playouts playouts that start with move j of table t's slab list (legal_slab() order) ended
        with a winner on the actor's side (the lord alone, or either farmer).  The env is only read.  One memset + one launch
        on the current stream, nothing on the host: capturable.
        salt: a different salt gives different draws for the same state; chunks: wavefronts per table (default: enough to
        fill the device when there are few tables; the result does not depend on it); wins: an int32 [T * stride] buffer to
        reuse (zeroed here); totals: int64 [4] on the device, += {moves applied, playouts run, playouts stopped unfinished, -}.
        hidden=True (playout spec v2): the opponents' hands are not read but dealt anew for every playout number from the
        cards the actor has not seen (deck - own hand - taken) with their known sizes, every move of a table on the same
        n_playouts worlds -- the evaluation a seat may use, and the one a state from a plain serving payload allows.  A table
        whose hand, taken row and sizes do not add up to a deck runs nothing and raises status bit 6.  roles (hidden form
        only): bit r set = tables whose actor is role r take part, the others are idle."""
        roles = _roles_mask(roles, hidden)
        st = self.slab_stride
        self._slab_lists("playouts need")
        n_playouts = int(n_playouts)
        if not 1 <= n_playouts < (1 << 23):
            raise ValueError("n_playouts must be in [1, 2^23)")
        if chunks is None:
            # a launch lasts as long as its heaviest wavefront, and lists are 1 .. 497 moves long: enough chunks to fill the
            # device (four rounds of its 256 x 24 resident wavefronts) and to cut the longest table's share to a few playouts
            # per move, but no more than ~1.5 M wavefronts in all -- one that finds nothing to do still sizes the root's list
            # (measured, profiles/r11_notes.md: 12 .. 24 chunks are best at K = 8, 24 .. 96 at K = 64)
            fill = -(-24576 // self.T)
            chunks = max(1, min(max(fill, min(3 * n_playouts, 96)), max(fill, 1572864 // self.T), 8192))
        wins = self._slab_counts(wins, "wins")
        self._totals(totals)
        wins.zero_()                   # (an enqueued memset of the whole buffer)
        if hidden:
            check(self.lib.ddz_playout_hidden(self._h, n_playouts, _salt(salt), int(chunks), st, roles, _p(wins),
                                              _p(totals), _stream(self.device)))
        else:
            check(self.lib.ddz_playout(self._h, n_playouts, _salt(salt), int(chunks), st, _p(wins), _p(totals),
                                       _stream(self.device)))
        return wins.view(self.T, st)

    def playout_worlds(self, n_worlds, salt=0, roles=0b111, out=None):
        """The worlds playout(hidden=True) plays on, alone (ddz_playout_worlds): uint8 [T, n_worlds, 2, 16], [t, k, 0] = the
        15 counts and the size of the NEXT player's hand in world k of table t, [t, k, 1] = the PREVIOUS player's -- a
        uniform deal of the cards the actor has not seen, with the known hand sizes.  A sampler for any search built on
        top.  Rows of idle tables, of tables `roles` leaves out and of tables outside the domain (status bit 6) are zero
        (left as they are in a buffer handed in as `out`).  The env is only read; one launch, capturable."""
        n_worlds = int(n_worlds)
        if not 1 <= n_worlds < (1 << 23) or self.T * n_worlds > 0x7FFFFFFF:
            raise ValueError("n_worlds must be in [1, 2^23) and T * n_worlds below 2^31")
        roles = _roles_mask(roles)
        if out is None:
            out = torch.zeros((self.T, n_worlds, 2, ROW), dtype=torch.uint8, device=self.device)
        else:
            self._arg(out, "out", torch.uint8, numel=self.T * n_worlds * 2 * ROW, why=" ([T, n_worlds, 2, 16])")
        check(self.lib.ddz_playout_worlds(self._h, n_worlds, _salt(salt), roles, _p(out), _stream(self.device)))
        return out.view(self.T, n_worlds, 2, ROW)

    def playout_choose(self, n_playouts, salt=0, out=None, chunks=None, hidden=False, roles=0b111):
        """The flat Monte-Carlo move of every table: int32 [T] canonical action ids, the FIRST maximum of playout()'s win
        counts over each table's list (ties to the lowest index), -1 for idle tables.  Feed them to
        step_slab(mode=STEP_IDS).  hidden / roles: as playout() -- a table that the hidden form leaves out (its actor not in
        `roles`, or outside the domain) has all-zero counts and so gets the first move of its list: mask the ids by role."""
        out = self._choose_out("playout_choose", out)
        return self._choose_wins(*self._run_kept("playout", n_playouts, salt=salt, chunks=chunks, hidden=hidden, roles=roles), out)

    # ---- UCT tree search around the playouts (search spec v1) ----
    SEARCH_MODES = {"reference": 0, "sides": 1}
    SEARCH_MAX_BUDGET = 4096

    def search(self, budget, trees=None, mode="reference", c=0.7, salt=0, hidden=False, roles=0b111, visits=None, wins=None,
               totals=None):
        """UCT tree search on every running table (search spec v1; the reference's MCTS player,
        server/mcts/interface.py:37-43 with get_bestchild.py and tree.py:33-51): `trees` independent trees of `budget`
        iterations each per table, their root statistics summed.  -> (visits, wins), int32 [T, stride] each: entry [t, j] =
        the visits of root move j of table t's slab list (legal_slab() order) and how many of them ended with a winner on the
        actor's side.  The env is only read.  Two memsets + one launch on the current stream: capturable.
        trees (default: enough to fill the device when there are few tables, at most 64); mode: "reference" follows
        get_bestchild.py literally (the maximum at the root actor's own nodes, the minimum at every other node), "sides"
        takes the maximum of the mover's side's win ratio at every node; c: the exploration constant (0.7 in the reference);
        salt: different draws for the same state; hidden=True: tree c plays on world c of playout(hidden=True) -- `trees`
        determinizations of the opponents' hands, the opponents' count bytes never read; roles (hidden only): bit r set =
        tables whose actor is role r take part.  visits / wins: int32 [T * stride] buffers to reuse (zeroed here); totals:
        int64 [4] on the device, += {moves applied, iterations run, iterations scored unfinished, nodes created}.  The
        trees live in a workspace of ddz_search_work_bytes(T, budget, trees) bytes cached on the env."""
        roles = _roles_mask(roles, hidden)
        budget, trees, c, visits, wins = self._search_args("search needs", budget, trees, mode, c, visits, wins, totals)
        st = self.slab_stride
        work = self._workspace("_search_work", int(self.lib.ddz_search_work_bytes(self.T, budget, trees)))
        visits.zero_()
        wins.zero_()
        check(self.lib.ddz_search(self._h, budget, trees, self.SEARCH_MODES[mode], c, _salt(salt), int(bool(hidden)),
                                  roles, st, _p(visits), _p(wins), _p(totals), _p(work), work.numel(), _stream(self.device)))
        return visits.view(self.T, st), wins.view(self.T, st)

    def _search_args(self, what, budget, trees, mode, c, visits, wins, totals):
        """the arguments search() and ismcts() share, checked; the slab lists made current -> (budget, trees, c, visits, wins)"""
        if mode not in self.SEARCH_MODES:
            raise ValueError('mode is "reference" or "sides"')
        self._slab_lists(what)
        budget = int(budget)
        if not 1 <= budget <= self.SEARCH_MAX_BUDGET:
            raise ValueError(f"budget must be in [1, {self.SEARCH_MAX_BUDGET}]")
        c = float(c)
        if not 0.0 <= c < 3.0e38:
            raise ValueError("c must be finite and not negative")
        if trees is None:       # one wavefront per (table, tree): the device holds 256 x 24 of them
            trees = max(1, min(64, 6144 // self.T))
        trees = int(trees)
        if not 1 <= trees <= 65536:
            raise ValueError("trees must be in [1, 65536]")
        visits, wins = self._slab_counts(visits, "visits"), self._slab_counts(wins, "wins")
        self._totals(totals)
        return budget, trees, c, visits, wins

    def search_choose(self, budget, trees=None, mode="reference", c=0.7, salt=0, hidden=False, roles=0b111, out=None):
        """The UCT move of every table: int32 [T] canonical action ids, the first maximum of wins / visits over the visited
        root moves of search() (get_bestchild_: the win ratio alone; ties to the lowest index), -1 where nothing was visited
        (idle tables, tables the hidden form leaves out).  Feed them to step_slab(mode=STEP_IDS)."""
        out = self._choose_out("search_choose", out)
        return self._choose_ratio(*self._run_kept("search", budget, trees=trees, mode=mode, c=c, salt=salt, hidden=hidden, roles=roles),
                                  out)

    # ---- information-set MCTS: one tree over all sampled worlds (search spec v2) ----
    def ismcts(self, budget, trees=None, mode="reference", c=0.7, salt=0, roles=0b111, visits=None, wins=None, totals=None):
        """Single-observer information-set MCTS on every running table (search spec v2; Whitehouse, Powley,
        Cowling, CIG 2011; Cowling, Powley, Whitehouse, TCIAIG 2012): where search(hidden=True) builds tree c on world c alone,
        every tree here is built over ALL of its worlds -- iteration i of tree c plays on world c * budget + i of
        playout(hidden=True) (playout_worlds(trees * budget) lists them), each step of the descent sees the moves legal in
        that world, and the UCB bonus uses the child's availability count.  No tree is built with full knowledge of one deal,
        and one tree gets the whole budget.  -> (visits, wins) as search(); mode, c, salt, roles, visits / wins / totals:
        as search(hidden=True).  The opponents' count bytes are never read; a table outside the domain runs nothing and raises
        status bit 6.  The env is only read.  Two memsets + one launch on the current stream: capturable.  The trees live in a
        workspace of ddz_ismcts_work_bytes(T, budget, trees) bytes cached on the env."""
        roles = _roles_mask(roles)
        budget, trees, c, visits, wins = self._search_args("ismcts needs", budget, trees, mode, c, visits, wins, totals)
        st = self.slab_stride
        work = self._workspace("_ismcts_work", int(self.lib.ddz_ismcts_work_bytes(self.T, budget, trees)))
        visits.zero_()
        wins.zero_()
        check(self.lib.ddz_ismcts(self._h, budget, trees, self.SEARCH_MODES[mode], c, _salt(salt), roles, st, _p(visits),
                                  _p(wins), _p(totals), _p(work), work.numel(), _stream(self.device)))
        return visits.view(self.T, st), wins.view(self.T, st)

    def ismcts_choose(self, budget, trees=None, mode="reference", c=0.7, salt=0, roles=0b111, out=None):
        """The ISMCTS move of every table: int32 [T] canonical action ids, search_choose()'s rule on ismcts()'s root
        statistics; -1 where nothing was visited.  Feed them to step_slab(mode=STEP_IDS)."""
        out = self._choose_out("ismcts_choose", out)
        return self._choose_ratio(*self._run_kept("ismcts", budget, trees=trees, mode=mode, c=c, salt=salt, roles=roles), out)

    # ---- UCT with leaf values from outside the kernel (search spec v3) ----
    GUIDED_ONE = 1024

    def guided(self, budget, trees=None, mode="reference", c=0.7, salt=0, hidden=False, roles=0b111):
        """Opens a guided UCT search on every running table (search spec v3): search()'s trees, but the score of
        a new non-terminal leaf is a value the caller hands in instead of a playout's result, and one launch runs one
        iteration of every (table, tree).  -> a GuidedSearch: step() it `budget` times, filling .values for the leaves
        .need marks from the rows in .leaves between the steps, then close() it for (visits, wins); or run(evaluator).
        Arguments as search(); budget * trees * 1024 must stay below 2^31.  THE ENVIRONMENT MUST NOT BE STEPPED, RESET OR
        IMPORTED INTO BETWEEN guided() AND close(): every launch re-reads the root from the state.  One search at a time
        per environment (they share the cached workspace): a second guided() before close() raises RuntimeError."""
        if getattr(self, "_guided_pending", None) is not None:
            raise RuntimeError("a guided search is open on this environment's workspace: close() it first")
        return GuidedSearch(self, budget, trees, mode, c, salt, hidden, roles)

    # ---- guided UCT with move priors (search spec v5) ----
    def guided_puct(self, budget, trees=None, c=1.25, salt=0, hidden=False, roles=0b111, pool=None, mode="sides"):
        """Opens a guided PUCT search on every running table (search spec v5): guided()'s phases and unit, but
        every evaluated node also keeps a prior weight for each of its moves, selection runs over ALL moves of a node by
        mean + c * p * sqrt(N) / (1 + V), and nothing is expanded at random.  -> a GuidedSearch with the extra field .priors
        (uint8 [T * trees, stride]): the evaluator fills .values AND .priors[k, :n] (the weights of the leaf's moves in the
        order of legal_slab() on the imported leaf row) between the steps; PlayoutLeaf and dqn_glue.QLeaf do.  The first step
        evaluates the root.  Only the "sides" rule (mode is there to say so: anything else is a ValueError).  pool: bytes of
        prior weights a tree can keep, a multiple of 16 (default 64 * budget rounded up); a node it has no room for is
        uniform and counted in totals[4].  close(totals) takes int64 [5].  budget * trees * 1024 must stay below 2^31; the
        same one-open-search-per-environment rule, shared with guided()."""
        if mode != "sides":
            raise ValueError('guided_puct has the "sides" rule only')
        if getattr(self, "_guided_pending", None) is not None:
            raise RuntimeError("a guided search is open on this environment's workspace: close() it first")
        return GuidedSearch(self, budget, trees, "sides", c, salt, hidden, roles, puct=True, pool=pool)

    def guided_puct_choose(self, evaluator, budget, trees=None, c=1.25, salt=0, hidden=False, roles=0b111, pool=None, out=None):
        """The guided-PUCT move of every table: int32 [T] canonical action ids, the move with the most visits of
        guided_puct(...).run(evaluator), ties to the lowest index (ddz_playout_choose's rule on the visits); an idle table
        gets what playout_choose gives it.  Feed them to step_slab(mode=STEP_IDS)."""
        out = self._choose_out("guided_puct_choose", out)
        visits, _ = self.guided_puct(budget, trees=trees, c=c, salt=salt, hidden=hidden, roles=roles, pool=pool).run(evaluator)
        return self._choose_wins(visits, out)

    def guided_choose(self, evaluator, budget, trees=None, mode="reference", c=0.7, salt=0, hidden=False, roles=0b111, out=None):
        """The guided-UCT move of every table: int32 [T] canonical action ids, search_choose()'s rule (ddz_search_choose: the
        first maximum of wins / visits, compared exactly) on guided(...).run(evaluator)'s root statistics; -1 where nothing
        was visited.  Feed them to step_slab(mode=STEP_IDS)."""
        out = self._choose_out("guided_choose", out)
        return self._choose_ratio(*self.guided(budget, trees=trees, mode=mode, c=c, salt=salt, hidden=hidden, roles=roles).run(evaluator),
                                  out)

    # ---- information-set MCTS with leaf values from outside the kernel (search spec v4) ----
    def guided_ismcts(self, budget, trees=None, mode="reference", c=0.7, salt=0, roles=0b111):
        """Opens a guided ISMCTS search on every running table (search spec v4): ismcts()'s trees -- ONE tree per
        (table, tree) over all of its worlds, iteration i of tree c on world c * budget + i, every step of the descent on the
        list of that world, the child's availability count in the bonus -- judged as guided()'s are: the score of a new
        non-terminal leaf is a value the caller hands in, one launch runs one iteration, and the leaf row holds that
        iteration's world as the opponents' hands.  Always the hidden form: the search a seat can run with a network.
        -> a GuidedSearch, used exactly as guided()'s (PlayoutLeaf and dqn_glue.QLeaf serve as they are); budget * trees *
        1024 must stay below 2^31; the same one-open-search-per-environment rule, shared with guided()."""
        if getattr(self, "_guided_pending", None) is not None:
            raise RuntimeError("a guided search is open on this environment's workspace: close() it first")
        return GuidedSearch(self, budget, trees, mode, c, salt, True, roles, ismcts=True)

    def guided_ismcts_choose(self, evaluator, budget, trees=None, mode="reference", c=0.7, salt=0, roles=0b111, out=None):
        """The guided-ISMCTS move of every table: int32 [T] canonical action ids, search_choose()'s rule on
        guided_ismcts(...).run(evaluator)'s root statistics; -1 where nothing was visited.  Feed them to
        step_slab(mode=STEP_IDS)."""
        out = self._choose_out("guided_ismcts_choose", out)
        return self._choose_ratio(*self.guided_ismcts(budget, trees=trees, mode=mode, c=c, salt=salt, roles=roles).run(evaluator), out)

    # ---- the CFR endgame solver (CFR spec v1) ----
    CFR_STRIDE = 16
    CFR_MAX_ITERATIONS = 64

    def cfr_default_slots(self):
        """slots of cfr() where none are asked for: endgames are a small share of live tables, so T / 16, at least 64, never
        more than T -- 108 MiB of workspace up to 1,024 tables, 6.75 GiB at 65,536"""
        return min(self.T, max(64, self.T // 16))

    def cfr(self, iterations=8, roles=0b111, slots=None, totals=None, out=None):
        """The reference's final_card (server/CFR.py: 8 iterations of vanilla CFR over every deal of the unseen cards) for
        every table that is an endgame: running, its actor in `roles`, at most 6 cards in the three hands together (CFR spec
        v1).  -> (n, ids, sigma, value): n int32 [T] = the size of the actor's legal list (0 idle, -1 not an
        endgame -- more than 6 cards, no status bit -- or rows that do not add up, status bit 6; -2 no workspace slot or over
        a capacity, status bit 7); ids int32 [T, 16] the list's canonical ids (-1 padded); sigma float64 [T, 16] the
        strategy at (actor, its hand, no action); value float64 [T] the last iteration's value of the game for the lord.
        Only the actor's hand, the taken and recent rows and the others' hand SIZES are read: a state from a plain serving
        payload is solved as the live table it describes.  Bit-identical from run to run.  The env is only read; two launches
        (the workspace head's zeroing, the solver) on the current stream: capturable.
        slots: endgames solved per call (default cfr_default_slots(): T / 16, at least 64, at most T); each owns 1,728 KiB of
        a workspace that stays cached on the env (slots * 1.69 MiB: 108 MiB at 64 slots, 6.75 GiB at 4,096).  Tables beyond
        the slots report -2 and can be solved by a second call with more slots or with `roles` / fewer tables.
        totals: int64 [4] on the device, += {deals, nodes, information sets, (set, action) pairs}.  out: the four tensors of
        an earlier call, to reuse."""
        iterations = int(iterations)
        if not 0 <= iterations <= self.CFR_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in [0, {self.CFR_MAX_ITERATIONS}]")
        roles = _roles_mask(roles)
        slots = self.cfr_default_slots() if slots is None else int(slots)
        need = int(self.lib.ddz_cfr_work_bytes(slots))
        if slots < 0 or need < 0:
            raise ValueError("slots must be in [0, 2^24]")
        self._totals(totals)
        if out is None:
            out = (torch.empty(self.T, dtype=torch.int32, device=self.device),
                   torch.empty((self.T, self.CFR_STRIDE), dtype=torch.int32, device=self.device),
                   torch.empty((self.T, self.CFR_STRIDE), dtype=torch.float64, device=self.device),
                   torch.empty(self.T, dtype=torch.float64, device=self.device))
        n, ids, sigma, value = self._cfr_tensors(out, "out")
        self._arg(value, "value", torch.float64, numel=self.T, why=" (of out)")
        work = self._workspace("_cfr_work", need)     # (at least the 256 bytes of its head)
        check(self.lib.ddz_cfr(self._h, iterations, roles, slots, _p(work), work.numel(), _p(n), _p(ids), _p(sigma), _p(value),
                               _p(totals), _stream(self.device)))
        return n, ids, sigma, value

    def cfr_choose(self, iterations=8, roles=0b111, slots=None, salt=0, greedy=False, solved=None, out=None):
        """The CFR move of every endgame table: int32 [T] canonical action ids for step_slab(mode=STEP_IDS), -1 where cfr()
        solved nothing (n <= 0: mask by it).  greedy: the first maximum of sigma; otherwise sampled from sigma as the
        reference's choose() does, with the engine's own draw (RNG domain 8, keyed by the table id, the seed and `salt`).
        solved: the (n, ids, sigma, value) of an earlier cfr() call to choose from (no solve)."""
        out = self._ids_out(out)
        if solved is None:
            solved = self._run_kept("cfr", iterations, roles=roles, slots=slots)
        n, ids, sigma, _ = self._cfr_tensors(solved, "solved")
        return self._choose_sigma(n, ids, sigma, salt, greedy, out)

    # ---- the exact endgame solver (solve spec v1) ----
    SOLVE_MAX_CARDS = 20
    SOLVE_MAX_BUDGET = 1 << 30
    SOLVE_MAX_TT = 1 << 20

    def _solve_tensors(self, t, name):
        """the (n, wins, unknown) of a solve() call, handed back as `name`"""
        n, wins, unknown = t
        why = f" (of {name}: the (n, wins, unknown) of an earlier solve() call)"
        self._arg(n, "n", torch.int32, numel=self.T, why=why)
        self._arg(wins, "wins", torch.int32, numel=self.T * self.slab_stride, why=why)
        self._arg(unknown, "unknown", torch.int32, numel=self.T * self.slab_stride, why=why)
        return n, wins, unknown

    def solve(self, budget=65536, max_cards=12, worlds=1, hidden=False, roles=0b111, salt=0, chunks=1, tt_entries=4096, out=None,
              totals=None):
        """The exact value of every legal move of every table that is an endgame (solve spec v1): open-hand
        minimax of the win / lose game between the lord and the two farmers, a depth-first search with a transposition table
        per root move.  -> (n, wins, unknown): n int32 [T] = the size of the actor's legal list where the table was solved (0
        idle; -1 not an endgame -- more than max_cards cards in the three hands, no status bit -- or, hidden form, rows that do
        not add up to a deck, status bit 6); wins int32 [T, stride], entry [t, j] = 1 iff after move j of table t's slab
        list (legal_slab() order) the actor's side wins under best play of both sides; unknown int32 [T, stride], 1 where the
        search of move j ran out of `budget` nodes (its wins entry is 0 then).  Where unknown is 0, wins is a fact about the
        game: it depends on none of budget, chunks and tt_entries.  The env is only read.  Two memsets + one launch on the
        current stream, nothing on the host: capturable.
        budget: nodes per root move; max_cards <= 20; hidden=True: the opponents' hands are not read but dealt `worlds` times
        from the cards the actor has not seen, exactly the worlds playout_worlds(worlds, salt) returns, and wins / unknown
        are sums over them (perfect-information Monte Carlo: the root list is the same in every world); roles (hidden form
        only): bit r set = tables whose actor is role r take part.  The open form takes worlds=1.  chunks: wavefronts per
        (table, world), chunk c solves the root moves j = c (mod chunks) with a table of its own; tt_entries: entries of a
        transposition table, a power of two (32 bytes each; T * worlds * chunks of them live in a workspace cached on the
        env: 128 KiB per wavefront at the default).  totals: int64 [4] on the device, += {nodes, table hits, root moves
        solved, root moves unknown}.  out: the three tensors of an earlier call, to reuse (wins / unknown are zeroed here)."""
        hidden = bool(hidden)
        roles = _roles_mask(roles, hidden)
        st = self.slab_stride
        self._slab_lists("solve needs")
        budget, max_cards, worlds, chunks, tt_entries = int(budget), int(max_cards), int(worlds), int(chunks), int(tt_entries)
        if not 1 <= budget <= self.SOLVE_MAX_BUDGET:
            raise ValueError(f"budget must be in [1, {self.SOLVE_MAX_BUDGET}]")
        if not 1 <= max_cards <= self.SOLVE_MAX_CARDS:
            raise ValueError(f"max_cards must be in [1, {self.SOLVE_MAX_CARDS}]")
        if not 1 <= worlds <= 65536 or (not hidden and worlds != 1):
            raise ValueError("worlds must be in [1, 65536], and 1 in the open form (hidden=False)")
        if not 1 <= chunks <= 65536:
            raise ValueError("chunks must be in [1, 65536]")
        if not 1 <= tt_entries <= self.SOLVE_MAX_TT or tt_entries & (tt_entries - 1):
            raise ValueError(f"tt_entries must be a power of two in [1, {self.SOLVE_MAX_TT}]")
        self._totals(totals)
        if out is None:
            out = (torch.empty(self.T, dtype=torch.int32, device=self.device),
                   torch.empty(self.T * st, dtype=torch.int32, device=self.device),
                   torch.empty(self.T * st, dtype=torch.int32, device=self.device))
        n, wins, unknown = self._solve_tensors(out, "out")
        work = self._workspace("_solve_work", int(self.lib.ddz_solve_work_bytes(self.T, worlds, chunks, tt_entries)))
        wins.zero_()
        unknown.zero_()
        check(self.lib.ddz_solve(self._h, budget, max_cards, worlds, int(hidden), roles, _salt(salt), chunks, tt_entries,
                                 st, _p(n), _p(wins), _p(unknown), _p(totals), _p(work), work.numel(), _stream(self.device)))
        return n, wins.view(self.T, st), unknown.view(self.T, st)

    def solve_choose(self, budget=65536, max_cards=12, worlds=1, hidden=False, roles=0b111, salt=0, chunks=1, tt_entries=4096,
                     solved=None, out=None, value=None):
        """The solver's move of every endgame table -> (ids, value): ids int32 [T] canonical action ids for
        step_slab(mode=STEP_IDS), the first move with the most wins, among equals the first with the fewest unknown, -1 for
        tables without a list (idle); value int32 [T] = 1 where that move is proven winning (it wins in every world), 0 where
        every move is proven losing, else -1.  A running table that solve() left out (n = -1) has all-zero counts and so gets
        the first move of its list and value 0: mask by n.  solved: the (n, wins, unknown) of an earlier solve() call with
        the same `worlds` to choose from (no solve)."""
        out = self._choose_out("solve_choose", out)
        if value is None:
            value = torch.empty(self.T, dtype=torch.int32, device=self.device)
        self._arg(value, "value", torch.int32, numel=self.T)
        worlds = int(worlds)
        if not 1 <= worlds <= 65536:
            raise ValueError("worlds must be in [1, 65536]")
        if solved is None:
            solved = self._run_kept("solve", budget, max_cards, worlds, hidden, roles, salt, chunks, tt_entries)
        _, wins, unknown = self._solve_tensors(tuple(x.view(-1) if x is not None and x.is_contiguous() else x for x in solved), "solved")
        return self._choose_solved(worlds, wins, unknown, out, value), value

    def rollout_random_csr(self, n_iters, traj=None, batch=None):
        """The same loop with packed CSR lists (offsets/rows/ids as legal() returns them: afterwards they hold the lists
        of the last iteration's pre-step states).  Same states and trajectories as rollout_random.
        batch (default: as many iterations as CSR_STAGING_BYTES = 16 GiB of staging hold -- 32 at 65,536 tables, 512 at 4096;
        the device has 288 GB -- at most 512): the lists of a batch of iterations are staged as slabs by ONE rollout launch and
        compacted to CSR by two more (ddz_rollout_random_csr_staged) -- no launch per iteration, and the longer the batch the
        less the launch's prologue weighs (tools/csr_batch_probe.py: 65,536 tables 1.95 G steps/s at 4 iterations per batch,
        2.81 G at 32); batch=0: the one-launch-per-iteration form (ddz_rollout_random_csr: CSR bases depend on every table,
        so each iteration waits for the scan of the one before)."""
        self._traj(traj, n_iters)
        if batch is None:
            per = self.T * MAX_LEGAL_PER_TABLE * (20 if self.ids is not None else 16)
            batch = max(2, min(512, CSR_STAGING_BYTES // per))
        if batch:
            batch = int(min(batch, max(1, n_iters)))
            need = self.lib.ddz_rollout_csr_staging_bytes(self.T, batch, int(self.ids is not None))
            self._workspace("_staging", need)
            check(self.lib.ddz_rollout_random_csr_staged(self._h, int(n_iters), batch, _p(self._staging), self._staging.numel(),
                                                         _p(self.offsets), _p(self.rows), _p(self.ids), self.cap, _p(traj),
                                                         _stream(self.device)))
        else:
            check(self.lib.ddz_rollout_random_csr(self._h, int(n_iters), _p(self.offsets), _p(self.rows),
                                                  _p(self.ids), self.cap, _p(traj), _stream(self.device)))
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False

    def rollout_random_timed(self, n_iters):
        """Same loop between two hipEvents; returns the elapsed ms of the n_iters launches.
        Synchronises; measurement aid for bench.py."""
        ms = (C.c_double * 2)()
        check(self.lib.ddz_rollout_random_timed(self._h, int(n_iters), _p(self.counts), _p(self.rows),
                                                _p(self.ids), self.slab_stride, ms,
                                                _stream(self.device)))
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False
        return ms[0]

    def stats(self):
        """{plies, episodes, legal_rows, lord_wins, up_wins, down_wins} accumulated so far (the
        per-role win counts of Game.compete, game.py:258-290); host sync."""
        check(self.lib.ddz_read_stats(self._h, _p(self._stats), _stream(self.device)))
        p, e, l, w, u, dn = self._stats.tolist()[:6]
        return {"plies": p, "episodes": e, "legal_rows": l, "lord_wins": w, "up_wins": u, "down_wins": dn}

    def status(self):
        """device status word (0 = healthy); host sync."""
        out = C.c_int32(0)
        check(self.lib.ddz_status(self._h, C.byref(out), _stream(self.device)))
        return out.value

    # ---- checkpoint (the whole env is one byte tensor) ----
    def state_export(self):
        return self.state.clone()

    def state_import(self, state):
        if state.numel() != self.state.numel():
            raise ValueError("state size mismatch")
        self.state.copy_(state.to(self.device).view(-1))
        check(self.lib.ddz_invalidate(self._h))
        self._legal_fresh = self._slab_fresh = self._csr_fresh = False


class GuidedSearch:
    """One open guided search of a BatchedEnv: guided UCT (search spec v3; BatchedEnv.guided makes it) or guided
    ISMCTS (search spec v4; BatchedEnv.guided_ismcts makes it: the same fields and calls, ddz_gismcts_*'s entry points and
    workspace), or guided PUCT (search spec v5; BatchedEnv.guided_puct makes it: ddz_puct_*'s entry points, the extra field
    `priors`, totals of five).  Item k = t * trees + c is tree c of table t.
      leaves  uint8 [T * trees, 11, 16]: after step(), the state row of every item's pending leaf (an all-zero row, dealt = 0,
              where the item waits for nothing: a leaf environment that imports them freezes those)
      need    int32 [T * trees]: 1 where the item waits for a value
      values  int32 [T * trees], CALLER-FILLED between the steps: the chance in 1024ths that the side of the leaf's ACTOR
              wins (clamped into [0, 1024] by the kernel; entries with need = 0 are not read)
      priors  (guided_puct only) uint8 [T * trees, stride], CALLER-FILLED beside values: priors[k, j] is the weight of move j
              of item k's leaf, in the order of legal_slab() on the imported leaf row; entries at or beyond the leaf's list
              size are not read
    step() backs up the previous step's leaves with `values` and runs one iteration; close() backs up the last ones and
    returns (visits, wins) int32 [T, stride], wins in 1024ths.  Every call is one launch on the current stream, nothing on
    the host: a whole run can be captured in a graph.  The environment must not change between guided() and close().
    step() after close(), or a second close(), raises RuntimeError without touching the device."""

    def __init__(self, env, budget, trees, mode, c, salt, hidden, roles, ismcts=False, puct=False, pool=None):
        self.env = env
        self.ismcts = bool(ismcts)
        self.puct = bool(puct)
        self.hidden = bool(hidden) or self.ismcts
        self.roles = _roles_mask(roles, self.hidden)
        self._verb = "ddz_gismcts" if self.ismcts else "ddz_puct" if self.puct else "ddz_guided"
        self.budget, self.trees, self.c, self._visits, self._wins = env._search_args("guided needs", budget, trees, mode, c, None, None,
                                                                                    None)
        if self.budget * self.trees * env.GUIDED_ONE >= 1 << 31:
            raise ValueError("budget * trees * 1024 must stay below 2^31 (the int32 root sums)")
        self.mode, self.salt = env.SEARCH_MODES[mode], _salt(salt)
        n = env.T * self.trees
        self.n_items = n
        self.leaves = torch.zeros((n, NFIELDS, ROW), dtype=torch.uint8, device=env.device)
        self.need = torch.zeros(n, dtype=torch.int32, device=env.device)
        self.values = torch.zeros(n, dtype=torch.int32, device=env.device)
        self.steps = 0
        self.closed = False
        self._pool = ()
        if self.puct:
            pool = (64 * self.budget + 15) & ~15 if pool is None else int(pool)
            if pool < 16 or pool % 16 or pool > 1 << 24:
                raise ValueError("pool must be a multiple of 16 in [16, 2^24]")
            self.pool, self._pool = pool, (pool,)
            self.priors = torch.zeros((n, env.slab_stride), dtype=torch.uint8, device=env.device)
        self._work = env._workspace("_gismcts_work" if self.ismcts else "_puct_work" if self.puct else "_guided_work",
                                    int(self._fn("work_bytes")(env.T, self.budget, self.trees, *self._pool)))
        check(self._fn("open")(env._h, *self._common(), env.slab_stride, *self._pool, _p(self._work), self._work.numel(),
                               _stream(env.device)))
        env._guided_pending = self

    def _fn(self, phase):
        """the entry point of `phase`: ddz_guided_*'s, or ddz_gismcts_*'s (the same arguments without `hidden`)"""
        return getattr(self.env.lib, f"{self._verb}_{phase}")

    def _common(self):
        head = (self.budget, self.trees, self.mode, self.c, self.salt)
        return head + (self.roles,) if self.ismcts else head + (int(self.hidden), self.roles)

    def _values(self):
        """(values,), or (values, priors) of a PUCT search: checked, as they go to a step or a close (None before the first step)"""
        got = (self.env._arg(self.values, "values", torch.int32, numel=self.n_items),)
        if self.puct:
            got += (self.env._arg(self.priors, "priors", torch.uint8, numel=self.n_items * self.env.slab_stride),)
        return tuple(_p(x) if self.steps else None for x in got)

    def step(self):
        """back up the pending leaves with .values, then one iteration of every item -> (leaves, need)"""
        if self.closed:
            raise RuntimeError("step() on a closed guided search")
        env = self.env
        values = self._values()
        env._arg(self.leaves, "leaves", torch.uint8, numel=self.n_items * NFIELDS * ROW)
        env._arg(self.need, "need", torch.int32, numel=self.n_items)
        check(self._fn("step")(env._h, *self._common(), env.slab_stride, *self._pool, *values,
                               _p(self.leaves), _p(self.need), _p(self._work), self._work.numel(), _stream(env.device)))
        self.steps += 1
        return self.leaves, self.need

    def close(self, totals=None):
        """back up the last pending leaves -> (visits, wins) int32 [T, stride]; totals: int64 [4] on the device, +=
        {moves applied, iterations run, iterations scored unfinished, nodes created}; a PUCT search: int64 [5], then the nodes
        that fell back to uniform priors"""
        if self.closed:
            raise RuntimeError("close() on a closed guided search")
        env = self.env
        values = self._values()
        if self.puct:
            env._arg(totals, "totals", torch.int64, at_least=5, none_ok=True)
        else:
            env._totals(totals)
        self._visits.zero_()
        self._wins.zero_()
        check(self._fn("close")(env._h, *self._common(), *values, env.slab_stride, *self._pool,
                                _p(self._visits), _p(self._wins), _p(totals), _p(self._work), self._work.numel(),
                                _stream(env.device)))
        self.closed = True
        env._guided_pending = None
        return self._visits.view(env.T, env.slab_stride), self._wins.view(env.T, env.slab_stride)

    def run(self, evaluator, totals=None):
        """`budget` steps with evaluator(self) between them (it fills .values from .leaves / .need), then close()"""
        for _ in range(self.budget):
            self.step()
            evaluator(self)
        return self.close(totals)


class PlayoutLeaf:
    """A leaf evaluator for GuidedSearch.run: flat Monte Carlo from the leaf.  The leaf rows are imported into a scratch
    BatchedEnv of one table per item (made once, with the searched environment's seed, rule set and table_id_base 0; made anew
    when a later search has another item count, device or rule set), playout(K) runs
    there, and value = (max_j wins_j * 1024) // K: the best move's win rate for the leaf's actor, in integers.  A search with
    a `priors` field (guided_puct) also gets the weight of every move j of a leaf's list, w_j = 1 + (254 * wins_j) // K: the
    scratch environment's slab lists are in the order the search reads them.  No network."""

    def __init__(self, n_playouts, salt=0, chunks=None):
        self.K, self.salt, self.chunks = int(n_playouts), salt, chunks
        self.env = None

    def scratch(self, search):
        if (self.env is None or self.env.T != search.n_items or self.env.device != search.env.device
                or self.env.native_joker_kickers != search.env.native_joker_kickers):
            self.env = BatchedEnv(search.n_items, seed=search.env.seed, device=search.env.device,
                                  native_joker_kickers=search.env.native_joker_kickers)
        return self.env

    def __call__(self, search):
        env = self.scratch(search)
        env.state_import(search.leaves)
        wins, = env._run_kept("playout", self.K, salt=self.salt, chunks=self.chunks)
        wins = wins.view(env.T, -1)
        search.values.copy_(torch.div(wins.amax(dim=1) * BatchedEnv.GUIDED_ONE, self.K, rounding_mode="floor"))
        priors = getattr(search, "priors", None)
        if priors is not None:
            w = (1 + torch.div(254 * wins, self.K, rounding_mode="floor")).to(torch.uint8)
            inside = torch.arange(wins.shape[1], device=wins.device)[None, :] < env.counts.view(-1, 1)
            priors.copy_(torch.where(inside, w, priors.view(env.T, -1)).view_as(priors))
        return search.values


def guided_values(rows, counts, q, inv_reward, net_roles=0b111, out=None):
    """ddz_guided_values: leaf values from a q slab.  rows uint8 [n, 176] leaf rows, counts int32 [n] list sizes, q f32
    [n, stride]; for every running row whose actor's role is in net_roles, out[i] = clamp((int)rintf((max q[i, :counts[i]] *
    inv_reward[role] + 1) * 512), 0, 1024) -- 512 for an empty list or a NaN -- and every other entry of `out` (int32 [n], made
    zero-filled if None) stays as it is.  No host sync."""
    dev = _require_gpu(rows.device)
    n = counts.numel()
    _chk(rows, "rows", torch.uint8, dev, numel=n * NFIELDS * ROW, why=" (176-byte rows)")
    _chk(counts, "counts", torch.int32, dev, shape=(n,))
    stride = q.numel() // n if n else 1
    _chk(q, "q", torch.float32, dev, numel=n * stride, why=" ([n, stride])")
    if out is None:
        out = torch.zeros(n, dtype=torch.int32, device=dev)
    else:
        _chk(out, "out", torch.int32, dev, numel=n)
    inv = (C.c_float * 3)(*[float(x) for x in inv_reward])
    if n:
        check(_lib.lib().ddz_guided_values(dev.index, _p(rows), _p(counts), _p(q), stride, n, inv, _roles_mask(net_roles, name="net_roles"),
                                           _p(out), _stream(dev)))
    return out


def puct_priors(rows, counts, q, inv_reward, inv_tau=1.0, net_roles=0b111, out=None):
    """ddz_puct_priors: prior weights from a q slab, beside guided_values.  rows uint8 [n, 176] leaf rows, counts int32 [n] list
    sizes, q f32 [n, stride]; for every running row whose actor's role is in net_roles, out[i, j] = clamp((int)rintf(255 *
    expf((q[i, j] - max q[i, :counts[i]]) * inv_reward[role] * inv_tau)), 0, 255) for j < counts[i] -- the maximum gets 255,
    a NaN in the row gives all ones -- and every other entry of `out` (uint8 [n, stride], made zero-filled if None) stays as
    it is.  No host sync."""
    dev = _require_gpu(rows.device)
    n = counts.numel()
    _chk(rows, "rows", torch.uint8, dev, numel=n * NFIELDS * ROW, why=" (176-byte rows)")
    _chk(counts, "counts", torch.int32, dev, shape=(n,))
    stride = q.numel() // n if n else 1
    _chk(q, "q", torch.float32, dev, numel=n * stride, why=" ([n, stride])")
    inv_tau = float(inv_tau)
    if not 0.0 <= inv_tau < 3.0e38:
        raise ValueError("inv_tau must be finite and not negative")
    if out is None:
        out = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    else:
        _chk(out, "out", torch.uint8, dev, numel=n * stride)
    inv = (C.c_float * 3)(*[float(x) for x in inv_reward])
    if n:
        check(_lib.lib().ddz_puct_priors(dev.index, _p(rows), _p(counts), _p(q), stride, n, inv, _roles_mask(net_roles, name="net_roles"),
                                         inv_tau, _p(out), _stream(dev)))
    return out


def rows_to_onehot(rows):
    """batch_arr2onehot (envi.py:139-146) on device: int8 [n,16] -> f32 [n,15,4]."""
    L = _lib.lib()
    dev = _require_gpu(rows.device)
    rows = rows.to(torch.int8).contiguous()
    n = rows.shape[0]
    out = torch.empty((n, 15, 4), dtype=torch.float32, device=dev)
    if n:
        check(L.ddz_rows_to_onehot(dev.index, _p(rows), n, _p(out), _stream(dev)))
    return out


def observe_states(states, index=None, variant=3, out=None):
    """ddz_observe_states: `face` f32 [n,P,15,4] of the packed state rows states[index] (states uint8 [m,176] or [m,11,16] on
    the device; index int64 [n] device tensor whose entries the CALLER keeps inside [0, m), or None = every row in order):
    BatchedEnv.observe's expression, bit for bit, on rows that are not an environment's.  No host sync."""
    dev = _require_gpu(states.device)
    P = FACE_PLANES[variant]
    m = states.numel() // (NFIELDS * ROW)
    _chk(states, "states", torch.uint8, dev, numel=m * NFIELDS * ROW, why=" (176-byte rows)")
    if index is None:
        n = m
    else:
        n = index.numel()
        _chk(index, "index", torch.int64, dev, shape=(n,))
        if n and m == 0:
            raise ValueError("index into an empty states tensor")
    if out is None:
        out = torch.empty((n, P, 15, 4), dtype=torch.float32, device=dev)
    else:
        _chk(out, "out", torch.float32, dev, numel=n * P * 60, why=f" ([n,{P},15,4])")
    if n:
        check(_lib.lib().ddz_observe_states(dev.index, _p(states), _p(index), n, int(variant), _p(out), _stream(dev)))
    return out


def _size_query(symbol, args, error):
    """the library's answer to a `*_bytes` query, or ValueError(error) where it refuses the arguments"""
    n = int(getattr(_lib.lib(), symbol)(*map(int, args)))
    if n < 0:
        raise ValueError(error)
    return n


def _layout_query(symbol, args, names, error):
    """{name: byte offset} from the library's `*_layout` query, or ValueError(error) where it refuses the arguments"""
    off = (C.c_int64 * len(names))()
    if getattr(_lib.lib(), symbol)(*map(int, args), off) != 0:
        raise ValueError(error)
    return dict(zip(names, [int(x) for x in off]))


def tr_ws_bytes(n_tables):
    """bytes of the transition recorder's workspace for n_tables tables (ddz_tr_ws_bytes; zero-filled by the caller)"""
    return _size_query("ddz_tr_ws_bytes", (n_tables,), "n_tables must be in 1 .. 2^30")


def tr_ring_bytes(capacity):
    """bytes of one role's ring of `capacity` packed transitions (ddz_tr_ring_bytes; zero-filled by the caller)"""
    return _size_query("ddz_tr_ring_bytes", (capacity,), "capacity must be in 1 .. 2^30")


TR_RING_FIELDS = ("count", "s0", "s1", "a0", "a1", "reward", "table", "done")


def tr_ring_layout(capacity):
    """{field: byte offset} of a ring (ddz_tr_ring_layout): count int64, s0 / s1 u8 [capacity,176], a0 / a1 int32, reward f32,
    table int32, done u8"""
    return _layout_query("ddz_tr_ring_layout", (capacity,), TR_RING_FIELDS, "capacity must be in 1 .. 2^30")


def mc_ws_bytes(n_tables, log_cap):
    """bytes of the return recorder's workspace for n_tables tables with log_cap log entries each (ddz_mc_ws_bytes; zero-filled
    by the caller; about 182 bytes per log entry)"""
    if not 1 <= int(log_cap) <= 255:
        raise ValueError("log_cap must be in 1 .. 255")
    return _size_query("ddz_mc_ws_bytes", (n_tables, log_cap), "n_tables must be positive and n_tables * log_cap at most 2^30")


MC_WS_REGIONS = ("rows", "act", "who", "cnt", "lost", "rank", "blk", "hdr")


def mc_ws_layout(n_tables, log_cap):
    """{region: byte offset} of the return recorder's workspace (ddz_mc_ws_layout): rows u8 [T,L,176], act int32 [T,L], who u8
    [T,L,2] = {role, ordinal}, cnt u8 [T,4] = {n, c[3]}, lost uint32 [T], rank int32 [T,4], blk int32 [nb,4], hdr int64 [8]"""
    return _layout_query("ddz_mc_ws_layout", (n_tables, log_cap), MC_WS_REGIONS,
                         "log_cap must be in 1 .. 255, n_tables positive and n_tables * log_cap at most 2^30")


def mc_ring_bytes(capacity):
    """bytes of one role's ring of `capacity` return entries (ddz_mc_ring_bytes; zero-filled by the caller)"""
    return _size_query("ddz_mc_ring_bytes", (capacity,), "capacity must be in 1 .. 2^30")


MC_RING_FIELDS = ("count", "s0", "a0", "ret", "table", "togo")


def mc_ring_layout(capacity):
    """{field: byte offset} of a return ring (ddz_mc_ring_layout): count int64, s0 u8 [capacity,176], a0 int32, ret f32, table
    int32, togo u8"""
    return _layout_query("ddz_mc_ring_layout", (capacity,), MC_RING_FIELDS, "capacity must be in 1 .. 2^30")


def teach_ws_bytes(n_tables):
    """bytes of ddz_teach's per-call scratch for n_tables tables (ddz_teach_ws_bytes; nothing in it has to be initialised)"""
    return _size_query("ddz_teach_ws_bytes", (n_tables,), "n_tables must be in 1 .. 2^30")


TEACH_WS_REGIONS = ("rank", "blk", "hdr")


def teach_ws_layout(n_tables):
    """{region: byte offset} of ddz_teach's scratch (ddz_teach_ws_layout): rank int32 [T,4], blk int32 [nb,4], hdr int64 [8]"""
    return _layout_query("ddz_teach_ws_layout", (n_tables,), TEACH_WS_REGIONS, "n_tables must be in 1 .. 2^30")


TeacherStats = collections.namedtuple("TeacherStats", "counts num den den_const unknown scale roles", defaults=(0b111,))
TeacherStats.__doc__ = """What Teacher.evaluate hands BatchedEnv.teach (teacher spec v1): counts int32 [T] the list sizes the
statistics belong to, num int32 [T * stride] the wins of the root actor's side per move, den int32 [T * stride] the visits per
move or None with den_const the total per table, unknown int32 [T * stride] or None, scale the unit of num; roles: the mask of
the roles whose tables the evaluator took (the others' statistics are all zero and must not be labelled).  Views of buffers
cached on the env: the next evaluate() overwrites them."""


class Teacher:
    """One of the evaluators as a source of training targets and of moves (teacher spec v1): kind "playout"
    (BatchedEnv.playout), "search", "ismcts", "guided" / "guided_ismcts" / "guided_puct" (BatchedEnv.guided(...) /
    guided_ismcts(...) / guided_puct(...) .run(evaluator); they need evaluator=, e.g. PlayoutLeaf or dqn_glue.QLeaf;
    "guided_ismcts" is always hidden; "guided_puct" has guided's root statistics and unit, and chooses by visits) or "solve";
    the keyword arguments are the evaluator's own (n_playouts, budget, trees, hidden, roles, salt, ...) and are passed through.  evaluate(env) runs the evaluator once on env's current states and
    returns TeacherStats; choose(env, stats) turns THE SAME statistics into moves with the evaluator's own rule
    (ddz_playout_choose / ddz_search_choose / ddz_solve_choose; "guided_puct": ddz_playout_choose on the visits): no second search.  Nothing here touches the host, so both
    can be captured.  hidden is the caller's choice: labels from open hands (hidden=False, what playout / search / solve
    default to) are legitimate for training a network that only sees its own face, not for serving moves to a seat."""
    KINDS = {"playout": ("playout", ("n_playouts",)), "search": ("search", ("budget",)), "ismcts": ("ismcts", ("budget",)),
             "guided": ("guided", ("budget",)), "guided_ismcts": ("guided_ismcts", ("budget",)),
             "guided_puct": ("guided_puct", ("budget",)), "solve": ("solve", ())}
    GUIDED = ("guided", "guided_ismcts", "guided_puct")     # the kinds that take a leaf evaluator
    _BUFFERS = ("self", "wins", "visits", "totals", "out")

    def __init__(self, kind, evaluator=None, **kwargs):
        import inspect
        if kind not in self.KINDS:
            raise ValueError(f"kind is one of {', '.join(self.KINDS)}")
        method, required = self.KINDS[kind]
        allowed = [p for p in inspect.signature(getattr(BatchedEnv, method)).parameters if p not in self._BUFFERS]
        bad = sorted(set(kwargs) - set(allowed))
        if bad:
            raise ValueError(f"{kind} takes {', '.join(allowed)}; not {', '.join(bad)}")
        missing = [p for p in required if p not in kwargs]
        if missing:
            raise ValueError(f"{kind} needs {', '.join(missing)}")
        if (kind in self.GUIDED) != (evaluator is not None):
            raise ValueError("evaluator= is the leaf evaluator of the kinds " + ", ".join(f'"{k}"' for k in self.GUIDED) + ", and of no other kind")
        self.kind, self.evaluator, self.kwargs = kind, evaluator, dict(kwargs)
        hidden = kind in ("ismcts", "guided_ismcts") or bool(kwargs.get("hidden", False))
        self.roles = _roles_mask(kwargs.get("roles", 0b111), hidden)

    # kind: the verb's statistics, each flat, as TeacherStats' (counts, num, den, den_const, unknown, scale)
    _STATS = {"playout": lambda env, kw, wins: (env.counts, wins, None, int(kw["n_playouts"]), None, 1),
              "search": lambda env, kw, visits, wins: (env.counts, wins, visits, None, None, 1),
              "ismcts": lambda env, kw, visits, wins: (env.counts, wins, visits, None, None, 1),
              "guided": lambda env, kw, visits, wins: (env.counts, wins, visits, None, None, BatchedEnv.GUIDED_ONE),
              "guided_ismcts": lambda env, kw, visits, wins: (env.counts, wins, visits, None, None, BatchedEnv.GUIDED_ONE),
              "guided_puct": lambda env, kw, visits, wins: (env.counts, wins, visits, None, None, BatchedEnv.GUIDED_ONE),
              # its own n as the list sizes: a table that is no endgame (n <= 0) emits nothing
              "solve": lambda env, kw, n, wins, unknown: (n, wins, None, int(kw.get("worlds", 1)), unknown, 1)}

    def evaluate(self, env):
        """run the evaluator on env's current states -> TeacherStats (the slab lists are made current by the evaluator)"""
        kw, kind = self.kwargs, self.kind
        if kind in self.GUIDED:
            got = [x.view(-1) for x in getattr(env, kind)(**kw).run(self.evaluator)]
        else:
            got = env._run_kept(kind, **kw)
        return TeacherStats(*self._STATS[kind](env, kw, *got), self.roles)

    def choose(self, env, stats, out=None):
        """the evaluator's move of every table from stats (evaluate()'s, of env's current states): int32 [T] canonical action
        ids, -1 where the teacher has none -- idle tables, nothing visited, and the tables the evaluator left out (a role
        outside `roles`, or for "solve" a table that is no endgame).  Feed them to step_slab(mode=STEP_IDS) where >= 0."""
        out = env._choose_out("Teacher.choose", out)
        if self.kind == "playout":
            env._choose_wins(stats.num, out)
        elif self.kind == "guided_puct":
            env._choose_wins(stats.den, out)
        elif self.kind == "solve":
            value = env._kept("teach value", lambda: torch.empty(env.T, dtype=torch.int32, device=env.device))
            env._choose_solved(int(stats.den_const), stats.num, stats.unknown, out, value)
            out.copy_(torch.where(stats.counts > 0, out, -1))
        else:
            env._choose_ratio(stats.den, stats.num, out)
        if stats.roles != 0b111:
            role = env.role.clamp(max=2).int()
            taken = (torch.full_like(role, stats.roles) >> role) & 1
            out.copy_(torch.where(taken.bool(), out, -1))
        return out


def state_prob(known60, size1, size2, device="cuda:0"):
    """get_state_prob_manual(known60, size1, size2) (server/core.py:26-33) for a batch: known60 [n,60] thermometers
    of own cards + cards played, size1 / size2 [n] = cards left of the next / next-but-one player.  Returns f32
    [n,2,15,4] on the device (prob planes spec v1: the last two planes of `face`)."""
    L = _lib.lib()
    dev = _require_gpu(device)
    k = torch.as_tensor(known60).reshape(-1, 60)
    k = (k != 0).to(device=dev, dtype=torch.uint8).contiguous()
    n = k.shape[0]
    sizes = torch.stack([torch.as_tensor(size1).reshape(n), torch.as_tensor(size2).reshape(n)], 1)
    sizes = sizes.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty((n, 2, 15, 4), dtype=torch.float32, device=dev)
    if n:
        check(L.ddz_state_prob(dev.index, _p(k), _p(sizes), n, _p(out), _stream(dev)))
    return out


def q_features(face, wf, bias, acnt, y):
    """ddz_q_features: first layer of the ragged Q forward per (table, rank, count) from `face` f32 [T,P,15,4] into
    y f32 [15,5,T,K] (K >= 256; columns >= 256 and counts 2..4 of the joker ranks are left alone).
    dqn_glue.FactorisedQ.tables drives it."""
    L = _lib.lib()
    dev, T, P = _face_arg(face)
    _chk(y, "y", torch.float32, dev, shape=(15, 5, T, y.shape[3] if y.dim() == 4 else 0), why=" ([15,5,T,K])")
    _weight_tables(dev, P, 1, wf, bias, acnt)
    check(L.ddz_q_features(dev.index, _p(face), T, P, _p(wf), _p(bias), _p(acnt), _p(y), int(y.shape[3]), _stream(dev)))
    return y


def _face_arg(face, planes=None):
    """face float32 [n,P,15,4], P among `planes` (None: any) -> (device, n, P).  The face anchors the device of its call: a CPU
    tensor is a DdzError before any shape is looked at."""
    dev = _require_gpu(face.device)
    n, P = (int(face.shape[0]), int(face.shape[1])) if face.dim() == 4 else (0, 0)
    if planes is not None and P not in planes:
        raise ValueError(f"face must be [n,P,15,4] with P among {sorted(planes)}")
    _chk(face, "face", torch.float32, dev, shape=(n, P, 15, 4))
    return dev, n, P


def _faces_arg(face, actions):
    """the learner's faces: face float32 [n,P,15,4] + actions float32 [n,15,4] -> (device, n, P)"""
    dev, n, P = _face_arg(face, FACE_PLANES)
    _chk(actions, "actions", torch.float32, dev, shape=(n, 15, 4))
    return dev, n, P


def _conv_params(dev, P, count, weights, biases=None):
    """the nn.Conv2d parameters of conv1..conv4 (count 4) and conv_shunzi (count 5) as they are"""
    if len(weights) != count or (biases is not None and len(biases) != count):
        raise ValueError("weights / biases: those of conv1..conv4" + (" and conv_shunzi" if count == 5 else ""))
    for k in range(count):
        _chk(weights[k], f"weights[{k}]", torch.float32, dev, shape=(256, P + 1, 1, k + 1) if k < 4 else (256, P + 1, 15, 1))
        if biases is not None:
            _chk(biases[k], f"biases[{k}]", torch.float32, dev, shape=(256,))


def _weight_tables(dev, P, n_nets, wf, bias, *acnt):
    """the first layer's tables of n_nets networks: wf [P*4,1024], bias [1024] and, where the call takes it, acnt [5,4,256] each"""
    _chk(wf, "wf", torch.float32, dev, numel=n_nets * P * 4 * 1024, why=" ([P*4,1024] per network)")
    _chk(bias, "bias", torch.float32, dev, numel=n_nets * 1024)
    for a in acnt:
        _chk(a, "acnt", torch.float32, dev, numel=n_nets * 5 * 4 * 256)


def q_first_fwd(face, actions, weights, biases, want_arg=True):
    """ddz_q_first_fwd: the learner's first layer -- cat, conv1..conv4, cat, max-pool of QNet.forward -- of a batch, the pre-pool
    tensor never materialised: face f32 [n,P,15,4], actions f32 [n,15,4], weights / biases the nn.Conv2d parameters of conv1..4
    as they are ([256,P+1,1,k], [256]) -> (y f32 [n,3840] in the order of net.py:94's view, arg u8 [n,3840] = the lowest conv
    that attains the max -- what q_first_bwd routes by -- or None with want_arg=False).  No host sync."""
    dev, n, P = _faces_arg(face, actions)
    _conv_params(dev, P, 4, weights, biases)
    y = torch.empty((n, 3840), dtype=torch.float32, device=dev)
    arg = torch.empty((n, 3840), dtype=torch.uint8, device=dev) if want_arg else None
    if n:
        check(_lib.lib().ddz_q_first_fwd(dev.index, _p(face), _p(actions), n, P, _ptrs(weights), _ptrs(biases), _p(y), _p(arg),
                                         _stream(dev)))
    return y, arg


def q_first_bwd(face, actions, gy, arg, weights):
    """ddz_q_first_bwd: the gradients of conv1..conv4's parameters from gy f32 [n,3840] and q_first_fwd's arg u8 [n,3840] (the
    conv that won takes the gradient), in the parameters' own shapes: (gw[4], gb[4]); `weights` give the shapes only.
    Deterministic (no atomics: per-block partials, a fixed-order reduce); no gradient of face / actions.  No host sync."""
    dev, n, P = _faces_arg(face, actions)
    _conv_params(dev, P, 4, weights)
    _chk(gy, "gy", torch.float32, dev, shape=(n, 3840))
    _chk(arg, "arg", torch.uint8, dev, shape=(n, 3840), why=" (q_first_fwd's arg)")
    L = _lib.lib()
    if n == 0:
        return [torch.zeros_like(w) for w in weights], [torch.zeros(256, dtype=torch.float32, device=dev) for _ in range(4)]
    gw = [torch.empty_like(w) for w in weights]
    gb = [torch.empty(256, dtype=torch.float32, device=dev) for _ in range(4)]
    ws = torch.empty(int(L.ddz_q_first_bwd_ws_bytes(n, P)), dtype=torch.uint8, device=dev)
    check(L.ddz_q_first_bwd(dev.index, _p(face), _p(actions), n, P, _p(gy), _p(arg), _ptrs(gw), _ptrs(gb), _p(ws), ws.numel(),
                            _stream(dev)))
    return gw, gb


STAGE_WIDTH = 4864      # the row of h: 3840 first-layer values (o * 15 + r), then conv_shunzi's 1024 (o * 4 + j)


def q_stage_source(face=None, actions=None, states=None, ids=None, index=None, table=None, variant=None):
    """The source of the learner's stage (ddz_q_src_t) from checked operands -> (descriptor, device, n, planes, kept tensors).
    faces: face f32 [n,P,15,4] + actions f32 [n,15,4].  rows: states u8 [m,176] + ids int32 [m] (a replay ring's s0 + a0 or
    s1 + a1), index int64 [n] or None (every row in order; the kernels clamp entries into the ring), table int8 [n_actions,16]
    (action_table), variant 0..3.  The descriptor holds raw addresses: the caller keeps the tensors alive across the launch."""
    src = _lib.QSrc()
    if states is None:
        if face is None or actions is None:
            raise ValueError("the stage's source is face + actions, or states + ids + table + variant")
        dev, n, P = _faces_arg(face, actions)
        src.kind, src.planes, src.face, src.action = 0, P, face.data_ptr(), actions.data_ptr()
        return src, dev, n, P, (face, actions)
    dev = _require_gpu(states.device)
    if variant is None or not 0 <= int(variant) < len(FACE_PLANES):
        raise ValueError("variant must be a face variant 0..3")
    m, n_actions = int(states.shape[0]), 0 if table is None else int(table.shape[0])
    if m == 0 or n_actions == 0 or states.data_ptr() % 16:
        raise ValueError("states must be 16-byte aligned with m > 0 rows, table the action table")
    _chk(states, "states", torch.uint8, dev, shape=(m, NFIELDS * ROW))
    _chk(ids, "ids", torch.int32, dev, shape=(m,))
    _chk(table, "table", torch.int8, dev, shape=(n_actions, 16), why=" (action_table)")
    n = m if index is None else int(index.numel())
    _chk(index, "index", torch.int64, dev, shape=(n,), none_ok=True)
    src.kind, src.variant, src.n_actions, src.n_rows = 1, int(variant), n_actions, m
    src.states, src.ids, src.table = states.data_ptr(), ids.data_ptr(), table.data_ptr()
    src.index = None if index is None else index.data_ptr()
    return src, dev, n, FACE_PLANES[int(variant)], (states, ids, index, table)


def q_stage_fwd(weights, biases, want_arg=True, **source):
    """ddz_q_stage_fwd: everything of QNet.forward in front of dropout / fc1 -- cat, conv1..conv4, cat, max-pool, conv_shunzi, the
    views and the cat -- of a batch in two launches, from faces (face=, actions=) or straight from packed replay rows (states=,
    ids=, index=, table=, variant=: q_stage_source), weights / biases the nn.Conv2d parameters of conv1..4 and conv_shunzi as they
    are -> (h f32 [n,4864], arg u8 [n,3840] as q_first_fwd's, or None with want_arg=False).  No host sync."""
    src, dev, n, P, keep = q_stage_source(**source)
    _conv_params(dev, P, 5, weights, biases)
    h = torch.empty((n, STAGE_WIDTH), dtype=torch.float32, device=dev)
    arg = torch.empty((n, 3840), dtype=torch.uint8, device=dev) if want_arg else None
    if n:
        check(_lib.lib().ddz_q_stage_fwd(dev.index, C.byref(src), n, _ptrs(weights), _ptrs(biases), _p(h), STAGE_WIDTH, _p(arg),
                                         _stream(dev)))
    return h, arg


def q_stage_bwd(gh, arg, weights, **source):
    """ddz_q_stage_bwd: the gradients of the ten convolution parameters from gh f32 [n,4864] and q_stage_fwd's arg, in the
    parameters' own shapes: (gw[5], gb[5]); `weights` give the shapes only.  Deterministic (per-block partials, a fixed-order
    reduce: three launches); no gradient of the data.  No host sync."""
    src, dev, n, P, keep = q_stage_source(**source)
    _conv_params(dev, P, 5, weights)
    _chk(gh, "gh", torch.float32, dev, shape=(n, STAGE_WIDTH))
    _chk(arg, "arg", torch.uint8, dev, shape=(n, 3840), why=" (q_stage_fwd's arg)")
    L = _lib.lib()
    if n == 0:
        return [torch.zeros_like(w) for w in weights], [torch.zeros(256, dtype=torch.float32, device=dev) for _ in range(5)]
    gw = [torch.empty_like(w) for w in weights]
    gb = [torch.empty(256, dtype=torch.float32, device=dev) for _ in range(5)]
    ws = torch.empty(int(L.ddz_q_stage_bwd_ws_bytes(n, P)), dtype=torch.uint8, device=dev)
    check(L.ddz_q_stage_bwd(dev.index, C.byref(src), n, _p(gh), STAGE_WIDTH, _p(arg), _ptrs(gw), _ptrs(gb), _p(ws), ws.numel(),
                            _stream(dev)))
    return gw, gb


def q_need_scratch_bytes(n_tables):
    return int(_lib.lib().ddz_q_need_scratch_bytes(int(n_tables)))


def q_features_needed(face, wf, bias, acnt, row_index, y0, dy):
    """ddz_q_features_needed: first layer into y0 f32 [T, 15 * 256] (count 0 of every rank) and dy f32 [rows, 256]
    (Y[count] - Y[0] at the row of every needed (table, rank, count): row_index from BatchedEnv.q_need)."""
    L = _lib.lib()
    dev, T, P = _face_arg(face)
    _weight_tables(dev, P, 1, wf, bias, acnt)
    _chk(row_index, "row_index", torch.int32, dev, shape=(T, 64))
    _chk(y0, "y0", torch.float32, dev, shape=(T, 15 * 256), none_ok=True, why=" (or None: dy alone)")
    _chk(dy, "dy", torch.float32, dev, shape=(dy.shape[0], 256))
    check(L.ddz_q_features_needed(dev.index, _p(face), T, P, _p(wf), _p(bias), _p(acnt), _p(row_index), _p(y0), _p(dy),
                                  int(dy.shape[0]), _stream(dev)))


def q_fc1_dense(a, w, c):
    """ddz_q_fc1_dense: c f32 [n,256] += a f32 [n,k] @ w f32 [k,256] on the fp32 matrix cores (exact f32; k % 16 == 0)."""
    L = _lib.lib()
    dev = _require_gpu(a.device)
    n, k = int(a.shape[0]), int(a.shape[1])
    _chk(a, "a", torch.float32, dev, shape=(n, k))
    _chk(w, "w", torch.float32, dev, shape=(k, 256))
    _chk(c, "c", torch.float32, dev, shape=(n, 256))
    check(L.ddz_q_fc1_dense(dev.index, _p(a), n, k, _p(w), _p(c), _stream(dev)))
    return c


def q_fc1_rows(dy, seg, row_cnt, w2, z, d):
    """ddz_q_fc1_rows: d[row] = dy[row] @ w2[rank of the row] + z[rank][row_cnt[row]] for the rows / rank segments of seg
    (device int32 [40]); z f32 [15,5,256]."""
    L = _lib.lib()
    dev = _require_gpu(dy.device)
    n = int(dy.shape[0])
    _chk(dy, "dy", torch.float32, dev, shape=(n, 256))
    _chk(seg, "seg", torch.int32, dev, at_least=40)
    if (row_cnt is None) != (z is None):
        raise ValueError("row_cnt and z: both or neither")
    _chk(row_cnt, "row_cnt", torch.uint8, dev, at_least=n, none_ok=True)
    _chk(w2, "w2", torch.float32, dev, shape=(15, 256, 256))
    _chk(z, "z", torch.float32, dev, numel=75 * 256, none_ok=True, why=" ([15,5,256])")
    _chk(d, "d", torch.float32, dev, shape=(n, 256))
    check(L.ddz_q_fc1_rows(dev.index, _p(dy), _p(seg), _p(row_cnt), _p(w2), _p(z), _p(d), n, _stream(dev)))
    return d


def q_shared_ws_bytes():
    return int(_lib.lib().ddz_q_shared_ws_bytes())


def q_shared_hash_ws_bytes(n_tables):
    """workspace of the hashed row finder (BatchedEnv.q_shared_rows with variant 1 / 2) for n_tables tables"""
    n = int(_lib.lib().ddz_q_shared_hash_ws_bytes(int(n_tables)))
    if n < 0:
        raise ValueError("n_tables must be in 1 .. 2^26")
    return n


SHARED_PLANES = (6, 7, 9)    # the faces the shared-rows form keys: EnvCooperationSimplify, EnvComplicated, EnvCooperation


def shared_row_width(planes):
    """ys row width of the shared-rows form: 256 first-layer values + the 4 P column values, padded to a multiple of 16"""
    return 256 + (4 * int(planes) + 15) // 16 * 16


def q_features_rows(face, wf, bias, rep, seg, ys, mz=None, g=None):
    """ddz_q_features_rows: ys f32 [rows,256] = the first layer (count 0) of the face column of every shared row (rep: row ->
    instance 16 t + r, from BatchedEnv.q_shared_rows); face f32 [T,P,15,4], P = 6, 7 or 9; ys [rows, shared_row_width(P)]:
    + the row's column values behind the 256."""
    L = _lib.lib()
    dev, T, P = _face_arg(face, SHARED_PLANES)
    n = int(ys.shape[0])
    w_ = shared_row_width(P)
    _weight_tables(dev, P, 1, wf, bias)
    _chk(rep, "rep", torch.int32, dev, at_least=n)
    _chk(seg, "seg", torch.int32, dev, at_least=40)
    _chk(ys, "ys", torch.float32, dev, shape=(n, 256 if ys.shape[1:] == (256,) else w_), why=" (or [rows,256])")
    if (mz is None) != (g is None):
        raise ValueError("mz and g: both or neither")
    _chk(mz, "mz", torch.float32, dev, shape=(P * 60, 256), none_ok=True)
    _chk(g, "g", torch.float32, dev, shape=(n, 256), none_ok=True)
    check(L.ddz_q_features_rows(dev.index, _p(face), T, P, _p(wf), _p(bias), _p(rep), _p(seg), _p(ys), int(ys.shape[1]), n, _p(mz), _p(g),
                                _stream(dev)))
    return ys


def q_fc1_rows_k(y, seg, w2k, g, accumulate=False):
    """ddz_q_fc1_rows_k: g[row] (+)= y[row] @ w2k[rank of the row] for the rows / rank segments of seg (device int32 [40]);
    y f32 [rows,k], w2k f32 [15,k,256], k a multiple of 16."""
    L = _lib.lib()
    dev = _require_gpu(y.device)
    n, k = int(y.shape[0]), int(y.shape[1])
    _chk(y, "y", torch.float32, dev, shape=(n, k))
    _chk(seg, "seg", torch.int32, dev, at_least=40)
    _chk(w2k, "w2k", torch.float32, dev, shape=(15, k, 256))
    _chk(g, "g", torch.float32, dev, shape=(n, 256))
    check(L.ddz_q_fc1_rows_k(dev.index, _p(y), k, _p(seg), _p(w2k), _p(g), n, 1 if accumulate else 0, _stream(dev)))
    return g


def q_shared_need_ws_bytes(shared_row_capacity):
    n = int(_lib.lib().ddz_q_shared_need_ws_bytes(int(shared_row_capacity)))
    if n < 0:
        raise ValueError("the shared row capacity must be a positive multiple of the fc1 tile")
    return n


def q_features_drows(face, wf, bias, acnt, rep, drep, dseg, dy):
    """ddz_q_features_drows: dy f32 [rows,256] = Y[c] - Y[0] of the column of every shared D row (drep: D row -> 4 * shared row
    + c - 1, rep: shared row -> instance; from BatchedEnv.q_shared_need / q_shared_rows); face f32 [T,P,15,4], P = 6, 7 or 9."""
    L = _lib.lib()
    dev, T, P = _face_arg(face, SHARED_PLANES)
    n = int(dy.shape[0])
    _weight_tables(dev, P, 1, wf, bias, acnt)
    _chk(rep, "rep", torch.int32, dev)
    _chk(drep, "drep", torch.int32, dev, at_least=n)
    _chk(dseg, "dseg", torch.int32, dev, at_least=40)
    _chk(dy, "dy", torch.float32, dev, shape=(n, 256))
    check(L.ddz_q_features_drows(dev.index, _p(face), T, P, _p(wf), _p(bias), _p(acnt), _p(rep), rep.numel(), _p(drep), _p(dseg),
                                 _p(dy), n, _stream(dev)))
    return dy


def q_gather_h0(g, rows, h0, base=None):
    """ddz_q_gather_h0: h0 f32 [T,256] (+)= sum_r g[rows[t, r]] (rank order); g f32 [g_rows,256], rows int32 [T,16]; with
    base f32 [256]: h0 = base + the sum."""
    L = _lib.lib()
    dev = _require_gpu(g.device)
    T = int(h0.shape[0])
    _chk(g, "g", torch.float32, dev, shape=(g.shape[0], 256))
    _chk(rows, "rows", torch.int32, dev, shape=(T, 16))
    _chk(h0, "h0", torch.float32, dev, shape=(T, 256))
    _chk(base, "base", torch.float32, dev, numel=256, none_ok=True)
    check(L.ddz_q_gather_h0(dev.index, _p(g), int(g.shape[0]), _p(rows), T, _p(base), _p(h0), _stream(dev)))
    return h0


def q_roles_ws_bytes(n_tables, variant, n_nets):
    """workspace of BatchedEnv.q_roles_rows: n_nets times the single-network finder's"""
    n = int(_lib.lib().ddz_q_roles_ws_bytes(int(n_tables), int(variant), int(n_nets)))
    if n < 0:
        raise ValueError("n_tables in 1 .. 2^26, variant 1, 2 or 3, n_nets 1 .. 3")
    return n


def q_roles_need_ws_bytes(shared_row_capacity, n_nets):
    n = int(_lib.lib().ddz_q_roles_need_ws_bytes(int(shared_row_capacity), int(n_nets)))
    if n < 0:
        raise ValueError("the shared row capacity must be a positive multiple of the fc1 tile, n_nets 1 .. 3")
    return n


def q_roles_features_rows(face, n_nets, wf, bias, rep, seg, ys, row_capacity):
    """ddz_q_roles_features_rows: q_features_rows on every slot's partition of ys [n_nets * row_capacity, shared_row_width(P)]
    with the slot's wf [n_nets, P*4, 1024] / bias [n_nets, 1024]."""
    (dev, T, P), N = _face_arg(face, SHARED_PLANES), int(n_nets)
    _weight_tables(dev, P, N, wf, bias)
    _chk(rep, "rep", torch.int32, dev, at_least=N * int(row_capacity))
    _chk(seg, "seg", torch.int32, dev, at_least=40 * N)
    _chk(ys, "ys", torch.float32, dev, at_least=N * int(row_capacity) * int(ys.shape[-1]), why=" ([n_nets * row_capacity, width])")
    check(_lib.lib().ddz_q_roles_features_rows(dev.index, _p(face), T, P, N, _p(wf), _p(bias), _p(rep), _p(seg), _p(ys), int(ys.shape[-1]),
                                               int(row_capacity), _stream(dev)))
    return ys


def q_roles_fc1_rows_k(n_nets, y, seg, w2k, g, row_capacity):
    """ddz_q_roles_fc1_rows_k: g[row] = y[row] @ w2k[slot][rank of the row] on every slot's partition; w2k f32 [n_nets,15,k,256]."""
    dev = _require_gpu(y.device)
    N, k, rows = int(n_nets), int(y.shape[-1]), int(n_nets) * int(row_capacity)
    _chk(y, "y", torch.float32, dev, at_least=rows * k, why=" ([n_nets * row_capacity, k])")
    _chk(seg, "seg", torch.int32, dev, at_least=40 * N)
    _chk(w2k, "w2k", torch.float32, dev, numel=N * 15 * k * 256, why=" ([n_nets,15,k,256])")
    _chk(g, "g", torch.float32, dev, at_least=rows * 256, why=" ([n_nets * row_capacity, 256])")
    check(_lib.lib().ddz_q_roles_fc1_rows_k(dev.index, N, _p(y), k, _p(seg), _p(w2k), _p(g), int(row_capacity), _stream(dev)))
    return g


def q_roles_gather_h0(n_nets, g, rows, slot, base, h0):
    """ddz_q_roles_gather_h0: h0[t] = base[slot[t]] + sum_r g[rows[t, r]] (rank order); rule tables (slot < 0) left alone."""
    dev = _require_gpu(g.device)
    T = int(h0.shape[0])
    _chk(g, "g", torch.float32, dev, shape=(g.shape[0], 256))
    _chk(rows, "rows", torch.int32, dev, shape=(T, 16))
    _chk(slot, "slot", torch.int8, dev, numel=T)
    _chk(base, "base", torch.float32, dev, numel=int(n_nets) * 256)
    _chk(h0, "h0", torch.float32, dev, shape=(T, 256))
    check(_lib.lib().ddz_q_roles_gather_h0(dev.index, int(n_nets), _p(g), int(g.shape[0]), _p(rows), _p(slot), T, _p(base), _p(h0),
                                           _stream(dev)))
    return h0


def q_roles_features_drows(face, n_nets, wf, bias, acnt, rep, shared_row_capacity, drep, dseg, dy, row_capacity):
    """ddz_q_roles_features_drows: q_features_drows on every slot's partition (acnt f32 [n_nets,5,4,256])."""
    (dev, T, P), N = _face_arg(face, SHARED_PLANES), int(n_nets)
    _weight_tables(dev, P, N, wf, bias, acnt)
    _chk(rep, "rep", torch.int32, dev, at_least=N * int(shared_row_capacity))
    _chk(drep, "drep", torch.int32, dev, at_least=N * int(row_capacity))
    _chk(dseg, "dseg", torch.int32, dev, at_least=40 * N)
    _chk(dy, "dy", torch.float32, dev, at_least=N * int(row_capacity) * 256, why=" ([n_nets * row_capacity, 256])")
    check(_lib.lib().ddz_q_roles_features_drows(dev.index, _p(face), T, P, N, _p(wf), _p(bias), _p(acnt), _p(rep), int(shared_row_capacity),
                                                _p(drep), _p(dseg), _p(dy), int(row_capacity), _stream(dev)))
    return dy


def q_roles_fc1_rows(n_nets, dy, seg, row_cnt, w2, z, d, row_capacity):
    """ddz_q_roles_fc1_rows: d[row] = dy[row] @ w2[slot][rank] + z[slot][rank][row_cnt[row]] on every slot's partition."""
    dev = _require_gpu(dy.device)
    N, rows = int(n_nets), int(n_nets) * int(row_capacity)
    _chk(dy, "dy", torch.float32, dev, at_least=rows * 256, why=" ([n_nets * row_capacity, 256])")
    _chk(seg, "seg", torch.int32, dev, at_least=40 * N)
    _chk(row_cnt, "row_cnt", torch.uint8, dev, at_least=rows)
    _chk(w2, "w2", torch.float32, dev, numel=N * 15 * 256 * 256, why=" ([n_nets,15,256,256])")
    _chk(z, "z", torch.float32, dev, numel=N * 75 * 256, why=" ([n_nets,15,5,256])")
    _chk(d, "d", torch.float32, dev, at_least=rows * 256, why=" ([n_nets * row_capacity, 256])")
    check(_lib.lib().ddz_q_roles_fc1_rows(dev.index, N, _p(dy), _p(seg), _p(row_cnt), _p(w2), _p(z), _p(d), int(row_capacity),
                                          _stream(dev)))
    return d


def action_table(device="cuda:0", native_joker_kickers=False):
    """The canonical action table on the device: int8 [n_actions, 16] = counts[15] + category, action id =
    row index (the order of card.py:34-159 get_action_space(); + the 24 joker-kicker rows if asked for)."""
    L = _lib.lib(jk=native_joker_kickers)
    dev = _require_gpu(device)
    rows = torch.empty((L.ddz_num_actions(), ROW), dtype=torch.int8, device=dev)
    check(L.ddz_action_table(dev.index, _p(rows), _stream(dev)))
    return rows


TRAJ_PACKED_BYTES = 8


def pack_trajectory(traj, native_joker_kickers=False):
    """uint8 [..., 32] trajectory records -> uint8 [..., 8] (include/ddz_env.h ddz_pack_trajectory): the action
    as its canonical id.  What dist.gather_trajectories(compact=True) sends over xGMI."""
    L = _lib.lib(jk=native_joker_kickers)
    dev = _require_gpu(traj.device)
    if traj.dtype != torch.uint8 or traj.shape[-1] != TRAJ_BYTES:
        raise ValueError("traj must be uint8 [..., 32]")
    traj = traj.contiguous()
    n = traj.numel() // TRAJ_BYTES
    out = torch.empty(traj.shape[:-1] + (TRAJ_PACKED_BYTES,), dtype=torch.uint8, device=dev)
    check(L.ddz_pack_trajectory(dev.index, _p(traj), n, _p(out), _stream(dev)))
    return out


def _hands_lasts(hands, lasts, dev):
    """the queries of the stateless verbs: count rows of any integer type, [n,15] or [n,16], as int8 [n,16] on `dev` each -> (hands,
    lasts, n)"""
    def pad(x, name, n):
        x = x.to(device=dev, dtype=torch.int8)
        if x.dim() == 2 and x.shape[1] == 15:
            x = torch.nn.functional.pad(x, (0, 1))
        return _chk(x.contiguous(), name, torch.int8, dev, shape=(n, ROW), why=" (or [n,15])")

    n = len(hands)
    return pad(hands, "hands", n), pad(lasts, "lasts", n), n


def get_moves(hands, lasts, want_ids=True, row_capacity=None, native_joker_kickers=False):
    """Batched r.get_moves(hand15, last15) (envi.py:111): hands/lasts int8 [n,15|16] on the
    GPU.  Returns (offsets[n+1] i32, rows[total,16] i8, ids[total] i32 | None); one host sync
    to trim the outputs.  native_joker_kickers: see BatchedEnv."""
    L = _lib.lib(jk=native_joker_kickers)
    NUM_ACTIONS = L.ddz_num_actions()
    dev = _require_gpu(hands.device)
    hands, lasts, n = _hands_lasts(hands, lasts, dev)
    cap = int(row_capacity) if row_capacity is not None else min(n * NUM_ACTIONS, 0x7FFFFFFF)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    scratch = torch.zeros(L.ddz_scratch_bytes(n), dtype=torch.uint8, device=dev)

    def run(capacity):
        rows = torch.empty((max(capacity, 1), ROW), dtype=torch.int8, device=dev)
        ids = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev) if want_ids else None
        check(L.ddz_get_moves(dev.index, _p(hands), _p(lasts), n, _p(offsets), _p(rows), _p(ids),
                              capacity, _p(scratch), scratch.numel(), _stream(dev)))
        return rows, ids

    if row_capacity is None and n * NUM_ACTIONS > (1 << 22):
        run(0)  # sizes only: offsets are exact whatever the capacity
        cap = int(offsets[-1].item())
        scratch.zero_()
    rows, ids = run(cap)
    total = int(offsets[-1].item())
    if total > cap:
        raise DdzError(f"row capacity {cap} too small for {total} rows")
    bad = int(scratch.view(torch.int32)[(scratch.numel() - 256) // 4].item()) & 4
    if bad:
        raise ValueError("a `last` vector is not a combo of the action space")
    return offsets, rows[:total], (ids[:total] if want_ids else None)


def auto_choose(hands, lasts, left, role, want_stats=False):
    """RuleBasedModel.choose for n independent queries (what server/core.py:80-87 calls on a payload): hands / lasts
    int8 [n,15|16] (last all-zero = lead), left int [n,3] = cards left of role 0 up / 1 lord / 2 down, role int [n].
    Returns int32[n] canonical action ids (0 = pass, -2 = invalid query) (and int64 [n,2] {combinations, nodes})."""
    L = _lib.lib()
    dev = _require_gpu(hands.device)
    hands, lasts, n = _hands_lasts(hands, lasts, dev)
    info = torch.zeros((n, 4), dtype=torch.uint8, device=dev)
    info[:, :3] = torch.as_tensor(left, device=dev).reshape(n, 3).to(torch.uint8)
    info[:, 3] = torch.as_tensor(role, device=dev).reshape(n).to(torch.uint8)
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.zeros((n, 2), dtype=torch.int64, device=dev) if want_stats else None
    check(L.ddz_auto_choose(dev.index, _p(hands), _p(lasts), _p(info), n, _p(ids), _p(stats), _stream(dev)))
    return (ids, stats) if want_stats else ids


def device_status(device="cuda:0"):
    """Status bits of the stateless rule-agent launches on this device since the last call (ddz_device_status; bit 3 = a
    cooperating wait hit its hang guard: do not trust those ids); host sync, clears the word."""
    L = _lib.lib()
    dev = _require_gpu(device)
    out = C.c_int32(0)
    check(L.ddz_device_status(dev.index, C.byref(out), _stream(dev)))
    return out.value


def cards_value(device="cuda:0"):
    """cards_value of rule_based/utils/evaluator.py:10-47 for every action id, float64 [13527] (device test hook)."""
    L = _lib.lib()
    dev = _require_gpu(device)
    out = torch.empty(NUM_ACTIONS, dtype=torch.int8, device=dev)
    check(L.ddz_debug_cards_value(dev.index, _p(out), _stream(dev)))
    return out.to(torch.float64) / 2.0


def get_moves_slab(hands, lasts, want_ids=True, native_joker_kickers=False, out=None):
    """Batched r.get_moves(hand15, last15) in the slab layout, ONE launch and no host sync: returns (counts int32 [n],
    rows int8 [n, 512, 16], ids int32 [n, 512] | None, status int32 [1]); query i's moves are rows[i, :counts[i]] in
    ascending canonical id (pass first when following); status bit 2 = some `last` was no combo (its list is empty).
    `out` = a previous result to write into (no allocation)."""
    L = _lib.lib(jk=native_joker_kickers)
    dev = _require_gpu(hands.device)
    hands, lasts, n = _hands_lasts(hands, lasts, dev)
    if out is None:
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        rows = torch.empty((n, MAX_LEGAL_PER_TABLE, ROW), dtype=torch.int8, device=dev)
        ids = torch.empty((n, MAX_LEGAL_PER_TABLE), dtype=torch.int32, device=dev) if want_ids else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        counts, rows, ids, status = out
        _chk(counts, "counts", torch.int32, dev, numel=n, why=" (out[0])")
        _chk(rows, "rows", torch.int8, dev, numel=n * MAX_LEGAL_PER_TABLE * ROW, why=" (out[1])")
        _chk(ids, "ids", torch.int32, dev, numel=n * MAX_LEGAL_PER_TABLE, none_ok=True, why=" (out[2])")
        _chk(status, "status", torch.int32, dev, numel=1, why=" (out[3])")
        status.zero_()
    check(L.ddz_get_moves_slab(dev.index, _p(hands), _p(lasts), n, _p(counts), _p(rows), _p(ids), MAX_LEGAL_PER_TABLE,
                               _p(status), _stream(dev)))
    return counts, rows, ids, status
