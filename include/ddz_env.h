/*
 * ddz_env.h -- C ABI of libddz_hip.so, the MI355X (gfx950) batched Doudizhu engine.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json:north_star:
 * what the reference reaches through its (absent) pybind modules `env` and `r`
 * (envi.py:10-13) plus the per-game Python adapter envi.py, re-cut as batched
 * verbs over T independent tables.  Plain pointers and sizes only: every buffer
 * is DEVICE memory owned by the caller (PyTorch tensors in the host mirror
 * doudizhu-rl_amd/envi.py); the library allocates nothing on the device, never
 * synchronises, and enqueues all work on the hipStream_t passed as `stream`
 * (void* so that this header needs no HIP include).  All entry points return 0
 * or a negative DDZ_E* code and never throw.  A handle is not thread-safe.
 *
 * Reference citations are relative to /root/reference.
 */
#ifndef DDZ_ENV_H
#define DDZ_ENV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDZ_ABI_VERSION 1
#define DDZ_NUM_ACTIONS 13527 /* rule_based/utils/card.py:34-159 */
/* Optional rule-set extension, a second build of the same source (libddz_hip_jk.so,
 * -DDDZ_NATIVE_JOKER_KICKERS=1; default library: off).  It adds the 24 vectors that card.py:116,142 exclude
 * but the reference's native r.get_moves is known to return -- server/mcts/get_moves.py:22-34 builds
 * exactly them ("sidaihuojian": quad + both jokers, 13; "sandaihuojian": two consecutive triples + both
 * jokers, 11) to filter them out.  Ids 13527 + quad rank (category FOUR_TAKE_ONE) and 13540 + start rank
 * (category THREE_ONE_LINE, len 2): last in every list.  ddz_num_actions() tells the builds apart.     */
#define DDZ_ROW 16            /* packed row: int8 counts[15] (3..K,A,2,BJ,CJ; envi.py:122-124) + 1 aux byte */
#define DDZ_NFIELDS 11
#define DDZ_TRAJ_BYTES 32
/* slab list layout: rows per table.  497 = the largest legal list of any hand of <= 20 cards, proven by exhaustive
 * enumeration of every 20-card hand (tools/max_legal_bound.c, tests/test_rules_bounds.py); the joker-kicker rule set
 * adds at most 24 rows to a list and the same exhaustive run (built with -DDDZ_JK_RULES) proves its maximum too: also 497 (the worst hands hold no jokers).
 * Smaller strides are DDZ_EINVAL. */
#define DDZ_SLAB_MIN_STRIDE 512

/* error codes */
#define DDZ_OK 0
#define DDZ_EINVAL (-1)   /* bad argument / shape / null pointer          */
#define DDZ_EHANDLE (-2)  /* bad or destroyed handle                       */
#define DDZ_EHIP (-3)     /* a HIP runtime call failed (see ddz_last_hip_error) */
#define DDZ_ECAP (-4)     /* row capacity cannot be indexed with int32     */
#define DDZ_ENODEV (-5)   /* no usable gfx950 device                       */

/* state fields: state is uint8 [T][DDZ_NFIELDS][16], table-major (the 11 rows of a table are 176 contiguous bytes).
 *   0..2  hand of role 0 up / 1 lord / 2 down (envi.py:24); byte 15 = cards left (envi.py:23)
 *   3..5  history: cumulative cards played by the role (envi.py:41)
 *   6..8  recent_handout of the role, zeros for a pass (envi.py:43); byte 15 = category
 *   9     taken: all cards played (envi.py:40)
 *   10    meta: [0] role to move, [1] done, [2] winner (0xFF running), [3] i8 last r,
 *               [4..5] u16 ply, [6] dealt, [8..11] u32 episode
 * A count byte (bytes 0..14 of rows 0..9) is at most 15.  The rollouts carry the table as nibbles: of a larger
 * count byte in an imported state they see, and write back, the low four bits only.  Byte 15 of every row is
 * kept exactly.                                                                              */
enum { DDZ_F_HAND0 = 0, DDZ_F_HIST0 = 3, DDZ_F_RECENT0 = 6, DDZ_F_TAKEN = 9, DDZ_F_META = 10 };

/* step modes */
#define DDZ_STEP_RANDOM 0 /* uniform index into the legal list, engine RNG   (envi.py:79-85 step_random) */
#define DDZ_STEP_CHOICE 1 /* sel = const int32_t[T], index into each table's legal segment              */
#define DDZ_STEP_ROWS 2   /* sel = const int8_t[T][16] count rows (envi.py:63-70 step_manual), validated
                             against the legal segment; no match -> illegal flag, table untouched       */
#define DDZ_STEP_IDS 3    /* sel = const int32_t[T] canonical action ids (index into card.py:get_action_space();
                             what ddz_auto_choose_state writes, or the arg-max of a policy head over
                             ddz_legal_mask), validated like ROWS; -1 = engine RNG for that table (RANDOM);
                             any other value that is no action id (DDZ_AUTO_INVALID) -> illegal flag         */
#define DDZ_AUTO_INVALID (-2) /* ddz_auto_choose[_state]: the query was invalid (no combo, role > 2, > 20 cards)   */

/* face variants (envi.py:87-96, :165-178, :182-198, :202-217) -> planes P = 4, 7, 9, 6 */
#define DDZ_FACE_ENV 0
#define DDZ_FACE_COMPLICATED 1
#define DDZ_FACE_COOPERATION 2
#define DDZ_FACE_COOPERATION_SIMPLIFY 3

typedef struct ddz_env ddz_env_t;

int ddz_abi_version(void);
int ddz_num_actions(void); /* 13527 (default) or 13551 (joker-kicker build) */
const char* ddz_strerror(int code);
/* last hipError_t seen by this library on the calling thread (0 = hipSuccess) */
int ddz_last_hip_error(void);

/* sizes of the caller-owned device buffers for T tables */
int64_t ddz_state_bytes(int64_t n_tables);   /* DDZ_NFIELDS * T * 16 */
int64_t ddz_scratch_bytes(int64_t n_tables); /* per-table query records, counts, scan partials, status */
int ddz_face_planes(int variant);            /* 4 / 7 / 9 / 6, or DDZ_EINVAL */

/* Replaces `Env(seed=)` construction (envi.py:17-28): binds caller-owned device
 * buffers to a handle.  `state` must be zero-filled (or hold an exported state);
 * table t of this handle is global table `table_id_base + t` for the RNG, so a
 * sharded run deals the same cards whatever the GPU count.                      */
int ddz_create(ddz_env_t** out, int64_t n_tables, uint64_t seed, uint64_t table_id_base,
               int device_id, void* state, int64_t state_bytes, void* scratch,
               int64_t scratch_bytes);
int ddz_destroy(ddz_env_t* env);
/* tell the engine that `state` was overwritten behind its back (checkpoint load) */
int ddz_invalidate(ddz_env_t* env);

/* Replaces Env.reset() + native prepare() (envi.py:30-36, game.py:170-171): clear the
 * bookkeeping and deal 17/20/17 (lord = role 1 moves first) for every table whose mask
 * byte is non-zero (mask NULL = all).  Deal/RNG = spec v2.                */
int ddz_reset(ddz_env_t* env, const uint8_t* table_mask, void* stream);

/* Replaces Env.valid_actions(tensor=False) / r.get_moves (envi.py:98-116) for all tables:
 * CSR list in ascending canonical action id (pass first when following).
 *   offsets int32[T+1]; rows int8[row_capacity][16] (byte 15 = category);
 *   ids int32[row_capacity] canonical action ids, may be NULL.
 * Writes beyond row_capacity are dropped and status bit 1 is raised.                  */
int ddz_legal(ddz_env_t* env, int32_t* offsets, int8_t* rows, int32_t* ids,
              int64_t row_capacity, void* stream);

/* Replaces Env.step_manual / step_random (+ _update) and the native step
 * (envi.py:38-43, 63-70, 79-85): apply one action per table, taken from the CSR list
 * produced by ddz_legal for the *current* state.  Outputs may be NULL:
 *   done u8[T]; reward i8[T] (-1 lord won, +1 farmers won, 0 running: rule_play.py:14);
 *   illegal u8[T]; traj u8[T][32].  With auto_reset a finished table is
 *   re-dealt inside the same call (episode + 1).                                       */
int ddz_step(ddz_env_t* env, int mode, const void* sel, const int32_t* offsets,
             const int8_t* rows, int auto_reset, uint8_t* done, int8_t* reward,
             uint8_t* illegal, uint8_t* traj, void* stream);

/* get_mask (rule_based/utils/utils.py:45-63) for every table: the legal moves as a dense 0/1 mask over the
 * action space (bit id; bit 0 = pass, forced 0 on lead), bit-packed into ddz_mask_words() = 424 uint32 per table
 * (bit id & 31 of word id >> 5; the tail bits are 0).  mask: [T][424] uint32, device memory.                  */
int ddz_mask_words(void);
int ddz_legal_mask(ddz_env_t* env, uint32_t* mask, void* stream);

/* Slab variant of ddz_legal / ddz_step (fixed-stride list layout, as ddz_rollout_random uses): table t owns
 * rows[t * stride ... t * stride + counts[t]).  Without the CSR prefix there is no dependency between tables,
 * so ONE launch per lock-step iteration does both halves of the reference's loop body (game.py:95-106 +
 * envi.py:98-116): ddz_step_slab applies the selections -- indices into (CHOICE) or rows of (ROWS) the lists that
 * are in the buffers -- and overwrites them with the lists of the new states.  ddz_legal_slab fills the buffers
 * for the current states (after ddz_reset / ddz_create / a state import).  stride >= 512 holds any list of a
 * <= 20-card hand; a list that does not fit raises status bit 1 and is reported empty.                       */
int ddz_legal_slab(ddz_env_t* env, int32_t* counts, int8_t* rows, int32_t* ids, int64_t stride, void* stream);
int ddz_step_slab(ddz_env_t* env, int mode, const void* sel, int32_t* counts, int8_t* rows, int32_t* ids,
                  int64_t stride, int auto_reset, uint8_t* done, int8_t* reward, uint8_t* illegal, uint8_t* traj,
                  void* stream);

/* The environment side of one lock-step iteration of a value-based policy in ONE launch (game.py:95-104 with
 * dqn.py:50-71): choose each table's move as the (epsilon-)greedy arg-max of q over its current slab list
 * (= ddz_select_slab: q f32 [T][stride], first maximum, engine RNG domain 3), apply it (= ddz_step_slab CHOICE), write the
 * lists of the new states and -- face != NULL -- their `face` tensors (= ddz_observe(face_variant): f32 [T][P][15][4]).
 * choice (may be NULL) receives the selected list indices.  Bit-identical to the three separate calls.          */
int ddz_policy_step_slab(ddz_env_t* env, const float* q, double epsilon, int32_t* counts, int8_t* rows, int32_t* ids,
                         int64_t stride, int auto_reset, uint8_t* done, int8_t* reward, uint8_t* illegal, uint8_t* traj,
                         int32_t* choice, int face_variant, float* face, void* stream);

/* Slab lists -> CSR (what ddz_legal writes, what a ragged NN forward over all legal moves consumes): offsets
 * int32[T+1], rows_out int8[row_capacity][16], ids_out int32[row_capacity] (NULL: no ids).  The prefix-sum compaction of
 * the variable-length lists as its own cheap pass (two small launches), so that ddz_step_slab / ddz_rollout_random
 * never wait on a scan over all tables: legal lists in CSR order cost ddz_step_slab + this instead of ddz_legal +
 * ddz_step.  A list index is the same in both layouts (ddz_select's choice feeds ddz_step_slab CHOICE).  Rows beyond
 * row_capacity are dropped and status bit 1 is raised; the offsets written are clamped to row_capacity, so every
 * segment [offsets[t], offsets[t+1]) stays inside rows_out (truncated lists are shorter or empty, never out of bounds). */
int ddz_slab_to_csr(ddz_env_t* env, const int32_t* counts, const int8_t* rows, const int32_t* ids, int64_t stride,
                    int32_t* offsets, int8_t* rows_out, int32_t* ids_out, int64_t row_capacity, void* stream);

/* Replaces the `face` property of the four Env classes: f32 [T][P][15][4].            */
int ddz_observe(ddz_env_t* env, int variant, float* face, void* stream);

/* What an agent reads per ply -- `face` (envi.py:87-96,165-217) and valid_actions(tensor=True) (envi.py:98-116) -- in ONE
 * call: ddz_observe(env, variant, face) followed by ddz_rows_to_onehot(rows, n, onehot) on the same stream (n = 0: the
 * face only).  The N = 1 `Env` view's per-ply call; the two launches are the ones of the separate entry points.        */
int ddz_observe_actions(ddz_env_t* env, int variant, float* face, const int8_t* rows, int64_t n, float* onehot, void* stream);

/* ddz_observe on state rows that are not an environment's (handle-free): face f32 [n][P][15][4] of the 176-byte rows
 * states[index[i]] (index int64[n], DEVICE memory; NULL = identity), the same expression, bit for bit.  What rebuilds the
 * s0 / s1 faces of a replay batch from the packed rings below.  Every index must name a row of `states` (the caller's
 * bound: the library does not know how many rows there are); a negative one reads row 0.                             */
int ddz_observe_states(int device_id, const uint8_t* states, const int64_t* index, int64_t n, int variant, float* face,
                       void* stream);

/* The learner's half of Game.train on the device (game.py:90-167, dqn.py:21-48; doudizhu-rl_amd/csrc/ddz_replay.h): the
 * bookkeeping of dqn_glue.TransitionAssembler + one Replay per role (dqn.py:14), with a transition kept PACKED as two state
 * rows, two canonical action ids, reward, done and the table (369 bytes; the faces are a function of the rows:
 * ddz_observe_states).  Nothing crosses to the host, every launch goes to `stream`, the counts stay in device memory; both
 * calls can be captured in a graph.
 *   ws: the recorder's state, ddz_tr_ws_bytes(T) bytes (a multiple of 256; 548 bytes per table + a little), 16-byte
 *     aligned, ZERO-FILLED by the caller before the first call (= nothing pending, every table fresh).
 *   rings: HOST array of three device pointers in role order (0 up, 1 lord, 2 down), each a ring of `capacity` entries:
 *     ddz_tr_ring_bytes(capacity) bytes (ring_bytes = the size of each), 16-byte aligned, zero-filled; NULL = that role
 *     records nothing (a role named in trained_roles must have one).  Fields at the byte offsets ddz_tr_ring_layout writes
 *     into offsets[8] (HOST): count int64 (total ever written), s0 u8[capacity][176], s1, a0 int32[capacity], a1, reward
 *     f32[capacity], table int32[capacity], done u8[capacity].  The transition with sequence number s is entry s % capacity.
 *   ddz_tr_before (TransitionAssembler.before_step; call it BEFORE the step, on the states the actors chose on): for every
 *     table that is active (active u8[T], NULL = all) and whose actor's role is in trained_roles (bit r = role r): if the
 *     role's slot is pending and the table is not fresh (a ply of its episode was played), the role's ring gets (s0, a0 of
 *     the slot, reward 0, s1 = the state now, a1 = greedy[t], done 0); then the slot takes (the state now, chosen[t]) and
 *     is pending.  Every active table stops being fresh.  chosen / greedy: int32[T] canonical action ids.
 *   ddz_tr_after (TransitionAssembler.after_step; call it AFTER the step, before the re-deal: no auto-reset): for every table
 *     with done[t] != 0, every pending role's ring gets (s0, a0 of its slot, +reward[role] if its side won, else
 *     -reward[role]; s1 = the state now, a1 = 0 = the pass, whose thermometer is the all-zero a1 of game.py:123; done 1).
 *     r i8[T] as ddz_step writes it (< 0: the lord won; the two farmers are one side); reward: HOST float[3] in role order.
 *     The table's pending bits are cleared unless replicate_reference_quirk (game.py never clears *_s0 / *_a0: the first
 *     feedback of down and up in the next episode then closes a transition across the re-deal), and it is fresh again.
 *   Order: emit g of a call into a ring, g = the number of lower-numbered tables that emit into that ring in this call (a
 *     scan over the tables, no atomics), gets sequence number count + g.  A call that emits E > capacity into one ring writes
 *     the last `capacity` of them only, at count .. count + capacity - 1, and count moves by capacity: what Replay.push keeps
 *     and where it puts it.  No two lanes of a launch store to one entry.
 *   A role byte above 2 (a corrupted import; every other entry point reads it as role 0): the table takes no part in
 *     ddz_tr_before -- nothing is recorded, its slots and flags are left alone, it does not stop being fresh -- because a
 *     slot is addressed by the role.  ddz_tr_after does not read the role byte.
 *   A NULL ring for a role that is pending on a finished table (ddz_tr_after names no trained roles): that role's terminal
 *     transition is dropped; the table's flags move as they do with a ring.
 *   A count the caller did not zero: any int64 is taken as it stands, sequence number s lives at entry s mod capacity with
 *     the non-negative remainder, so a negative count still stores inside the ring.
 *   Both calls store to the entries named above and to nothing else of a ring: an entry that takes no emit, and the padding
 *     between the fields, keep their bytes.  (tests/test_gpu_recorder_cases.py)                                      */
int64_t ddz_tr_ws_bytes(int64_t n_tables);
int64_t ddz_tr_ring_bytes(int64_t capacity);
int ddz_tr_ring_layout(int64_t capacity, int64_t* offsets);
int ddz_tr_before(ddz_env_t* env, void* ws, int64_t ws_bytes, void* const* rings, int64_t ring_bytes, int64_t capacity,
                  const int32_t* chosen, const int32_t* greedy, const uint8_t* active, int trained_roles, void* stream);
int ddz_tr_after(ddz_env_t* env, void* ws, int64_t ws_bytes, void* const* rings, int64_t ring_bytes, int64_t capacity,
                 const uint8_t* done, const int8_t* r, const float* reward, int replicate_reference_quirk, void* stream);

/* Monte-Carlo return targets (return spec v1; doudizhu-rl_amd/csrc/ddz_returns.h; dqn_glue.ReturnAssembler is the
 * host statement): a decision is regressed onto its own episode's return instead of r + gamma * Q_target(s1, a1).  Two calls
 * around the step of a lock-step iteration, used exactly as ddz_tr_before / ddz_tr_after are: on the caller's stream, nothing
 * on the host, no atomics, capturable in a graph, deterministic.
 *   ws: caller-owned, 16-byte aligned, ZERO-FILLED before the first call, ddz_mc_ws_bytes(T, log_cap) bytes (a multiple of
 *     256; log_cap in 1..255 entries per table, T * log_cap <= 2^30; about 182 bytes per log entry).  Per table: an episode
 *     log of log_cap entries (state row uint4[11], a0 int32, role u8, ordinal u8), the count n of its entries, a decision
 *     counter per role c[3] (u8, saturating) and a cumulative counter `lost` (u32, saturating) of the decisions that were not
 *     logged because the log was full; then the per-call scratch of the scan and hdr int64[8] with the meaning
 *     ddz_replay.h gives it: [k] the sequence number of ring k's emit 0, [4 + k] the emits dropped in front.
 *     ddz_mc_ws_layout writes the byte offsets of the regions into offsets[8] (HOST): rows u8[T][log_cap][176], act
 *     int32[T][log_cap], who u8[T][log_cap][2] = {role, ordinal}, cnt u8[T][4] = {n, c[3]}, lost uint32[T], rank int32[T][4],
 *     blk int32[nb][4], hdr int64[8] (what a caller needs to forget the logs of tables it re-deals itself: zero their cnt).
 *   rings: HOST array of three device pointers in role order (0 up, 1 lord, 2 down), each ddz_mc_ring_bytes(capacity) bytes
 *     (ring_bytes = the size of each), 16-byte aligned, zero-filled; NULL = that role's emits are dropped (and counted in
 *     hdr[4 + k]).  Fields at the byte offsets ddz_mc_ring_layout writes into offsets[6] (HOST), each 256-aligned: count
 *     int64 (total ever written), s0 u8[capacity][176], a0 int32[capacity], ret f32[capacity], table int32[capacity], togo
 *     u8[capacity].  The entry with sequence number s is entry s % capacity.
 *   ddz_mc_before (call it BEFORE the step, on the states the actors chose on): for every table whose role byte is <= 2, that
 *     is active (active u8[T], NULL = all) and whose role is in trained_roles (bit r = role r): if n < log_cap the log takes
 *     (the state row now, chosen[t], role, ordinal = c[role]) at position n and n goes up, otherwise lost goes up; in both
 *     cases c[role] goes up.  A role byte above 2 takes no part, as in ddz_tr_before.  chosen: int32[T] canonical action ids.
 *   ddz_mc_after (call it AFTER the step, before the re-deal: no auto-reset): for every table with done[t] != 0, every log
 *     entry in ascending position, with role k and ordinal j, emits into ring k: s0 = the logged row, a0 = the logged action,
 *     table = t, togo = c[k] - 1 - j, ret = g after togo steps of g <- g * gamma in f32 from g = +reward[k] if role k's side
 *     won, else -reward[k] (r i8[T] as ddz_step writes it, < 0: the lord won; the two farmers are one side -- exactly as
 *     ddz_tr_after decides it; reward: HOST float[3] in role order).  Repeated f32 multiplication, not powf: a host
 *     reproduces ret bit for bit.  Then n and c of the table return to zero; lost stays.
 *   Order of a call's emits into a ring: ascending table, within a table ascending log position; emit g gets sequence number
 *     count + g.  Overflow as ddz_tr_after: a call that emits E > capacity into one ring writes its last `capacity` only, the
 *     earlier ones take no sequence number and are counted in hdr[4 + k].  No two lanes store to one entry.  Entries that take
 *     no emit, and the padding between the fields, keep their bytes.
 *   When the log overflowed: togo counts the role's later decisions whether or not they were logged, so with the reference's
 *     gamma ret is what the reference's own chain of transitions gives the decision under y_i = r_i + (1 - done_i) * gamma *
 *     y_{i+1}; with gamma = 1 it is the Deep Monte Carlo target.                       (tests/test_gpu_return_recorder.py) */
int64_t ddz_mc_ws_bytes(int64_t n_tables, int log_cap);
int ddz_mc_ws_layout(int64_t n_tables, int log_cap, int64_t* offsets);
int64_t ddz_mc_ring_bytes(int64_t capacity);
int ddz_mc_ring_layout(int64_t capacity, int64_t* offsets);
int ddz_mc_before(ddz_env_t* env, void* ws, int64_t ws_bytes, int log_cap, const int32_t* chosen, const uint8_t* active,
                  int trained_roles, void* stream);
int ddz_mc_after(ddz_env_t* env, void* ws, int64_t ws_bytes, int log_cap, void* const* rings, int64_t ring_bytes,
                 int64_t capacity, const uint8_t* done, const int8_t* r, const float* reward, float gamma, void* stream);

/* Teacher targets (teacher spec v1; doudizhu-rl_amd/csrc/ddz_teach.h; dqn_glue.TeacherAssembler is the host
 * statement): the root statistics of an evaluator -- a wins count per move of every table's slab list, counted for the root
 * actor's side, beside a visit count per move or a total per table -- become entries of the return rings above, one per
 * qualifying move of every selected table, with the value of the move as the regression target.  One call, on the caller's
 * stream, nothing on the host, no atomics, capturable in a graph, deterministic; the env is only read.
 *   counts int32[T], ids int32[T * stride]: a slab list as ddz_legal_slab wrote it, or any arrays of that shape (the caller
 *     passes them, as to ddz_playout_choose).  stride >= 1 (only the caller's arrays are read, so DDZ_SLAB_MIN_STRIDE is not
 *     required); T * stride < 2^31 (else DDZ_ECAP).
 *   num, den, unknown: int32[T * stride].  den == NULL: every entry's denominator is den_const (ddz_playout's n_playouts,
 *     ddz_solve's worlds).  unknown may be NULL; where given it is subtracted from the denominator (ddz_solve's unknown worlds).
 *   scale: the unit num is counted in -- 1, or DDZ_GUIDED_ONE for ddz_guided_close's wins.  1 <= scale <= 1024, 1 <= min_den.
 *   active u8[T] or NULL (all); trained_roles: bit r = role r.
 *   ws: per-call scratch, 16-byte aligned, ddz_teach_ws_bytes(T) bytes, nothing in it has to be initialised.
 *     ddz_teach_ws_layout writes the byte offsets of its regions into offsets[3] (HOST): rank int32[T][4], blk int32[nb][4]
 *     (nb = ceil(T / 256)), hdr int64[8].  After the call hdr[k] is the sequence number of ring k's emit 0 and hdr[4 + k] the
 *     emits dropped in front, k = 0..2, as ddz_mc_after leaves them (hdr[3] and hdr[7] are not written).
 *   rings, ring_bytes, capacity, reward: exactly ddz_mc_after's -- three device pointers in role order, each
 *     ddz_mc_ring_bytes(capacity) bytes with the fields of ddz_mc_ring_layout, or NULL: that role's emits are dropped and
 *     counted in hdr[4 + k]; reward: HOST float[3] in role order.
 *   Which tables emit: table t with role byte k takes part when k <= 2, active is NULL or active[t] != 0, bit k of
 *     trained_roles is set and counts[t] > 0.
 *   Which entries emit: for j < min(counts[t], stride), d = (den ? den[t * stride + j] : den_const) - (unknown ?
 *     unknown[t * stride + j] : 0), computed in 64 bits; the entry emits when d >= min_den.  num is not validated.
 *   The emitted entry, into ring k: s0 = the 176-byte state row of t, a0 = ids[t * stride + j], table = t, togo = 0,
 *     ret = reward[k] * ((float)(2 * (int64)num - p) / (float)p) with p = d * scale (int64): two round-to-nearest int64 -> f32
 *     conversions, one IEEE f32 division, one f32 multiplication, so a host reproduces ret bit for bit.  A move that wins every
 *     playout gets +reward[k], one that loses every playout -reward[k]: the scale of ddz_mc_after's targets.
 *   Order and overflow as ddz_mc_after: emit g of a call into ring k, counted by ascending table, then ascending j, gets
 *     sequence number count + g and lives at entry s % capacity; of E > capacity emits only the last `capacity` are written,
 *     the earlier ones take no sequence number and are counted in hdr[4 + k].  No two lanes store to one entry; entries that
 *     take no emit, and the padding between the fields, keep their bytes.
 *   Errors, all from the host before any launch: DDZ_EINVAL for a NULL or misaligned pointer, stride < 1, scale outside
 *     1..1024, min_den < 1, den == NULL with den_const < 1, bits above 2 in trained_roles, a bad capacity or short ring;
 *     DDZ_ECAP for a workspace shorter than ddz_teach_ws_bytes(T).                          (tests/test_gpu_teach.py) */
int64_t ddz_teach_ws_bytes(int64_t n_tables);
int ddz_teach_ws_layout(int64_t n_tables, int64_t* offsets);
int ddz_teach(ddz_env_t* env, const int32_t* counts, const int32_t* ids, int64_t stride, const int32_t* num, const int32_t* den,
              int32_t den_const, const int32_t* unknown, int32_t scale, int32_t min_den, const uint8_t* active, int trained_roles,
              void* ws, int64_t ws_bytes, void* const* rings, int64_t ring_bytes, int64_t capacity, const float* reward,
              void* stream);

/* Replaces the native get_state_prob_manual(known60, size1, size2) (server/core.py:26-33; Env.get_state_prob(),
 * envi.py:94, is the same function of the live table): known60 u8[n][60] = thermometer of the cards the actor can see
 * (own hand + everything played), sizes int32[n][2] = cards left of the next and the next-but-one player;
 * out f32[n][2][15][4] = the two probability planes of `face` (prob planes spec v1, DESIGN.md 4: PARITY UNPINNED,
 * bit-identical to the last two planes ddz_observe writes for the same table).                                  */
int ddz_state_prob(int device_id, const uint8_t* known60, const int32_t* sizes, int64_t n, float* out, void* stream);

/* Replaces batch_arr2onehot (envi.py:139-146) on device: rows int8[n][16] -> f32 [n][15][4] */
int ddz_rows_to_onehot(int device_id, const int8_t* rows, int64_t n, float* out, void* stream);

/* Replaces r.get_moves(hand15, last15) (envi.py:111, server/core.py:65, server/CFR.py:55)
 * for n independent queries: hands/lasts int8[n][16] (byte 15 ignored; `last` all-zero =
 * lead; a `last` that is no combo of the action space yields an empty list and status
 * bit 2).  scratch: ddz_scratch_bytes(n) bytes, zero-filled by the caller; its status
 * word (bits as ddz_status) is the int32 at byte ddz_scratch_bytes(n) - 256.           */
int ddz_get_moves(int device_id, const int8_t* hands, const int8_t* lasts, int64_t n,
                  int32_t* offsets, int8_t* rows, int32_t* ids, int64_t row_capacity,
                  void* scratch, int64_t scratch_bytes, void* stream);

/* ddz_get_moves in the slab layout (as ddz_legal_slab): query i owns rows[i * stride ... i * stride + counts[i]),
 * ascending canonical id, pass first when following; stride >= DDZ_SLAB_MIN_STRIDE.  ONE launch, no scratch, no size
 * pass: the low-latency form for a serving path (server/core.py:56-67 valid_actions).  status (device int32, may be
 * NULL) gets bit 2 when a `last` is no combo of the action space (that query's list is empty) and bit 1 when a list
 * does not fit (a hand of more than 20 cards can have more than 512 moves: use ddz_get_moves for those).            */
int ddz_get_moves_slab(int device_id, const int8_t* hands, const int8_t* lasts, int64_t n, int32_t* counts, int8_t* rows,
                       int32_t* ids, int64_t stride, int32_t* status, void* stream);

/* The lock-step loop of Game.play under a random policy (game.py:169-181 with
 * envi.py:79-85): n_iters iterations of {legal list, step_random(auto_reset)} in ONE kernel
 * launch.  The lists are written in the SLAB layout: table t owns
 * rows[t * stride .. t * stride + counts[t]) (ascending canonical id, same rows as
 * ddz_legal), so no table depends on another: a wavefront keeps its table in registers
 * across the iterations and stores the trajectory record of EVERY iteration.  A launch
 * leaves the lists of its LAST iteration's pre-step states in counts / rows / ids: every
 * iteration would overwrite the table's slab and nothing can read it in between, so the
 * earlier iterations store no list, and slab rows at and beyond counts[t] are not written
 * (who needs every iteration's lists calls ddz_rollout_random_csr_staged, or this with
 * n_iters = 1).  A call of more than 2^20 iterations is several launches; what it leaves
 * is the same.  The state is stored ONCE, after the last iteration: nothing can read it
 * between the iterations of a launch.
 *   counts int32[T]; rows int8[T * stride][16]; ids int32[T * stride] or NULL;
 *   stride >= 512 covers every list of a <= 20-card hand (497 is the maximum);
 *   stats (device, int64[8], may be NULL) accumulates {plies, finished episodes, total legal
 *   rows, lord wins, up wins, down wins, -, -} (Game.compete's per-role win counts,
 *   game.py:258-290); traj (may be NULL) is u8[n_iters][T][32].                            */
int ddz_rollout_random(ddz_env_t* env, int64_t n_iters, int32_t* counts, int8_t* rows,
                       int32_t* ids, int64_t stride, int64_t* stats, uint8_t* traj,
                       void* stream);

/* Playout evaluation (the reference's Monte-Carlo player as flat Monte Carlo: server/mcts/interface.py:15-45 with
 * default_policy.py:4-10 and the reward of tree.py:71-81; perfect information: all three hands of the state are used).
 * "Playout spec v1" (DESIGN.md 4): for every running table t (dealt, not done) with legal list L in slab order (what
 * ddz_legal_slab writes, n = |L|), every move index j < n and every playout number k < n_playouts: start from a copy of the
 * table's state, apply L[j] as ddz_step does without auto-reset, then, while the table is not done, apply the move at index
 * (draw * A) >> 32 of the state's legal list (A its size; A = 0, an imported state outside the domain, stops the playout) with
 *   draw = philox4x32_10(counter = (gid_lo, gid_hi, k << 9 | j, 4 << 16 | ply), key = (seed_lo ^ salt_lo, seed_hi)).x,
 * gid = table_id_base + t, ply = the u16 ply counter of the state being stepped (RNG domain 4; domains 1..3 are unchanged).
 * At most DDZ_PLAYOUT_MAX_PLIES moves are applied per playout, the root move included (>= the 162 plies of the longest game).
 *   wins int32 [T * stride], stride >= DDZ_SLAB_MIN_STRIDE: wins[t * stride + j] += the playouts of move j that ended with a
 *     winner on the root actor's side (the lord alone, or either farmer) -- entry j belongs to row j of ddz_legal_slab's slab at
 *     the same state.  The caller zeroes what it wants counted from zero; idle tables (done / not dealt) run nothing and their
 *     entries, like every entry at or beyond n, are left as they are.
 *   totals (device int64[4], may be NULL) += {moves applied (root moves included), playouts run, playouts that stopped
 *     unfinished (0 on every state play reaches), -}.
 *   chunks >= 1 (at most 2^20): wavefronts per table.  The n * n_playouts playouts of a table are dealt round-robin over its
 *     chunks, so one table -- also one with a long list and n_playouts = 1 -- fills the device; wins and totals do not depend on it
 *     (integer sums; 32-bit atomic adds where chunks share a move).  1 <= n_playouts < 2^23.
 * The env is only read: state, lists and statistics are untouched.  One launch on `stream`, nothing on the host (capturable).
 * A root list that would exceed `stride` or the kernel's staging capacity (impossible for hands of <= 20 cards) raises status
 * bit 1 and the table runs nothing.
 * A running table whose ACTOR's hand is empty (an imported state outside the domain: ddz_step ends a table with the card that
 * empties a hand) has the empty list, as a lead and facing a combination alike: nothing runs, its wins and the totals stay as
 * they are, and the status word is not touched.
 * ddz_playout_choose: choice[t] = ids[t * stride + the first maximum of wins[t * stride + 0 .. counts[t])] (ties to the lowest
 * index, as torch.argmax in dqn.py:60), -1 where counts[t] <= 0: feed it to ddz_step_slab(DDZ_STEP_IDS).  counts / ids as
 * ddz_legal_slab wrote them; a small launch over the live entries only. */
#define DDZ_PLAYOUT_MAX_PLIES 192
int ddz_playout(ddz_env_t* env, int64_t n_playouts, uint64_t salt, int64_t chunks, int64_t stride, int32_t* wins,
                int64_t* totals, void* stream);
int ddz_playout_choose(ddz_env_t* env, const int32_t* counts, const int32_t* ids, int64_t stride, const int32_t* wins,
                       int32_t* choice, void* stream);

/* Playouts over HIDDEN hands ("playout spec v2"): what ddz_playout computes, but with the two opponents' hands
 * sampled per playout number from the cards the actor has not seen -- their 15 count bytes are NEVER read, so a state built
 * from the plain serving payload (own hand, histories, hand sizes) is evaluated as the live table it describes.  Read of a
 * running table with actor `role`: the actor's hand row, the taken row, the recent rows with their category bytes, the meta
 * row, and byte 15 (cards left) of the other two hand rows.
 *   unseen_r = deck_r - hand[role]_r - taken_r (deck_r = 4 for the ranks 0..12, 1 for each joker); card c of Deal v2's
 *     numbering (rank c / 4 for c < 52, 52 = BJ, 53 = CJ) is in the pool iff (c & 3) < unseen_{c/4}, resp. unseen_13 / unseen_14
 *     = 1; n_next = left[(role + 1) % 3], n_prev = left[(role + 2) % 3].
 *   Domain: 0 <= unseen_r <= deck_r for every rank, n_next >= 1, n_prev >= 1, sum unseen = n_next + n_prev.  A running table
 *     outside it runs nothing, its wins and the totals stay as they are, and status bit 6 is raised.
 *   World k: pool card c draws key_c = philox4x32_10((gid_lo, gid_hi, k, 5 << 16 | c >> 2), (seed_lo ^ salt_lo, seed_hi))[c & 3]
 *     (RNG domain 5; domains 1..4 are unchanged); the pool is ranked by (key, c); the n_next lowest cards are the next
 *     player's hand, the others the previous player's.  A world depends on (gid, k, seed, salt) only: every root move of a
 *     table is played on the same n_playouts worlds (common random numbers); vary salt for fresh worlds per decision.
 *   Playout (j, k) is ddz_playout's, word for word, from the root with the opponents' hands replaced by world k: the draws
 *     of domain 4, the root move, the score, DDZ_PLAYOUT_MAX_PLIES, totals, idle tables and the independence from `chunks`.
 *   roles: bit r set = tables whose actor is role r take part, the others are idle (7 = every table).
 * ddz_playout_worlds: the worlds alone.  out uint8 [T][n_worlds][2][16]: [t][k][0] = the 15 counts and the size (byte 15) of
 * the next player's hand in world k of table t, [t][k][1] = the previous player's.  Idle tables, tables `roles` leaves out and
 * tables outside the domain (status bit 6) are left as they are.  1 <= n_worlds < 2^23, T * n_worlds <= 2^31 - 1.
 * Both: the env is only read; one launch on `stream`, nothing on the host (capturable). */
int ddz_playout_hidden(ddz_env_t* env, int64_t n_playouts, uint64_t salt, int64_t chunks, int64_t stride, int roles,
                       int32_t* wins, int64_t* totals, void* stream);
int ddz_playout_worlds(ddz_env_t* env, int64_t n_worlds, uint64_t salt, int roles, uint8_t* out, void* stream);

/* UCT tree search around the playouts: the reference's MCTS player (server/mcts/interface.py:37-43: tree_policy ->
 * default_policy -> backup, 1000 times; get_bestchild.py; tree.py:33-51), batched.  "Search spec v1 (UCT)" (DESIGN.md 4), for
 * every running table t (dealt, not done) and every tree c < trees; the trees of a table are independent (root parallelism)
 * and their root statistics are summed.
 *   Node: a state reached from the root by a path of moves.  It carries its actor, n = the size of its legal list in slab
 *     (ascending canonical id) order, the children created so far (each belongs to one list index), visits V and reward W
 *     (u32), and whether the move that led to it emptied a hand (terminal, winner = the mover).  Node 0 is the table's state;
 *     a root with an empty list runs nothing (visits, wins and totals stay as they are).
 *   Iteration i < budget (1 <= budget <= DDZ_SEARCH_MAX_BUDGET; the reference uses 1000): start at the root; while the node is
 *     not terminal and has n > 0: if fewer than n children exist, EXPAND the node and stop descending, otherwise go to the
 *     SELECTED child.  A non-terminal node with n = 0 (an imported state outside the domain) ends the iteration with reward 0,
 *     counted as unfinished; so does a non-terminal node DDZ_SEARCH_MAX_DEPTH moves below the root (beyond the 162 plies of the
 *     longest game: no state of the domain reaches it).
 *   Selection at a fully expanded node with visits N: child j with (V_j, W_j) has, in fp32 from correctly rounded single
 *     operations with nothing fused, mean = W_j / V_j, bonus = c * sqrt((2 * LN[N]) / V_j), value = mean + bonus, where
 *     LN[N] = (float)log((double)N) is a table of DDZ_SEARCH_MAX_BUDGET + 1 floats that the library fills from the host's libm
 *     once per device (ddz_search copies nothing from the host).  c >= 0 (0.7 in get_bestchild.py:4).
 *     mode DDZ_SEARCH_REFERENCE (get_bestchild.py:20-32, literally): the maximum of value at a node whose actor is the ROOT's
 *     actor, the minimum of value at every other node -- the partner farmer's included.
 *     mode DDZ_SEARCH_SIDES: the maximum of value at a node whose actor is on the root actor's side (the lord alone, or either
 *     farmer), otherwise the maximum of (V_j - W_j) / V_j + bonus.
 *     Ties go to the LOWEST list index (the reference draws among ties: a departure, as ddz_playout_choose's).
 *   Expansion: with u = the untried list indices, the ((draw_e * u) >> 32)-th of them in ascending order,
 *     draw_e = philox4x32_10((gid_lo, gid_hi, c << 16 | i, 6 << 16), key).x, key = (seed_lo ^ salt_lo, seed_hi), gid =
 *     table_id_base + t (RNG domain 6; domains 1..5 are unchanged).  The lead list has no pass, so tree.py:43's rejection loop
 *     has nothing to reject.  The child's n is the size of its state's list.
 *   Playout from the new child: playout spec v1's rule, index (draw * A) >> 32 of the state's list, draw =
 *     philox4x32_10((gid_lo, gid_hi, c << 16 | i, 7 << 16 | ply), key).x (domain 7), ply = the u16 ply counter of the state
 *     being stepped; at most DDZ_PLAYOUT_MAX_PLIES moves are applied from the child, a playout that stops unfinished scores 0.
 *     A terminal child, or a terminal node reached by selection, scores without a playout.  Score: 1 if the winner is on the
 *     ROOT actor's side (tree.py:71-81), else 0.
 *   Backup: V += 1 and W += score on every node of the path, the root included.
 *   visits / wins int32 [T * stride], stride >= DDZ_SLAB_MIN_STRIDE: [t * stride + j] += the V / W of root child j, summed
 *     over the table's trees (32-bit integer atomics: the result does not depend on scheduling).  The caller zeroes them.
 *   totals (device int64[4], may be NULL) += {moves applied (descent and playout), iterations run, iterations scored
 *     unfinished, nodes created}.
 *   hidden != 0: tree c plays on world k = c of playout spec v2 (the same deal of domain 5, the same domain check with status
 *     bit 6, the same `roles` mask; the opponents' count bytes are never read): trees = the number of determinizations.
 *     roles must be 7 in the open form.
 *   work: caller-owned device scratch of >= ddz_search_work_bytes(T, budget, trees) bytes, 16-byte aligned; a smaller buffer
 *     is DDZ_ECAP from the host.  Per tree it holds budget + 1 node records and an open-addressing table of the power of two
 *     >= 2 * (budget + 1) entries keyed by (parent, list index): a function of the budget alone in every position, no overflow
 *     mode.  Nothing in it has to be initialised and nothing in it is an output.  1 <= trees <= 65536.
 * The env is only read.  One launch on `stream`, nothing on the host (capturable).
 * ddz_search_choose: choice[t] = ids[t * stride + the first maximum of wins / visits over the entries j < counts[t] with
 * visits > 0], compared exactly as w_a * v_b > w_b * v_a in 64-bit integers (get_bestchild_: the win ratio alone), ties to
 * the lowest index; -1 where nothing was visited.  Feed it to ddz_step_slab(DDZ_STEP_IDS). */
#define DDZ_SEARCH_MAX_BUDGET 4096
#define DDZ_SEARCH_MAX_DEPTH 192
#define DDZ_SEARCH_REFERENCE 0
#define DDZ_SEARCH_SIDES 1
int64_t ddz_search_work_bytes(int64_t n_tables, int64_t budget, int64_t trees);
int ddz_search(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
               int64_t stride, int32_t* visits, int32_t* wins, int64_t* totals, void* work, int64_t work_bytes, void* stream);
int ddz_search_choose(ddz_env_t* env, const int32_t* counts, const int32_t* ids, int64_t stride, const int32_t* visits,
                      const int32_t* wins, int32_t* choice, void* stream);

/* Information-set MCTS over the sampled worlds: "search spec v2 (ISMCTS)" (DESIGN.md 4), the single-observer ISMCTS of
 * Whitehouse, Powley, Cowling (CIG 2011) and Cowling, Powley, Whitehouse (IEEE TCIAIG 4(2), 2012).  Where ddz_search(hidden)
 * builds tree c on world c alone, ddz_ismcts builds ONE tree per (table t, tree c) over all of its worlds.  Always the hidden
 * form: domain, `roles` mask, idle tables and status bit 6 are ddz_search(hidden != 0)'s; the opponents' count bytes are
 * never read.
 *   Worlds and draws: iteration i < budget of tree c plays on world k = c * budget + i of playout spec v2 (domain 5, keyed by
 *     (gid, k)): ddz_playout_worlds(trees * budget) lists exactly these worlds.  The expansion draw (domain 6) and the playout
 *     draws (domain 7) are spec v1's, on the counter (gid, c << 16 | i, ..).
 *   Node: (parent, the move into it), the move being its canonical action = its count row.  It carries V, W, the
 *     availability count A, terminal and winner (hand sizes are public: terminal is a function of the path).  It has no list
 *     size and no count of children created.
 *   Descent: at a non-terminal node less than DDZ_SEARCH_MAX_DEPTH moves below the root take the list L of the state in THIS
 *     world, in slab (ascending canonical id) order.  An empty list ends the iteration unfinished.  With U = the entries of L
 *     without a child, ascending: if U is not empty, create the ((draw_e * |U|) >> 32)-th entry of U with A = 1, raise A of
 *     every child that exists and whose move is in L by 1, and run spec v1's playout from the new child.  Otherwise select
 *     among the children whose moves are in L: value = W / V + c * sqrt((2 * LN[A]) / V) with the child's OWN A in place of the
 *     parent's N -- the five fp32 operations, the LN table and both modes are spec v1's -- ties to the lowest index of L, on
 *     the counts of before this iteration; then every child whose move is in L gets A += 1, the selected one included.
 *     Children whose moves are not in L take no part and keep their A.
 *   Backup, score, totals and the root outputs are spec v1's; the root actor's own list is the same in every world, so
 *     visits / wins stay aligned with the slab list.
 *   work: >= ddz_ismcts_work_bytes(T, budget, trees) bytes, 16-byte aligned; a smaller buffer is DDZ_ECAP from the host.  Per
 *     tree: budget + 1 node records of 32 bytes and an open-addressing table of the power of two >= 2 * (budget + 1) entries
 *     keyed by (parent, count row) and compared in full.  Nothing in it has to be initialised, nothing in it is an output.
 * Arguments, checks and error codes are ddz_search's.  The env is only read; one launch on `stream`, nothing on the host
 * (capturable).  ddz_search_choose picks the move from visits / wins. */
int64_t ddz_ismcts_work_bytes(int64_t n_tables, int64_t budget, int64_t trees);
int ddz_ismcts(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int roles, int64_t stride,
               int32_t* visits, int32_t* wins, int64_t* totals, void* work, int64_t work_bytes, void* stream);

/* UCT with leaf values from outside the kernel: "search spec v3 (guided UCT)" (DESIGN.md 4).  Spec v1 with the playout lifted
 * out: the score of a new non-terminal leaf is a value the caller hands in, so a network (or anything else) can judge the
 * position.  Everything not named here is ddz_search's: nodes, n, budget and depth limits, both modes, ties, the LN table,
 * the expansion draw (domain 6), root parallelism, `roles`, the hidden form on world c with status bit 6, status bit 1.
 *   Unit: W counts in DDZ_GUIDED_ONE = 1024ths, V counts visits.  budget * trees * 1024 must stay below 2^31 (the int32 root
 *     sums): a call that breaks this is DDZ_EINVAL, nothing launched.  Selection: mean = ((float)W / (float)V) * 2^-10, then
 *     spec v1's operations; DDZ_SEARCH_SIDES uses V * 1024 - W where v1 uses V - W.
 *   One launch = one iteration of every (table, tree).  Descend as in v1.  A node with untried indices: expand one child; if
 *     the move empties a hand the child is terminal, scores 1024 when the winner is on the root actor's side, else 0, and is
 *     backed up in the same launch; otherwise the child is a PENDING LEAF: its n is the size of its state's list, its state
 *     row is written to leaf_rows[item], need[item] = 1, and the iteration waits.  A terminal node reached by selection is
 *     scored and backed up at once.  A non-terminal node with n = 0, or DDZ_SEARCH_MAX_DEPTH below the root: score 0, unfinished.
 *   Leaf value: values[item] (item = t * trees + c), the chance in 1024ths that the side of the LEAF's actor wins, clamped
 *     into [0, 1024]; the score is v where the leaf's actor is on the root actor's side, else 1024 - v.  Backup (V += 1,
 *     W += score on the path, the new node's record written whole) happens at the start of the next launch, or in close.
 *   Leaf row: the 176 bytes ddz_step (no auto-reset) would hold after the path's moves: hands with their count bytes (the
 *     world's for the opponents in the hidden form), histories, recent rows with category bytes, taken, meta (role, done 0,
 *     winner 0xFF, last r 0, ply, the root's bytes 6..15).  Items that are idle, outside the domain, finished at once or past
 *     their budget get an all-zero row (dealt = 0) and need 0.
 *   ddz_guided_open: sizes the root list, zeroes table and header, writes node 0.  ddz_guided_step: values may be NULL on
 *     the first step only; leaf_rows uint8 [T * trees][176], 16-byte aligned; need int32 [T * trees].  ddz_guided_close: backs
 *     up the last pending leaf, then visits / wins [T * stride] += the V / W (1024ths) of the root's children summed over
 *     trees, totals += {moves applied, iterations run, unfinished, nodes created}.  ddz_search_choose serves as the chooser.
 *   work: >= ddz_guided_work_bytes(T, budget, trees) bytes, 16-byte aligned, the same buffer for open, every step and close;
 *     per tree spec v1's nodes and table, a 64-byte header and the stored path.  The env is only read but must not change
 *     between open and close (the root is re-read by every launch).  Argument checks and codes are ddz_search's; one launch
 *     per call on `stream`, nothing on the host (capturable).
 * ddz_guided_values: leaf values from a q slab, one wavefront per leaf: for every row of rows [n][176] that is running and
 *   whose actor's role is in net_roles, values[i] = clamp((int)rintf((qmax * inv_reward[role] + 1) * 512), 0, 1024), qmax = the
 *   maximum of q[i * stride .. + counts[i]), single fp32 operations; counts[i] = 0 or a NaN among them gives 512.  Other
 *   entries of values are left as they are.  inv_reward: HOST float[3] in role order. */
#define DDZ_GUIDED_ONE 1024
int64_t ddz_guided_work_bytes(int64_t n_tables, int64_t budget, int64_t trees);
int ddz_guided_open(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
                    int64_t stride, void* work, int64_t work_bytes, void* stream);
int ddz_guided_step(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
                    int64_t stride, const int32_t* values, uint8_t* leaf_rows, int32_t* need, void* work, int64_t work_bytes,
                    void* stream);
int ddz_guided_close(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
                     const int32_t* values, int64_t stride, int32_t* visits, int32_t* wins, int64_t* totals, void* work,
                     int64_t work_bytes, void* stream);
int ddz_guided_values(int device_id, const uint8_t* rows, const int32_t* counts, const float* q, int64_t stride, int64_t n,
                      const float* inv_reward, int net_roles, int32_t* values, void* stream);

/* Guided UCT with move priors: "search spec v5 (guided PUCT)" (DESIGN.md 4).  ddz_guided_*'s launches (open / step / close, W in
 * 1024ths, budget * trees * 1024 < 2^31, the clamped value scored v or 1024 - v by the leaf actor's side, the leaf row, need, the
 * backup at the start of the next launch or in close, the hidden form on world c with status bit 6, status bit 1) with a PRIOR
 * WEIGHT for every move of every evaluated node: selection runs over all list indices of a node, visited or not, and nothing
 * is expanded at random (no expansion draw).  mode must be DDZ_SEARCH_SIDES (else DDZ_EINVAL): a node's actor maximises its own
 * side's mean.
 *   priors: uint8 [T * trees][stride], 16-byte aligned, CALLER-FILLED between the steps beside values: priors[item * stride + j]
 *     is the weight of index j of the pending node's list, in the order of ddz_legal_slab on the imported leaf row, j < n;
 *     entries at or beyond n are never read.  values and priors may be NULL on the first step only.
 *   Node: 32 bytes: ddz_search's 24 | prior-pool offset u32 (0xFFFFFFFF: none stored) | weight sum S u32.  Prior pool: `pool` bytes
 *     per tree behind the hash table, pool a multiple of 16 in [16, 2^24] (else DDZ_EINVAL); the run of a node with list size n is
 *     n bytes at the next multiple of 4, in the order the nodes are backed up (= created).  A run that does not fit is not stored:
 *     the node is UNIFORM and counted in totals[4].  A run whose weights are all zero is uniform too (not counted).  A terminal
 *     node and a node with n = 0 take no run.
 *   Iteration 0 (the first step of a live item) descends nowhere: node 0 is left pending with the root's row (hidden: on the
 *     tree's world) and need = 1; its backup stores the root's priors and adds the root's value to node 0.  So `budget`
 *     iterations grow at most budget - 1 nodes below the root.
 *   Descent: at a non-terminal node with n > 0, N = its V, for every list index j, single fp32 operations, nothing fused:
 *       mean_j = ((float)Wside_j / (float)V_j) * 2^-10 where child j exists, else the node's own ((float)Wside / (float)N) * 2^-10
 *                (Wside = W where the node's actor is on the root actor's side, else V * 1024 - W)
 *       p_j = (float)w_j / (float)S, or 1.0f / (float)n at a uniform node
 *       value_j = mean_j + ((c * p_j) * sqrtf((float)N)) / (float)(1 + V_j);   the maximum, ties to the lowest index.
 *     The selected index has a child: go to it (a terminal one is scored at once).  Otherwise the child is created: a move that
 *     empties a hand makes it terminal (1024 or 0, backed up in the same launch), any other leaves it pending with its row as
 *     ddz_guided_step leaves a leaf.  n = 0 or DDZ_SEARCH_MAX_DEPTH below the root: score 0, unfinished.
 *   ddz_puct_close: backs up the last pending node, then visits / wins as ddz_guided_close; totals int64 [5] += {moves applied,
 *     iterations run, unfinished, nodes created, nodes that fell back to uniform priors}.  The move with the most visits is
 *     ddz_playout_choose on visits.
 *   work: >= ddz_puct_work_bytes(T, budget, trees, pool) bytes (a function of these alone; -1 for arguments out of range),
 *     16-byte aligned.  A launch that finds a header open did not write, or one out of range, runs nothing on that tree.
 *     Argument checks and codes are ddz_guided_*'s, in their order; then the mode, the pool.
 * ddz_puct_priors: prior weights from a q slab, one wavefront per leaf: for every row of rows [n][176] that is running and whose
 *   actor's role is in net_roles, priors[i * stride + j] = clamp((int)rintf(255 * expf(((q_j - qmax) * inv_reward[role]) *
 *   inv_tau)), 0, 255) for j < counts[i], qmax = the row's maximum (an entry equal to it gets 255), single fp32 operations; a
 *   NaN in the row gives all ones.  Other rows and the entries at or beyond counts[i] are left as they are.  inv_tau finite,
 *   >= 0; inv_reward: HOST float[3] in role order. */
int64_t ddz_puct_work_bytes(int64_t n_tables, int64_t budget, int64_t trees, int64_t pool);
int ddz_puct_open(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
                  int64_t stride, int64_t pool, void* work, int64_t work_bytes, void* stream);
int ddz_puct_step(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
                  int64_t stride, int64_t pool, const int32_t* values, const uint8_t* priors, uint8_t* leaf_rows, int32_t* need,
                  void* work, int64_t work_bytes, void* stream);
int ddz_puct_close(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int hidden, int roles,
                   const int32_t* values, const uint8_t* priors, int64_t stride, int64_t pool, int32_t* visits, int32_t* wins,
                   int64_t* totals, void* work, int64_t work_bytes, void* stream);
int ddz_puct_priors(int device_id, const uint8_t* rows, const int32_t* counts, const float* q, int64_t stride, int64_t n,
                    const float* inv_reward, int net_roles, float inv_tau, uint8_t* priors, void* stream);

/* Information-set MCTS with leaf values from outside the kernel: "search spec v4 (guided ISMCTS)" (DESIGN.md 4).  ddz_ismcts's
 * tree and descent in ddz_guided_*'s phases, unit and leaf value: no tree is built with full knowledge of one deal, and a
 * network (or anything else) judges the leaves.  Everything not named here is ddz_ismcts's for the tree (always the hidden
 * form, the `roles` gate, the domain with status bit 6, nodes keyed by (parent, move) with V, W and the availability count A,
 * the descent enumerating the list of the state in this iteration's world, A += 1 for every existing child in that list, the
 * child's own A in the bonus, the expansion draw of domain 6 on (gid, c << 16 | i)) and ddz_guided_*'s for the launches (open /
 * step / close, W in 1024ths, budget * trees * 1024 < 2^31 else DDZ_EINVAL, the clamped value scored v or 1024 - v by the leaf
 * actor's side, the leaf row, need, the backup at the start of the next launch or in close).
 *   The step that runs iteration i of tree c deals world c * budget + i of playout spec v2 itself; there are no playout
 *     draws.  Selection value: ((float)W / (float)V) * 2^-10 + c * sqrt((2 * LN[A]) / V), nothing fused; DDZ_SEARCH_SIDES away
 *     from the root's side uses V * 1024 - W.  A new child has A = 1; one whose move empties a hand is terminal, scores 1024
 *     or 0 and is backed up in the same launch; any other is a pending leaf whose row holds this iteration's world as the two
 *     opponents' hands (its list is not enumerated).  An empty list or DDZ_SEARCH_MAX_DEPTH below the root: score 0, unfinished.
 *   ddz_gismcts_close: backs up the last pending leaf, then visits / wins [T * stride] += the V / W (1024ths) of the root's
 *     children at their index of the root's own list (the same in every world), totals += {moves applied, iterations run,
 *     unfinished, nodes created}.  ddz_search_choose serves as the chooser.
 *   work: >= ddz_gismcts_work_bytes(T, budget, trees) bytes, 16-byte aligned, the same buffer for open, every step and close;
 *     per tree ddz_ismcts's nodes and table, a 64-byte header and the stored path.  A launch that finds a header open did not
 *     write runs nothing on that tree.  Argument checks and codes are ddz_guided_*'s, in their order. */
int64_t ddz_gismcts_work_bytes(int64_t n_tables, int64_t budget, int64_t trees);
int ddz_gismcts_open(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int roles, int64_t stride,
                     void* work, int64_t work_bytes, void* stream);
int ddz_gismcts_step(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int roles, int64_t stride,
                     const int32_t* values, uint8_t* leaf_rows, int32_t* need, void* work, int64_t work_bytes, void* stream);
int ddz_gismcts_close(ddz_env_t* env, int64_t budget, int64_t trees, int mode, float c, uint64_t salt, int roles,
                      const int32_t* values, int64_t stride, int32_t* visits, int32_t* wins, int64_t* totals, void* work,
                      int64_t work_bytes, void* stream);

/* The CFR endgame solver: the reference's final_card (server/CFR.py: deal / initiate_game / VanillaCFR.run(8)), the engine
 * its predictor uses when the three hands hold 6 cards or fewer (server/core.py:88), batched.  "CFR spec v1" (DESIGN.md 4):
 * the reference's computation with everything it leaves to chance pinned.  Seats are the reference's player numbers, 0 lord /
 * 1 down / 2 up = role (seat + 1) % 3, and the turn order is seat 0, 1, 2.
 *   Domain: a running table (dealt, not done) with actor `role` whose bit is set in `roles`, left[role] = the cards of its hand
 *     row, left of the other two = byte 15 of their hand rows (their count bytes are NEVER read, as in playout spec v2), with
 *     every left >= 1, left[0] + left[1] + left[2] <= DDZ_CFR_MAX_CARDS, pool_r = deck_r - taken_r >= 0, sum pool = sum left,
 *     and the actor's hand row inside pool.  Read besides: the recent rows with their category bytes and the meta row.
 *     n[t] = 0 for an idle table (not running, or its actor not in `roles`); n[t] = -1 and NO status bit for a running table
 *     with more than DDZ_CFR_MAX_CARDS cards ("not an endgame": what a dispatcher tests); n[t] = -1 and status bit 6 where the
 *     rows do not add up.  The combination to beat and its owner: the previous seat's recent row if non-empty, else the row
 *     of the seat before it, else a lead owned by the actor.
 *   Deals: every distinct assignment of pool to the seats by per-rank counts with the seats' sizes, ordered as CFR.py:deal
 *     yields them (ranks ascending; per rank the lord's count, then down's count, ascending); D <= DDZ_CFR_MAX_DEALS, each
 *     weighs 1 / D.
 *   Tree of a deal: a node's actions are the legal list of its state in slab order (ascending canonical id, pass first when
 *     following); after a pass the next seat leads if it owns the combination to beat, else it faces the same combination
 *     (CFR.py:152-174); a node where a hand is empty is terminal with utility +1 if that hand is the lord's, else -1.
 *   Information set: (mover, the mover's hand in the deal, the actions from the root); at most one node per deal.
 *   Arithmetic: IEEE double, every operation rounded on its own, nothing fused.  sigma starts at 1 / n.  Iteration (the
 *     reference runs 8; 0 <= iterations <= DDZ_CFR_MAX_ITERATIONS): reaches ra, rb, rc start at 1 and the mover's is multiplied
 *     by sigma[a] towards child a; value = ((0 + s0 * u0) + s1 * u1) + ... in action order; cfr_reach = rb * rc, ra * rc,
 *     ra * rb for mover 0, 1, 2; R[I][a] += cfr_reach * (u_a - value), negated for a farmer, IN ASCENDING DEAL ORDER (the
 *     reference walks a Python set: this is the pinning); after all deals sigma_a = max(R_a, 0) / S, S = the positive R_a
 *     added in action order, and 1 / n where S <= 0; value_t = (1 / D) * (u_root(0) + u_root(1) + ...).
 *   Result: n[t] = the size of the actor's legal list, ids[t][j] its canonical ids, sigma[t][j] the row of the information
 *     set (actor, its actual hand, no action), value[t] = the last iteration's value_t (0 with no iteration).  ids and sigma
 *     are [T][DDZ_CFR_STRIDE], written whole for every table (ids -1 / sigma 0 beyond n and where nothing is solved).
 *     totals (device int64[4], may be NULL) += {deals, nodes, information sets, (information set, action) pairs} of the
 *     solved tables.  The result is bit-identical from run to run: no floating-point atomics, no order left to scheduling.
 *   Workspace: ddz_cfr_work_bytes(slots) bytes, 16-byte aligned, nothing in it to initialise: a head with a counter (zeroed
 *     by a one-wave launch of this call) and `slots` slots of about 1.7 MiB.  Every table inside the domain takes one
 *     slot; one that finds none, or whose forest exceeds a capacity (DDZ_CFR_MAX_NODES, DDZ_CFR_MAX_INFOSETS, ...: twice what
 *     any endgame was measured to need, tools/cfr_sweep.py), gets n[t] = -2 and status bit 7.  slots >= 0.
 * The env is only read.  Two launches on `stream` (the head's zeroing, the solver), nothing on the host (capturable).
 * ddz_cfr_choose: choice[t] = ids[t][j], -1 where n[t] <= 0.  greedy != 0: j = the first maximum of sigma[t].  Otherwise, as
 *   the reference's choose(): u = x * 2^-32 with x = philox4x32_10((gid_lo, gid_hi, 0, 8 << 16), (seed_lo ^ salt_lo, seed_hi)).x
 *   (RNG domain 8; domains 1..7 are unchanged), j = the first index with u below the running sum of sigma in list order,
 *   else the last index with sigma_j > 0.  Feed it to ddz_step_slab(DDZ_STEP_IDS). */
#define DDZ_CFR_MAX_CARDS 6
#define DDZ_CFR_STRIDE 16
#define DDZ_CFR_MAX_DEALS 90        /* 6! / (2! 2! 2!) */
#define DDZ_CFR_MAX_ACTIONS 8       /* a hand of at most 4 cards has at most 5 moves */
#define DDZ_CFR_MAX_DEPTH 24        /* at most 6 plays, each followed by at most 2 passes */
#define DDZ_CFR_MAX_NODES 32768     /* measured maximum 10,512 */
#define DDZ_CFR_MAX_INFOSETS 8192   /* measured maximum 2,835 */
#define DDZ_CFR_MAX_ITERATIONS 64
int64_t ddz_cfr_work_bytes(int64_t slots);
int ddz_cfr(ddz_env_t* env, int iterations, int roles, int64_t slots, void* work, int64_t work_bytes, int32_t* n, int32_t* ids,
            double* sigma, double* value, int64_t* totals, void* stream);
int ddz_cfr_choose(ddz_env_t* env, const int32_t* n, const int32_t* ids, const double* sigma, uint64_t salt, int greedy,
                   int32_t* choice, void* stream);

/* The exact endgame solver: open-hand minimax of the two-sided win / lose game (the lord against the two farmers) for every
 * root move of every table that is an endgame.  The reference has no such solver; "Solve spec v1"  is the
 * engine's own, pinned by a CPU restatement on the oracle (tests/solve_reference.py).
 *   Domain: a running table (dealt, not done) whose actor's bit is set in `roles` and whose three hands together hold
 *     1 .. max_cards cards, max_cards <= DDZ_SOLVE_MAX_CARDS.  Open form (hidden == 0; worlds must be 1 and roles 7): the
 *     three hand rows are read.  Hidden form (hidden != 0, worlds = K >= 1): the actor's hand row and byte 15 of the other two
 *     hand rows are read -- the opponents' count bytes NEVER -- and world k < K is world k of playout spec v2, exactly what
 *     ddz_playout_worlds(K, salt) returns (the same deal of RNG domain 5 keyed by (gid, k), the same domain test).
 *     n[t] = the size of the actor's legal list where the table was solved, 0 for an idle table (not running, or its actor
 *     not in `roles`), -1 and NO status bit for a running table with more than max_cards cards ("not an endgame": what a
 *     dispatcher tests), -1 and status bit 6 where the hidden form's rows do not add up to a deck.
 *   Value: the mover whose hand empties wins for its side (the lord alone, or either farmer).  wins[t * stride + j] += 1 for
 *     every world in which, after move j of table t's slab list (ddz_legal_slab order), the ROOT ACTOR's side wins under best
 *     play of both sides; unknown[t * stride + j] += 1 for every world in which the search of move j ran out of `budget` (that
 *     world adds nothing to wins).  Entries of tables that were not solved are not touched.  The caller zeroes both arrays
 *     (int32 [T * stride], stride >= DDZ_SLAB_MIN_STRIDE); 32-bit integer atomics, the result does not depend on scheduling.
 *     Where unknown is 0, wins is a fact about the game: it does not depend on budget, chunks or tt_entries.
 *   Search of root move j (budget nodes of its own; no cut among the root moves): the move is applied; if it empties the
 *     actor's hand the actor's side has won, else the position behind it is ENTERED.  A position is (the three hands, the
 *     combination to beat, the passes since it was played, the mover); two passes hand the lead back, and a position whose
 *     passes reached 2 IS the lead position (nothing to beat, no passes).  Entering a position: if the nodes of move j have
 *     reached budget, move j is unknown and its search ends; else nodes += 1, the table is probed and a hit returns its value
 *     (hits += 1); else the children are tried in list order (slab order, pass first when following): a child whose move
 *     empties the mover's hand wins for the mover at once -- it is not entered and counts no node -- any other child is
 *     entered, and its value is the mover's where both movers are on one side, the opposite otherwise.  The first child
 *     that wins for the mover's side ends the position as won (the cut); with no such child -- or an empty list -- it is
 *     lost.  A finished position is stored in the table; the positions an exhausted budget leaves open are not.
 *   Transposition table: tt_entries entries (a power of two, 1 .. DDZ_SOLVE_MAX_TT) per (table, world, chunk), direct
 *     mapped, always replaced, empty before the first root move of the chunk and shared by its root moves in ascending
 *     order.  With hc / hn / hp the hands of the mover, the next and the previous player as 15 nibbles (rank r at bits
 *     4r .. 4r+3) and cb the cards of the combination to beat in the same form, the key is x = hc | mover << 60, y = hn,
 *     z = hp, w = cb | passes << 60 (w = 0 for the lead position), all of which an entry holds and a hit compares, and
 *     slot = low 32 bits of h, h = x * 0x9E3779B97F4A7C15 ^ y * 0xC2B2AE3D27D4EB4F ^ z * 0x165667B19E3779F9 ^
 *     w * 0x85EBCA77C2B2AE63, h ^= h >> 29, h *= 0xBF58476D1CE4E5B9, h ^= h >> 32 (mod 2^64), masked by tt_entries - 1.
 *   Work split: one wavefront per (table, world, chunk); chunk c solves the root moves j = c (mod chunks).  1 <= chunks <=
 *     65536, 1 <= worlds <= 65536, 1 <= budget <= DDZ_SOLVE_MAX_BUDGET.
 *   Depth: a move that is no pass removes a card, at most two passes follow one and at most two precede the first, the
 *     last move of a game is no pass: at most 3 * cards moves, DDZ_SOLVE_MAX_DEPTH frames.  A deeper search (impossible
 *     inside the domain) raises status bit 8 and leaves its move unknown.
 *   totals (device int64[4], may be NULL) += {nodes, table hits, root moves solved, root moves unknown}: with the order,
 *     the node count and the table fixed as above they are functions of the arguments, as unknown is.
 *   work: caller-owned device scratch of >= ddz_solve_work_bytes(T, worlds, chunks, tt_entries) bytes (32 per entry),
 *     16-byte aligned; a smaller buffer is DDZ_ECAP from the host.  Nothing in it has to be initialised: a wavefront clears
 *     its own table.
 * The env is only read.  One launch on `stream`, nothing on the host (capturable).
 * ddz_solve_choose: choice[t] = ids[t * stride + j], j = the first maximum of wins over the entries j < counts[t], among
 *   equal wins the first with the fewest unknown (remaining ties to the lowest index); -1 where counts[t] <= 0.  value[t] = 1
 *   where that move is proven winning (wins = worlds), 0 where every move is proven losing (wins = unknown = 0 throughout),
 *   else -1 (also where counts[t] <= 0).  Feed choice to ddz_step_slab(DDZ_STEP_IDS). */
#define DDZ_SOLVE_MAX_CARDS 20      /* one full hand */
#define DDZ_SOLVE_MAX_DEPTH 60      /* 3 * DDZ_SOLVE_MAX_CARDS */
#define DDZ_SOLVE_MAX_BUDGET (1 << 30)
#define DDZ_SOLVE_MAX_TT (1 << 20)
int64_t ddz_solve_work_bytes(int64_t n_tables, int64_t worlds, int64_t chunks, int64_t tt_entries);
int ddz_solve(ddz_env_t* env, int64_t budget, int max_cards, int64_t worlds, int hidden, int roles, uint64_t salt, int64_t chunks,
              int64_t tt_entries, int64_t stride, int32_t* n, int32_t* wins, int32_t* unknown, int64_t* totals, void* work,
              int64_t work_bytes, void* stream);
int ddz_solve_choose(ddz_env_t* env, const int32_t* counts, const int32_t* ids, int64_t stride, int64_t worlds,
                     const int32_t* wins, const int32_t* unknown, int32_t* choice, int32_t* value, void* stream);

/* The same random-policy loop with the lists in the CSR layout of ddz_legal (offsets/rows/ids
 * packed across tables).  CSR bases need a scan over all tables, so this variant is one
 * launch per iteration: the fused kernel writes the list of the current state, steps, and
 * sizes + scans the lists of the new state for the next launch.  Same trajectories, same
 * states as ddz_rollout_random; after the call offsets/rows hold the last pre-step lists.     */
int ddz_rollout_random_csr(ddz_env_t* env, int64_t n_iters, int32_t* offsets, int8_t* rows,
                           int32_t* ids, int64_t row_capacity, uint8_t* traj, void* stream);
/* The same loop, same outputs (offsets / rows / ids hold the CSR lists of the last iteration's pre-step states, exactly as
 * ddz_legal writes them; every iteration's lists are written there at their CSR positions), WITHOUT a launch per iteration:
 * the lists of `batch` iterations are staged as slabs by one rollout launch and compacted by two more (the cross-table
 * prefix of an iteration is nobody's launch boundary).  staging: caller-owned device scratch of
 * ddz_rollout_csr_staging_bytes(n_tables, batch, ids != NULL) bytes (batch x n_tables x 512 rows of 16 (+ 4) bytes: size
 * the batch for the memory you have), 256-byte aligned.  Same states, trajectories and RNG draws as ddz_rollout_random.  */
int64_t ddz_rollout_csr_staging_bytes(int64_t n_tables, int batch, int want_ids);
int ddz_rollout_random_csr_staged(ddz_env_t* env, int64_t n_iters, int batch, void* staging, int64_t staging_bytes,
                                  int32_t* offsets, int8_t* rows, int32_t* ids, int64_t row_capacity, uint8_t* traj, void* stream);

/* Measurement aid: the same loop between two hipEvents on `stream`.  ms (HOST, double[2])
 * receives {elapsed ms of the launch, n_iters}; synchronises the stream.
 * Used by bench.py for the roofline figure.                                                */
int ddz_rollout_random_timed(ddz_env_t* env, int64_t n_iters, int32_t* counts, int8_t* rows,
                             int32_t* ids, int64_t stride, double* ms, void* stream);

/* stats (device, int64[8]) += {plies, finished episodes, legal rows, lord wins, up wins, down
 * wins, -, -} accumulated by ddz_step / ddz_legal / the rollouts since the last read; the
 * internal accumulators are cleared.                                                      */
int ddz_read_stats(ddz_env_t* env, int64_t* stats, void* stream);

/* Replaces the action selection of DQNFirst.greedy_action / e_greedy_action (dqn.py:50-71)
 * for all tables: q float[offsets[T]] holds one value per legal row in CSR order;
 * choice int32[T] = first index of the segment's maximum (torch.argmax, dqn.py:60,70), -1 for
 * an empty list.  With epsilon > 0 a table explores with that probability (engine RNG
 * domain 3, keyed by table id / episode / ply): uniform index (dqn.py:57-58).             */
int ddz_select(ddz_env_t* env, const float* q, const int32_t* offsets, double epsilon,
               int32_t* choice, void* stream);

/* ddz_select for the slab layout: q is f32 [T][stride] (values beyond counts[t] are ignored). */
int ddz_select_slab(ddz_env_t* env, const float* q, const int32_t* counts, int64_t stride, double epsilon,
                    int32_t* choice, void* stream);

/* First layer of the Q forward below per (table, rank, count), from `face` alone: conv1..conv4 (net.py:141-144: a (1,k)
 * window, stride 4, on the width-4 input = one output column per rank) + the (1,4) max-pool (net.py:93-94 = the max over
 * the four convs), for every count cnt = 0..4 an action could take of that rank (its thermometer, envi.py:139-146, is the
 * action plane net.py:89-90 appends):
 *   y[((r * 5 + cnt) * T + t) * y_row_stride + c] = max_k (bias[k][c] + sum_{p, j <= k} wf[p * 4 + j][k * 256 + c] * face[t][p][r][j]
 *                                                          + acnt[cnt][k][c]),   c < 256
 * (the two joker ranks r = 13, 14 exist once: only cnt = 0, 1 are written for them).
 * face f32 [T][planes][15][4] (ddz_observe / ddz_policy_step_slab), wf f32 [planes * 4][1024], bias f32 [1024], acnt f32
 * [5][4][256] (weight-only tables, built by FactorisedQ.refresh from the network's conv weights); planes in {4, 6, 7, 9}.
 * acnt[0] (count 0: an empty thermometer, all zeros) is NOT READ by any first-layer kernel: count 0 adds nothing.
 * The training glue (dqn_glue.FactorisedQ.tables, ragged_q) multiplies y by fc1 per rank.  Stateless; fp32.          */
int ddz_q_features(int device_id, const float* face, int64_t n_tables, int planes, const float* wf, const float* bias,
                   const float* acnt, float* y, int64_t y_row_stride, void* stream);

/* The learner's first layer (net.py:87-94: cat, conv1..conv4, cat, the (1,4) max-pool) for a replay batch, forward and
 * backward, with the [n][256][15][4] pre-pool tensor never materialised (doudizhu-rl_amd/csrc/ddz_qtrain.h).  With
 * C = planes + 1 and x[n][c][r][j] = the planes of face f32 [n][planes][15][4] followed by action f32 [n][15][4] (two pointers,
 * no cat), the nn.Conv2d parameters are read as they lie in memory -- w[k - 1] = conv_k.weight f32 [256][C][1][k], b[k - 1] =
 * conv_k.bias f32 [256], k = 1..4 (HOST arrays of four DEVICE pointers) -- nothing is repacked, nothing cached:
 *   s_k               = b_k[o] + sum_{c < C, j < k} w_k[o][c][0][j] * x[n][c][r][j]            o < 256, r < 15
 *   y[n][o * 15 + r]   = max_k s_k                       f32 [n][3840]: the layout of net.py:94's view, what fc1 consumes
 *   arg[n][o * 15 + r] = the LOWEST k - 1 that attains it   u8 0..3 (max_pool2d's tie rule); arg may be NULL (a no-grad pass)
 * Backward, from gy f32 [n][3840] and arg, into gw[k - 1] / gb[k - 1] in the parameters' own shapes (no gradient of x):
 *   gw_k[o][c][0][j] = sum over (n, r) with arg[n][o * 15 + r] == k - 1 of gy[n][o * 15 + r] * x[n][c][r][j]
 *   gb_k[o]          = sum over (n, r) with arg[n][o * 15 + r] == k - 1 of gy[n][o * 15 + r]
 * DETERMINISTIC: no floating-point atomics -- every block stores its partial sums into ws (caller-owned, at least
 * ddz_q_first_bwd_ws_bytes bytes, not initialised, not kept) and a second launch adds the partials in a fixed order: equal
 * operands give bit-equal gradients.  planes in {4, 6, 7, 9}; face, action, y, gy and arg 16-byte aligned; fp32; stateless;
 * every launch on `stream`, nothing on the host (capturable).  n = 0 is a no-op (DDZ_OK); unknown planes, a null or
 * misaligned operand and a short workspace are DDZ_EINVAL.  NaN operands are outside the contract.                  */
int ddz_q_first_fwd(int device_id, const float* face, const float* action, int64_t n, int planes, const float* const w[4],
                    const float* const b[4], float* y, uint8_t* arg, void* stream);
int64_t ddz_q_first_bwd_ws_bytes(int64_t n, int planes);
int ddz_q_first_bwd(int device_id, const float* face, const float* action, int64_t n, int planes, const float* gy,
                    const uint8_t* arg, float* const gw[4], float* const gb[4], void* ws, int64_t ws_bytes, void* stream);

/* The learner's whole stage in front of dropout / fc1 (net.py:87-97: the first layer above, conv_shunzi, the view and the cat)
 * for a replay batch, forward and backward, from faces or straight from packed replay rows: h f32 [n][4864] is written whole
 * by two launches, the backward gives all ten convolution-parameter gradients (three launches), no face is materialised for
 * the rows source and no library convolution runs.  With x[n][c][r][j] and C as above, w[0..3] / b[0..3] as above and
 * w[4] = conv_shunzi.weight f32 [256][C][15][1], b[4] = conv_shunzi.bias f32 [256] (HOST arrays of five DEVICE pointers):
 *   h[n][o * 15 + r]        = max_k s_k            the first layer; arg u8 [n][3840] as above (NULL: a no-grad pass)
 *   h[n][3840 + o * 4 + j]  = b[4][o] + sum_{c < C, r < 15} w[4][o][c][r][0] * x[n][c][r][j]            o < 256, j < 4
 * Backward, from gh f32 [n][4864] and arg, into gw[0..4] / gb[0..4] in the parameters' own shapes:
 *   gw[0..3], gb[0..3]      = the first layer's, from the columns gh[n][o * 15 + r]: bit for bit those of the first-layer entry
 *   gw[4][o][c][r][0]       = sum_{n, j} gh[n][3840 + o * 4 + j] * x[n][c][r][j]
 *   gb[4][o]                = sum_{n, j} gh[n][3840 + o * 4 + j]
 * The source of x is a descriptor:
 *   kind DDZ_Q_SRC_FACES  planes in {4, 6, 7, 9}, face f32 [n][planes][15][4], action f32 [n][15][4] (as the first-layer entry)
 *   kind DDZ_Q_SRC_ROWS   variant 0..3 (planes 4 / 7 / 9 / 6), states u8 [n_rows][176] and ids int32 [n_rows] (a replay ring's
 *                         s0 + a0 or s1 + a1), index int64 [n] (NULL: sample i is entry i; entries are clamped into
 *                         [0, n_rows)), table int8 [n_actions][16] (the rows the action-table entry point writes, so either
 *                         rule set serves).  Sample i's planes are the face of `variant` of state row index[i] (the observe
 *                         entry points' expression, bit for bit) and its action plane the thermometer of
 *                         table[clamp(ids[index[i]], 0, n_actions - 1)] (slot j set iff count > j): for equal inputs both
 *                         kinds give bit-equal h, arg and gradients.
 * h_stride / gh_stride: the row stride in floats; 4864 is the one supported (else DDZ_EINVAL).  DETERMINISTIC as above: ws is
 * caller-owned, at least ddz_q_stage_bwd_ws_bytes bytes (its size depends on n and planes alone), not initialised, not kept.
 * fp32; face / action / states / h / gh / arg 16-byte aligned; stateless; every launch on `stream`, nothing on the host
 * (capturable).  n = 0 is a no-op (DDZ_OK); an unknown kind / planes / variant, a null or misaligned operand and a short
 * workspace are DDZ_EINVAL; n > 2^30 is DDZ_ECAP.  NaN operands are outside the contract.                          */
#define DDZ_Q_SRC_FACES 0
#define DDZ_Q_SRC_ROWS 1
typedef struct ddz_q_src {
  int kind;               /* DDZ_Q_SRC_FACES / DDZ_Q_SRC_ROWS */
  int planes;             /* faces */
  const float* face;      /* faces */
  const float* action;    /* faces */
  int variant;            /* rows */
  int n_actions;          /* rows */
  const uint8_t* states;  /* rows */
  const int32_t* ids;     /* rows */
  const int64_t* index;   /* rows; may be NULL */
  const int8_t* table;    /* rows */
  int64_t n_rows;         /* rows */
} ddz_q_src_t;
int ddz_q_stage_fwd(int device_id, const ddz_q_src_t* source, int64_t n, const float* const w[5], const float* const b[5],
                    float* h, int64_t h_stride, uint8_t* arg, void* stream);
int64_t ddz_q_stage_bwd_ws_bytes(int64_t n, int planes);
int ddz_q_stage_bwd(int device_id, const ddz_q_src_t* source, int64_t n, const float* gh, int64_t gh_stride, const uint8_t* arg,
                    float* const gw[5], float* const gb[5], void* ws, int64_t ws_bytes, void* stream);

/* The reference's ragged Q forward -- policy_net(face, actions) over ALL legal actions of a state (game.py:95-104,
 * dqn.py:56,67; net.py:99-101 relu(fc1) -> fc2) -- for every table at once, over the slab lists as ddz_step_slab /
 * ddz_legal_slab left them, with the first layer factorised per (rank, count) and evaluated over NEEDED rows only: nothing
 * on the host, no host-side sizes (doudizhu-rl_amd/csrc/ddz_qnet.h; BASELINE configs[2]: net.py inference in the loop):
 *   fc1 pre-activation of move j of table t = H0[t] + sum over the ranks r the move touches of D[row(t, r, cnt_jr)]
 *   H0[t] = table_term[t] + sum_r fc1_r^T Y[t][r][0]               one dense GEMM, K = 15 * 256
 *   D[row] = fc1_r^T (Y[t][r][c] - Y[t][r][0]) + z[r][c], c >= 1   only for the (r, c) some LEGAL MOVE of table t takes
 * ddz_q_need: finds those (r, c) from the slab lists (counts / rows as ddz_step_slab left them) and lays their rows out in
 *   fifteen rank segments: row_index int32 [T][64] (the row of (r < 13, c = 1..4) at column 4 r + c - 1, of a joker's count 1
 *   at column 52 / 53; -1 = not needed) and seg int32 [40] (DEVICE memory:
 *   [r] first row of rank r's segment -- a multiple of the tile, ddz_q_fc1_tile_rows() = 128 --, [15] rows in use, [16 + r] first tile of rank r, [31]
 *   tiles in use, [32] rows needed, [33] 1 if row_capacity was too small -- then status bit 1 is raised and the rows that did
 *   not fit are -1); row_cnt uint8 [row_capacity]: the count c of every needed row (ddz_q_fc1_rows adds z[rank][c]).
 *   row_capacity: rows of dy / d, a multiple of the tile, >= 15 tiles; 20 T + 15 tiles always suffices (a move
 *   takes at most what the actor holds: <= 20 cards).  scratch: ddz_q_need_scratch_bytes(T) bytes, 256-byte aligned.
 * ddz_q_features_needed: the first layer (as ddz_q_features) into y0 f32 [T][15 * 256] (count 0 of every rank: the dense
 *   GEMM's left operand) and dy f32 [row_capacity][256] (Y[t][r][c] - Y[t][r][0] at the row of every needed (t, r, c)).
 * ddz_q_fc1_dense: c f32 [n_rows][256] += a f32 [n_rows][k] x w f32 [k][256] (k a multiple of 16); ddz_q_fc1_rows:
 *   d[row] = dy[row] x w2[rank of the row] + z[rank][row_cnt[row]] (w2 f32 [15][256][256], input-major; z f32 [15][5][256]: the
 *   action plane's own path through conv_shunzi and fc1, weights only), rows and ranks from seg -- both one launch
 *   of a hand-written fp32 MFMA kernel (v_mfma_f32_32x32x2_f32: exact f32, a k-ordered fmaf chain; no library GEMM).
 * ddz_q_slab_needed: the per-row stage from h0 f32 [T][256], d and row_index: q[t * stride + j] = b2[0] + w2 . relu(fc1
 *   pre-activation of move j of table t) for j < counts[t] (entries beyond counts[t] are left alone) -- what
 *   ddz_policy_step_slab / ddz_select_slab take.  hidden must be 256 (net.py:147); w2 f32 [hidden], b2 f32 [1]: DEVICE
 *   memory.  A table's needed rows are staged in LDS once (every move that takes that count of the rank uses the row); a
 *   move whose (r, c) has no row (a list that does not belong to this row_index) contributes nothing for that rank and
 *   raises status bit 5.
 * fp32 throughout (tests: 1e-5 against the literal nn.Conv2d network; and every kernel of this forward alone, EXACTLY,
 * on integer / dyadic operands whose partial sums fp32 represents -- equal to an fp64 statement of the formulas above
 * whatever the summation order -- and within gamma_n * sum |terms| of it on random operands:
 * tests/test_gpu_q_kernels.py against tests/q_reference.py, the whole forward on an integer network included). */
int ddz_q_fc1_tile_rows(void);   /* rows per tile of the fc1 kernel: segment starts and row_capacity are multiples of it */
int64_t ddz_q_need_scratch_bytes(int64_t n_tables);
int ddz_q_need(ddz_env_t* env, const int32_t* counts, const int8_t* rows, int64_t stride, int64_t row_capacity, void* scratch,
               int64_t scratch_bytes, int32_t* row_index, int32_t* seg, uint8_t* row_cnt, void* stream);
int ddz_q_features_needed(int device_id, const float* face, int64_t n_tables, int planes, const float* wf, const float* bias,
                          const float* acnt, const int32_t* row_index, float* y0, float* dy, int64_t row_capacity, void* stream);
int ddz_q_fc1_dense(int device_id, const float* a, int64_t n_rows, int64_t k, const float* w, float* c, void* stream);
int ddz_q_fc1_rows(int device_id, const float* dy, const int32_t* seg, const uint8_t* row_cnt, const float* w2, const float* z,
                   float* d, int64_t row_capacity, void* stream);
int ddz_q_slab_needed(ddz_env_t* env, const float* h0, const float* d, int64_t row_capacity, const int32_t* row_index,
                      int64_t hidden, const float* w2, const float* b2, const int32_t* counts, const int8_t* rows,
                      int64_t stride, float* q, void* stream);

/* H0 from SHARED rows (doudizhu-rl_amd/csrc/ddz_qnet.h section 5; the same forward, net.py:81-102, for faces of
 * EnvCooperationSimplify, envi.py:201-217): Y[t][r][0] depends only on the face column of rank r, i.e. on (hand_r, taken_r,
 * b1_r, b2_r) and -- through n / (n1 + n2), and only where hand_r + taken_r < total -- on (n1, n2) reduced by their gcd; across
 * the tables of a batch those columns repeat (3.6 % distinct at 65,536 tables).  One row per
 * DISTINCT (rank, column): first layer + G[row] = Y[row] x fc1[rank] (ddz_q_fc1_rows with z = row_cnt = NULL), then
 * H0[t] = table_term[t] + sum_r G[rows[t][r]] -- instead of the K = 15 * 256 dense product.  Exact per call (nothing is kept
 * between calls), equal to the dense form up to fp32 summation order.
 * ddz_q_shared_rows: from env's CURRENT state: rows int32 [T][16] (row of (t, r); column 15 = -1), rep int32 [row_capacity]
 *   (row -> a (table, rank) instance 16 t + r that has this column; -1 = padding), seg int32 [40] as ddz_q_need's (rank
 *   segments, starts multiples of the tile).  row_capacity: a multiple of the tile, >= min(15 T, 4134375) + 15 tiles (then
 *   nothing can overflow).  ws: ddz_q_shared_ws_bytes() bytes (16.6 MB: one int32 slot per possible (rank, column)), 16-byte
 *   aligned, contents irrelevant on entry.  Row numbers follow the key order: deterministic.
 *   DOMAIN: byte 15 of a hand row (the cards left) <= 20, as in every state play reaches.  The table has 21 x 21 codes for
 *   (n1, n2), so a larger byte is read as 20: the row is still inside its rank's segment and nothing is indexed outside, but
 *   it is shared with the tables of the saturated key, and whichever instance becomes rep[row] lends ALL of them its column
 *   ((25, 5) shares the row of (20, 5): 0.8 and 0.8333333 in ddz_observe's face, one of the two in the row).  Count bytes
 *   above 4 and a role byte above 2 are inside the domain (they read as 4 / role 0, as in ddz_observe).
 * ddz_q_shared_rows_hashed: the same outputs for the faces of EnvComplicated (variant 1, 7 planes: hand, taken, the three
 *   history planes, the two prob planes) and EnvCooperation (variant 2, 9 planes: + the two recent-handout planes), whose
 *   columns are too many to address directly (517 M for variant 2): the key (rank, hand_r, taken_r, the three history counts
 *   of rank r[, the two recent-handout counts], each saturated at 4, and the canonical (n1, n2) as above) is hashed into an
 *   open-addressed table with one region per rank (ddz_qnet.h section 5b).  The same DOMAIN as ddz_q_shared_rows: cards left
 *   <= 20; a larger byte is read as 20 and the row is shared with the saturated key's tables.  variant must be 1 or 2 (else
 *   DDZ_EINVAL).
 *   row_capacity: a multiple of the tile, >= 15 T + 15 tiles (else DDZ_ECAP).  ws: ddz_q_shared_hash_ws_bytes(T) bytes
 *   (12 bytes per slot, 15 regions of max(2048, pow2 >= 2 T) slots: 23.6 MB at 65,536 tables), 16-byte aligned, contents
 *   irrelevant on entry.  Row numbers follow the slot order, which under hash collisions depends on which insert wins: the
 *   numbering is NOT deterministic, the values computed from it are (a row's G and D depend only on its column and rank).
 * ddz_q_features_rows: ys f32 [row_capacity][ys_ld] (ys_ld 256, or 256 + ceil16(4 planes): 288 for 6 / 7 planes, 304 for 9) =
 *   first layer (count 0) of every row's column, read from `face` f32 [T][planes][15][4] at rep[row]; padding rows = 0.  planes
 *   must be 6, 7 or 9 (the faces whose columns ddz_q_shared_rows / ddz_q_shared_rows_hashed key).
 * ddz_q_gather_h0: h0 f32 [T][256] += sum over r = 0..14 (in this order) of g[rows[t][r]] (g f32 [g_rows][256]; rows < 0 or
 *   >= g_rows contribute nothing).
 * ddz_q_features_needed with y0 = NULL then evaluates only the ranks a legal move takes cards of (dy alone). */
/* The needed rows shared as well (ddz_qnet.h section 6): D[(t, r, c)] depends on (rank, column, c) only -- one D row per
 * distinct (shared row, count) some table needs.
 * ddz_q_shared_need: row_index (ddz_q_need's: >= 0 <=> (t, r, c) is needed), rows / sseg (ddz_q_shared_rows') -> row_index2
 *   int32 [T][64] (the D row of every needed (t, r, c); -1 otherwise: what ddz_q_slab_needed indexes d with), drep int32
 *   [row_capacity] (D row -> 4 * shared row + c - 1; -1 = padding), dseg int32 [40] (rank segments of the D rows, as seg),
 *   row_cnt uint8 [row_capacity] (c of every D row, for ddz_q_fc1_rows' z fold).  row_capacity as ddz_q_need's (distinct
 *   pairs never outnumber the needed triples).  ws: ddz_q_shared_need_ws_bytes(shared_row_capacity) bytes, 16-byte aligned.
 * ddz_q_features_drows: dy f32 [row_capacity][256] = Y[c] - Y[0] of every D row's column (face read at the shared row's
 *   representative rep[]); padding rows = 0.  planes must be 6, 7 or 9. */
int64_t ddz_q_shared_need_ws_bytes(int64_t shared_row_capacity);
int ddz_q_shared_need(ddz_env_t* env, const int32_t* row_index, const int32_t* rows, const int32_t* sseg,
                      int64_t shared_row_capacity, void* ws, int64_t ws_bytes, int64_t row_capacity, int32_t* row_index2,
                      int32_t* drep, int32_t* dseg, uint8_t* row_cnt, void* stream);
int ddz_q_features_drows(int device_id, const float* face, int64_t n_tables, int planes, const float* wf, const float* bias,
                         const float* acnt, const int32_t* rep, int64_t shared_row_capacity, const int32_t* drep,
                         const int32_t* dseg, float* dy, int64_t row_capacity, void* stream);
int64_t ddz_q_shared_ws_bytes(void);
int ddz_q_shared_rows(ddz_env_t* env, void* ws, int64_t ws_bytes, int64_t row_capacity, int32_t* rows, int32_t* rep,
                      int32_t* seg, void* stream);
int64_t ddz_q_shared_hash_ws_bytes(int64_t n_tables);
int ddz_q_shared_rows_hashed(ddz_env_t* env, int variant, void* ws, int64_t ws_bytes, int64_t row_capacity, int32_t* rows,
                             int32_t* rep, int32_t* seg, void* stream);
int ddz_q_features_rows(int device_id, const float* face, int64_t n_tables, int planes, const float* wf, const float* bias,
                        const int32_t* rep, const int32_t* seg, float* ys, int64_t ys_ld, int64_t row_capacity, const float* mz,
                        float* g, void* stream);
int ddz_q_gather_h0(int device_id, const float* g, int64_t g_rows, const int32_t* rows, int64_t n_tables, const float* base,
                    float* h0, void* stream);
/* The table term folded into the rows: it is linear in the face (fc1 bias + the face part of conv_shunzi through fc1), i.e.
 * base + sum_r column_r x mz[p * 60 + 4 r + w] (mz f32 [60 * 6][256]: the operand of the [T, 360] x [360, 256] GEMM it
 * replaces).  ddz_q_features_rows with ys_ld = 288 appends the row's 24 column values (plane-major; then 8 zeros) behind its
 * 256 first-layer values; ddz_q_fc1_rows_k(k = 288): g[row] (+)= y[row] x w2k[rank] with w2k f32 [15][k][256] = fc1's block of
 * the rank, then the rank's 24 rows of mz, then zeros -- ONE product per row gives both terms; ddz_q_gather_h0 with base f32
 * [256] (or NULL: h0 += ...): h0[t] = base + sum_r g[rows[t][r]].  (ys_ld = 256 with mz / g: the product of the column is
 * written into g instead and the GEMM accumulates -- the same values, one more pass over g.) */
int ddz_q_fc1_rows_k(int device_id, const float* y, int64_t k, const int32_t* seg, const float* w2k, float* g,
                     int64_t row_capacity, int accumulate, void* stream);

/* Per-role networks in ONE shared-rows forward (ddz_qnet.h section 7; the reference's Game gives every role its own network or
 * the rule agent, game.py:11-43,95-106).  net_of_role int32 [3] (host; role order 0 up, 1 lord, 2 down): a network slot 0 ..
 * n_nets - 1 per role, or -1 = the rule agent; every slot names at least one role (else DDZ_EINVAL); 1 <= n_nets <= 3.  The
 * weights are stacked slot-major, one face variant for all slots.  Every row buffer holds n_nets slot-major PARTITIONS of
 * row_capacity rows (slot s: rows [s * row_capacity, (s + 1) * row_capacity)); seg / dseg int32 [n_nets][40] hold one segment
 * table per slot in ddz_q_need's layout, RELATIVE to the slot's partition (a one-slot map writes exactly the single-network
 * words).  A table whose actor's role maps to -1 (a RULE table) takes no part: no shared row, no D row, q left alone.
 * ddz_q_roles_rows: ddz_q_shared_rows (variant 3) / ddz_q_shared_rows_hashed (1, 2) keyed by (slot, rank, column): rows int32
 *   [T][16] (ABSOLUTE shared row of (t, r); -1 for column 15 and for every column of a rule table), rep int32 [n_nets *
 *   row_capacity] (-1 = padding), seg, slot int8 [T] (the slot of every table, -1 = rule table).  row_capacity per slot as
 *   ddz_q_shared_rows' (variant 3) / ddz_q_shared_rows_hashed's (1, 2) and n_nets * row_capacity * 256 < 2^31 (else
 *   DDZ_ECAP).  ws: ddz_q_roles_ws_bytes(T, variant, n_nets) bytes = n_nets times the single-network workspace (16.5 MB /
 *   23.6 MB at 65,536 tables per slot, all of it cleared every call), 16-byte aligned.  Deterministic row numbers for variant
 *   3, not for 1 / 2 (as the single-network finders).  Every variant has ddz_q_shared_rows' DOMAIN (cards left <= 20; beyond
 *   it a row may be another table's column of the same slot and rank).
 * ddz_q_roles_features_rows / ddz_q_roles_fc1_rows_k: ddz_q_features_rows (no mz / g) / ddz_q_fc1_rows_k (no accumulate) on
 *   every slot's partition with the slot's weights: wf f32 [n_nets][planes * 4][1024], bias [n_nets][1024], ys f32 [n_nets *
 *   row_capacity][ys_ld], w2k f32 [n_nets][15][k][256], g f32 [n_nets * row_capacity][256].
 * ddz_q_roles_gather_h0: h0[t] = base[slot[t]] + sum over r = 0..14 (in this order) of g[rows[t][r]] (base f32 [n_nets][256]);
 *   rule tables' h0 rows are left alone.
 * ddz_q_roles_need: ddz_q_shared_need over the slots: row_index (ddz_q_need's, all tables), rows / sseg (ddz_q_roles_rows'),
 *   shared_row_capacity (ddz_q_roles_rows' row_capacity) -> row_index2 int32 [T][64] (ABSOLUTE D rows; -1 for every column of a
 *   rule table), drep / row_cnt [n_nets * row_capacity] (drep slot-relative: 4 * the slot's shared row + c - 1), dseg.
 *   row_capacity per slot as ddz_q_need's; ws: ddz_q_roles_need_ws_bytes(shared_row_capacity, n_nets) bytes.  Status bit 1
 *   as ddz_q_shared_need.
 * ddz_q_roles_features_drows / ddz_q_roles_fc1_rows: ddz_q_features_drows / ddz_q_fc1_rows on every slot's partition: acnt f32
 *   [n_nets][5][4][256], w2 f32 [n_nets][15][256][256], z f32 [n_nets][15][5][256], dy / d f32 [n_nets * row_capacity][256].
 * ddz_q_roles_slab: ddz_q_slab_needed with the weights of the table's slot, w2 f32 [n_nets][256], b2 f32 [n_nets] (device); d
 *   has d_rows rows.  Every q entry of a rule table is left alone and such a table raises no status bit; status bit 5 as
 *   ddz_q_slab_needed for the others.
 * Nothing crosses to the host; every launch can be captured (n_nets launches of the per-slot kernels per call).
 * Cost of the fixed partitions: every buffer is n_nets times the single-network one (ys, g, dy and d: about 4.9 GB per slot at
 * 65,536 tables for 9 planes, so 14.7 GB for three networks), and every call clears n_nets times the single-network regions
 * (finder workspace, rep, the D chain's slots and drep: 48.6 MB per slot at 65,536 tables for variants 1 / 2, 41.5 MB for 3). */
int64_t ddz_q_roles_ws_bytes(int64_t n_tables, int variant, int n_nets);
int ddz_q_roles_rows(ddz_env_t* env, int variant, const int32_t* net_of_role, int n_nets, void* ws, int64_t ws_bytes,
                     int64_t row_capacity, int32_t* rows, int32_t* rep, int32_t* seg, int8_t* slot, void* stream);
int ddz_q_roles_features_rows(int device_id, const float* face, int64_t n_tables, int planes, int n_nets, const float* wf,
                              const float* bias, const int32_t* rep, const int32_t* seg, float* ys, int64_t ys_ld,
                              int64_t row_capacity, void* stream);
int ddz_q_roles_fc1_rows_k(int device_id, int n_nets, const float* y, int64_t k, const int32_t* seg, const float* w2k, float* g,
                           int64_t row_capacity, void* stream);
int ddz_q_roles_gather_h0(int device_id, int n_nets, const float* g, int64_t g_rows, const int32_t* rows, const int8_t* slot,
                          int64_t n_tables, const float* base, float* h0, void* stream);
int64_t ddz_q_roles_need_ws_bytes(int64_t shared_row_capacity, int n_nets);
int ddz_q_roles_need(ddz_env_t* env, int n_nets, const int32_t* row_index, const int32_t* rows, const int32_t* sseg,
                     int64_t shared_row_capacity, void* ws, int64_t ws_bytes, int64_t row_capacity, int32_t* row_index2,
                     int32_t* drep, int32_t* dseg, uint8_t* row_cnt, void* stream);
int ddz_q_roles_features_drows(int device_id, const float* face, int64_t n_tables, int planes, int n_nets, const float* wf,
                               const float* bias, const float* acnt, const int32_t* rep, int64_t shared_row_capacity,
                               const int32_t* drep, const int32_t* dseg, float* dy, int64_t row_capacity, void* stream);
int ddz_q_roles_fc1_rows(int device_id, int n_nets, const float* dy, const int32_t* seg, const uint8_t* row_cnt, const float* w2,
                         const float* z, float* d, int64_t row_capacity, void* stream);
int ddz_q_roles_slab(ddz_env_t* env, int n_nets, const int8_t* slot, const float* h0, const float* d, int64_t d_rows,
                     const int32_t* row_index, int64_t hidden, const float* w2, const float* b2, const int32_t* counts,
                     const int8_t* rows, int64_t stride, float* q, void* stream);

/* The canonical action table: rows[ddz_num_actions()][16] = int8 counts[15] + category of action id
 * (rule_based/utils/card.py:34-159 order), device memory. */
int ddz_action_table(int device_id, int8_t* rows, void* stream);

/* 32-byte trajectory records -> 8-byte records (for the end-of-batch gather over xGMI: 4x fewer bytes).
 *   word 0: action id (14 bits; 0x3FFF = not an action: flags != 0, or a row outside the action space) | n_legal << 14 (9 bits) | role << 23 (2) | done << 25 |
 *           reward code << 26 (0: 0, 1: +1, 2: -1) | flags << 28 (bit0 illegal, bit1 frozen)
 *   word 1: choice + 1 (10 bits) | ply << 10 (8 bits) | episode << 18 (low 14 bits)
 * traj: u8[n][32], packed: u8[n][8], device memory. */
#define DDZ_TRAJ_PACKED_BYTES 8
int ddz_pack_trajectory(int device_id, const uint8_t* traj, int64_t n_records, uint8_t* packed, void* stream);

/* Replaces Env.step_auto (envi.py:72-77; game.py:106 for every role without a network; rule_based/rule_play.py:16-23):
 * the move of the rule-based opponent.  The native step_auto is absent from the reference; its in-repo statement is
 * RuleBasedModel.choose (rule_based/utils/rule_based_model.py:43-101) over Decomposer.get_combinations
 * (rule_based/utils/decomposer.py:17-76) and cards_value (rule_based/utils/evaluator.py:10-47), which this computes
 * -- with "decomposer spec v1"  in place of the two absent native decomposition functions.
 *   ddz_auto_choose_state: for every table whose ACTOR's role bit is set in auto_roles (bit r = role r: 0 up, 1 lord,
 *     2 down) ids[t] = the canonical id of the chosen action (0 = pass), for all other tables -1.  Feed ids to
 *     ddz_step / ddz_step_slab with DDZ_STEP_IDS: rule agents move as chosen, everybody else by the engine RNG; or
 *     merge a policy's own ids into the -1 slots first.
 *   ddz_auto_choose: the same for n independent queries (server/core.py:80-87 calls choose() on a payload):
 *     hands / lasts int8[n][16] (byte 15 ignored, `last` all-zero = lead), info u8[n][4] = cards left of role 0, 1, 2
 *     (envi.py:23 `left`) and the acting role; an invalid query (no combo, role > 2, more than 20 cards) yields
 *     DDZ_AUTO_INVALID (-2: unlike -1 it is never taken for "engine RNG" by DDZ_STEP_IDS) and status bit 2 of the handle.
 *   Both entry points may be issued on any stream, also concurrently on several streams of one handle: every launch has
 *   its own work-distribution word, zeroed on its stream (nothing for the caller to initialise or re-arm).
 *   stats (may be NULL): int64[n][2] = {combinations scored, search nodes} of the FULL enumeration per table / query.
 *     With stats == NULL the search is an exact branch and bound (subtrees whose score bound is strictly
 *     below a score already reached are skipped): the same ids from about a tenth of the nodes, 3x faster.          */
int ddz_auto_choose_state(ddz_env_t* env, int auto_roles, int32_t* ids, int64_t* stats, void* stream);
int ddz_auto_choose(int device_id, const int8_t* hands, const int8_t* lasts, const uint8_t* info, int64_t n,
                    int32_t* ids, int64_t* stats, void* stream);
/* test hook: 2 * cards_value (rule_based/utils/evaluator.py:10-47) of every action id, int8[DDZ_NUM_ACTIONS] */
int ddz_debug_cards_value(int device_id, int8_t* out, void* stream);
/* test hook: the rule agent's score of one finished combination (rule_based_model.py:60-86) on its own: in int32[n][4] =
 * {2 * sum of cards_value, 2 * smallest eligible cards_value or 127 = none, actions, following | pass allowed << 1},
 * rp f64[n] = round_penalty -> value f64[n], move int32[n] (0 = pass, 7 = the eligible move, -1 = none).  The f64
 * operations round exactly as Python's (the product small_num * rp BEFORE the subtraction): tested bit for bit.     */
int ddz_debug_auto_leaf(int device_id, const int32_t* in, const double* rp, int64_t n, double* value, int32_t* move, void* stream);
/* test hook: ddz_auto_choose_state with an explicit kernel: 1 = the sequential full-enumeration walk (cross-check),
 * 2 = the lane-parallel branch-and-bound kernel as ddz_auto_choose_state runs it (tables ordered heaviest hand first),
 * 3 = the same kernel in table order.  Same ids by construction.                                                  */
int ddz_debug_auto_choose_state(ddz_env_t* env, int kernel, int auto_roles, int32_t* ids, int64_t* stats, void* stream);
/* test hook: launch geometry of a handle (tables per wavefront 1..64, 0 = keep; block-cooperative one-table-per-wave
 * form of ddz_step_slab 0 / 1, 2 = that form with every list written by one wavefront (1: leads of 5 or more scan rounds
 * -- plane-rich hands, the lord's first lead -- are written by the whole workgroup; n > 2: from n rounds on), -1 = keep; ddz_step_slab's block work list of deals + lists -- most expensive first --
 * 0 / 1, -1 = keep).  Call right after ddz_create.  Results never depend on it; the library reads no environment
 * variables.                                                                                                     */
int ddz_debug_set_geometry(ddz_env_t* env, int tables_per_wave, int slab_coop, int slab_work_list);
/* test hook: 2 (the default) = ddz_auto_choose_state's wavefronts that run out of tables help the searches still running in
 * their workgroup; 1 = additionally the predicted-heaviest decisions (one per workgroup) are searched by their whole
 * workgroup from the start ("team first": built and measured in round 4, no gain, off by default); 0 = neither.  Same ids
 * and stats in every mode (tests compare them).                                                                    */
int ddz_debug_set_auto_teams(ddz_env_t* env, int on);

/* the bits of the device status word ("status bit k" in the comments above is bitk here, the name with the value 1 << k;
 * a continuation line belongs to the name above it):
 *   DDZ_ST_MISMATCH      bit0  enumerator/count mismatch
 *   DDZ_ST_CAPACITY      bit1  row capacity overflow
 *   DDZ_ST_BAD_LAST      bit2  invalid `last` combo
 *   DDZ_ST_AUTO_WAIT     bit3  a wait of ddz_auto_choose_state's cooperating wavefronts hit its hang guard (never in a working
 *                        launch; the ids of that launch are not to be trusted)
 *   DDZ_ST_AUTO_DEPTH    bit4  the sequential cross-check kernel's depth guard (cannot happen: at most 20 actions)
 *   DDZ_ST_Q_NO_ROW      bit5  a move of ddz_q_slab_needed (or of a network table of ddz_q_roles_slab) whose (rank, count) has no
 *                        row in row_index (-1, or at or beyond row_capacity: not dereferenced, that rank contributed nothing)
 *   DDZ_ST_DOMAIN        bit6  a running table of ddz_playout_hidden / ddz_playout_worlds outside the hidden-hand domain (its hand,
 *                        taken row and hand sizes do not add up to a deck): that table ran nothing -- and a running table of
 *                        ddz_cfr with at most DDZ_CFR_MAX_CARDS cards whose rows do not add up, or of the hidden form of
 *                        ddz_solve with at most max_cards cards whose rows do not add up
 *   DDZ_ST_CFR_CAPACITY  bit7  a table of ddz_cfr that found no workspace slot or whose forest exceeds a capacity (n = -2)
 *   DDZ_ST_SOLVE_DEPTH   bit8  a search of ddz_solve deeper than DDZ_SOLVE_MAX_DEPTH (impossible inside its domain: that root
 *                        move is left unknown)                                                                        */
enum {
  DDZ_ST_MISMATCH = 1,
  DDZ_ST_CAPACITY = 2,
  DDZ_ST_BAD_LAST = 4,
  DDZ_ST_AUTO_WAIT = 8,
  DDZ_ST_AUTO_DEPTH = 16,
  DDZ_ST_Q_NO_ROW = 32,
  DDZ_ST_DOMAIN = 64,
  DDZ_ST_CFR_CAPACITY = 128,
  DDZ_ST_SOLVE_DEPTH = 256
};
/* the status word of a handle.  Copies 4 bytes D2H on `stream` and synchronises it.    */
int ddz_status(ddz_env_t* env, int32_t* status_out, void* stream);
/* the same word for the STATELESS rule-agent entry point (ddz_auto_choose has no handle): one per device, bits as above
 * (bit 3: a cooperating wait hit its hang guard -- the ids of launches since the last call are not to be trusted).
 * Copies 4 bytes D2H on `stream`, clears the word, synchronises.                                                  */
int ddz_device_status(int device_id, int32_t* status_out, void* stream);
/* hipStreamSynchronize(stream) on the device: the ONE wait per ply of the N = 1 `Env` view (doudizhu-rl_amd/envi.py), whose
 * state / list-size buffers live in pinned host memory that the kernels write directly (envi.py:63-116 reads them back
 * after every native call).  No other entry point of this library waits for the device except ddz_status.           */
int ddz_sync(int device_id, void* stream);

/* test hook: CardGroup.to_cardgroup (card.py:327-335) of arbitrary count rows int8[n][16] ->
 * out u32[n] = category | value << 8 | len << 16, or 0xFF when the row is no combo.       */
int ddz_debug_classify(int device_id, const int8_t* rows, int64_t n, uint32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
