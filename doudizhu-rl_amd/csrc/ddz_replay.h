// ddz_replay.h -- the learner's half of Game.train on the device (game.py:90-167, dqn.py:21-48): a transition recorder and a
// packed replay ring per role.  Included from ddz_engine.hip (inside its namespace, after k_observe / face_cell).
//
// A `face` is a pure function of the table's 176-byte state row (k_observe) and an action is a canonical id, so a transition
// is kept PACKED -- two state rows, two ids, a reward, a flag, the table: 369 bytes -- and the faces are rebuilt when a batch is
// sampled (k_observe_states: face_cell, the one statement of the expression).  The same ring serves every face variant.
//
// Recorder workspace (caller-owned, zero-filled = nothing pending, every table fresh; ddz_tr_ws_bytes(T)):
//   slots uint4 [T][3][11]   the state row the role acted on last (s0 of its open transition)
//   meta  uint4 [T]          {a0 of up, of lord, of down, flags}: flags bits 0..2 = pending per role, bit 8 = a ply of the
//                            episode was played (the complement of TransitionAssembler.fresh, so that zero means fresh),
//                            bits 16..17 = the role that acted in the last ddz_tr_before
//   mark  uint32 [T]         per call: bits 0..2 = emits into ring up / lord / down, bit 3 = opens a slot, bit 4 = takes part;
//                            bytes 1..3 = how many lower tables of the table's 256-block emit into ring up / lord / down
//   blk   int32 [nb][4]      per call: emits of each 256-block per ring, then (k_tr_scan) their exclusive prefix
//   hdr   int64 [8]          per call: [k] sequence number of the ring's emit 0, [4 + k] emits dropped in front (overflow)
// Ring of one role (caller-owned, zero-filled; ddz_tr_ring_bytes(capacity), fields at ddz_tr_ring_layout's offsets):
//   count int64 (total ever written), s0 / s1 uint4 [capacity][11], a0 / a1 int32, reward f32, table int32, done u8;
//   the transition with sequence number s lives at entry s % capacity.
//
// Order: deterministic.  Emit g of a call into a ring (g = the number of lower-numbered tables that emit into that ring in
// this call: a block scan over the tables, k_tr_mark + k_tr_scan; no atomics anywhere) gets sequence number count + g.  A call
// that emits E > capacity into one ring writes its last `capacity` emits only, at count .. count + capacity - 1 (the earlier
// E - capacity are never written and take no sequence number: exactly what Replay.push keeps and where it puts it), so the
// sequence numbers one launch stores are distinct and fewer than capacity + 1: no two lanes store to one entry.
// Three launches per call, all on the caller's stream, nothing on the host: mark (thread per table), scan (one block),
// emit (16 lanes per table: lanes 0..10 move the state row 16 bytes each, lane 11 the scalars, lane 12 the table's meta).

constexpr int TR_BT = 256;        // tables per block of k_tr_mark: a rank inside the block fits a byte
constexpr int TR_SLOT_ROWS = 3 * DDZ_NFIELDS;

struct TrWs {
  uint4* slots;
  uint4* meta;
  uint32_t* mark;
  int32_t* blk;
  int64_t* hdr;
};
struct TrWsLayout { int64_t slots, meta, mark, blk, hdr, bytes, nb; };
inline int64_t tr_align(int64_t x) { return (x + 255) / 256 * 256; }
inline TrWsLayout tr_ws_layout(int64_t T) {
  TrWsLayout l;
  l.nb = (T + TR_BT - 1) / TR_BT;
  l.slots = 0;
  l.meta = tr_align(l.slots + T * TR_SLOT_ROWS * 16);
  l.mark = tr_align(l.meta + T * 16);
  l.blk = tr_align(l.mark + T * 4);
  l.hdr = tr_align(l.blk + l.nb * 16);
  l.bytes = l.hdr + 256;
  return l;
}
inline TrWs tr_bind(void* ws, const TrWsLayout& l) {
  uint8_t* p = (uint8_t*)ws;
  return TrWs{(uint4*)(p + l.slots), (uint4*)(p + l.meta), (uint32_t*)(p + l.mark), (int32_t*)(p + l.blk), (int64_t*)(p + l.hdr)};
}

struct TrRing {
  int64_t* count;
  uint4 *s0, *s1;
  int32_t *a0, *a1;
  float* reward;
  int32_t* table;
  uint8_t* done;
};
struct TrRings { TrRing r[3]; int64_t cap; };
// offsets[8]: count, s0, s1, a0, a1, reward, table, done; returns the bytes of a ring
inline int64_t tr_ring_layout(int64_t cap, int64_t* off) {
  int64_t o = 0;
  const int64_t sz[8] = {8, cap * STATE_ROW_BYTES, cap * STATE_ROW_BYTES, cap * 4, cap * 4, cap * 4, cap * 4, cap};
  for (int k = 0; k < 8; ++k) {
    if (off) off[k] = o;
    o = tr_align(o + sz[k]);
  }
  return o;
}
inline TrRing tr_ring_bind(void* ring, int64_t cap) {
  TrRing r{};
  if (!ring) return r;
  int64_t off[8];
  tr_ring_layout(cap, off);
  uint8_t* p = (uint8_t*)ring;
  r.count = (int64_t*)(p + off[0]); r.s0 = (uint4*)(p + off[1]); r.s1 = (uint4*)(p + off[2]);
  r.a0 = (int32_t*)(p + off[3]); r.a1 = (int32_t*)(p + off[4]); r.reward = (float*)(p + off[5]);
  r.table = (int32_t*)(p + off[6]); r.done = (uint8_t*)(p + off[7]);
  return r;
}

constexpr uint32_t TR_PLAYED = 0x100u;   // meta flags: a ply of the episode was played (= not fresh)

// which tables emit into which ring in this call, and their rank among the emitting tables of their block.
// AFTER = false (ddz_tr_before): gate = active u8[T] or null (all); AFTER = true (ddz_tr_after): gate = done u8[T].
template <bool AFTER>
__global__ __launch_bounds__(TR_BT) void k_tr_mark(const uint8_t* __restrict__ state, int64_t T, TrWs ws,
                                                   const uint8_t* __restrict__ gate, int trained) {
  __shared__ int sh[3][TR_BT / 64];
  const int64_t t = (int64_t)blockIdx.x * TR_BT + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t bits = 0;
  if (t < T) {
    const uint32_t flags = ws.meta[t].w;
    if (AFTER) {
      if (gate[t]) bits = (flags & 7u) | 16u;      // every pending role of a finished table closes (game.py:113-123)
    } else {
      const int role = state[t * STATE_ROW_BYTES + DDZ_F_META * 16];
      if (role <= 2 && (!gate || gate[t])) {
        bits = 16u;
        if ((trained >> role) & 1) {
          bits |= 8u;
          // the first ply of an episode has no feedback in front of it (game.py:129-130): a fresh table closes nothing
          if (((flags >> role) & 1u) && (flags & TR_PLAYED)) bits |= 1u << role;
        }
      }
    }
  }
  uint32_t word = bits;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t b = __ballot((bits >> k) & 1u);
    const int pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) sh[k][wv] = __popcll(b);
    __syncthreads();
    int wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TR_BT / 64; ++w) {
      if (w < wv) wbase += sh[k][w];
      tot += sh[k][w];
    }
    word |= (uint32_t)(wbase + pre) << (8 + 8 * k);   // <= 255 lower tables in the block (read only where bit k is set)
    if (threadIdx.x == 0) ws.blk[4 * (int64_t)blockIdx.x + k] = tot;
  }
  if (t < T) ws.mark[t] = word;
}

// block totals -> exclusive prefix; the rings' counts move on.  One block.
__global__ __launch_bounds__(TR_BT) void k_tr_scan(TrWs ws, int64_t nb, TrRings rings) {
  __shared__ int sh[TR_BT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < 3; ++k) {
    long long carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += TR_BT) {
      const int64_t i = c0 + threadIdx.x;
      const int v = i < nb ? ws.blk[4 * i + k] : 0;
      const int incl = wave_incl_scan(v, lane);
      if (lane == 63) sh[wv] = incl;
      __syncthreads();
      int wbase = 0, tot = 0;
#pragma unroll
      for (int w = 0; w < TR_BT / 64; ++w) {
        if (w < wv) wbase += sh[w];
        tot += sh[w];
      }
      if (i < nb) ws.blk[4 * i + k] = (int32_t)(carry + wbase + incl - v);   // (<= T <= 2^30)
      carry += tot;
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      int64_t* cnt = rings.r[k].count;
      const long long old = cnt ? *cnt : 0;
      const long long drop = carry > rings.cap ? carry - rings.cap : 0;
      ws.hdr[k] = old - drop;          // sequence number of emit g: hdr[k] + g, for g >= drop
      ws.hdr[4 + k] = cnt ? drop : carry;   // (a role without a ring drops everything)
      if (cnt) *cnt = old + carry - drop;
    }
  }
}

struct TrAfter { float reward[3]; int quirk; };

template <bool AFTER>
__global__ __launch_bounds__(BLOCK) void k_tr_emit(const uint8_t* __restrict__ state, int64_t T, TrWs ws, TrRings rings,
                                                   const int32_t* __restrict__ chosen, const int32_t* __restrict__ greedy,
                                                   const int8_t* __restrict__ r, TrAfter af) {
  const int64_t idx = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t t = idx >> 4;
  const int l = (int)(idx & 15);
  if (t >= T) return;
  const uint32_t m = ws.mark[t];
  if (!(m & 16u)) return;
  const uint4* st = (const uint4*)(state + t * STATE_ROW_BYTES);
  uint4* sl = ws.slots + t * TR_SLOT_ROWS;
  uint4 meta = ws.meta[t];
  const int32_t a0s[3] = {(int32_t)meta.x, (int32_t)meta.y, (int32_t)meta.z};
  uint4 cur = make_uint4(0, 0, 0, 0);
  if (l < DDZ_NFIELDS) cur = st[l];
  const int64_t b = t / TR_BT;
  const int role = AFTER ? 0 : (int)state[t * STATE_ROW_BYTES + DDZ_F_META * 16];   // (<= 2: k_tr_mark took the table)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!((m >> k) & 1u) || !rings.r[k].count) continue;
    const long long g = (long long)ws.blk[4 * b + k] + ((m >> (8 + 8 * k)) & 255u);
    if (g < ws.hdr[4 + k]) continue;                       // overflow: only the last `capacity` emits are written
    int64_t e = (int64_t)((ws.hdr[k] + g) % rings.cap);
    if (e < 0) e += rings.cap;                              // (a count the caller did not zero: still inside the ring)
    const TrRing& q = rings.r[k];
    if (l < DDZ_NFIELDS) {
      q.s0[e * DDZ_NFIELDS + l] = sl[k * DDZ_NFIELDS + l];
      q.s1[e * DDZ_NFIELDS + l] = cur;
    } else if (l == 11) {
      q.a0[e] = a0s[k];
      q.table[e] = (int32_t)t;
      if (AFTER) {
        // winners +reward, losers -reward; the two farmers are one side (game.py:113-123); a1 = the pass = zeros[15,4]
        const bool lord_won = r[t] < 0;
        q.a1[e] = 0;
        q.reward[e] = (lord_won == (k == 1)) ? af.reward[k] : -af.reward[k];
        q.done[e] = 1;
      } else {
        q.a1[e] = greedy[t];
        q.reward[e] = 0.f;
        q.done[e] = 0;
      }
    }
  }
  if (AFTER) {
    if (l == 12) {
      if (!af.quirk) meta.w &= ~7u;
      meta.w &= ~TR_PLAYED;
      ws.meta[t] = meta;
    }
  } else {
    if ((m & 8u) && l < DDZ_NFIELDS) sl[role * DDZ_NFIELDS + l] = cur;
    if (l == 12) {
      if (m & 8u) {
        const uint32_t c = (uint32_t)chosen[t];
        if (role == 0) meta.x = c; else if (role == 1) meta.y = c; else meta.z = c;
        meta.w |= 1u << role;
      }
      meta.w = (meta.w & ~0x30000u) | TR_PLAYED | ((uint32_t)role << 16);
      ws.meta[t] = meta;
    }
  }
}

// face f32 [n][P][15][4] of the state rows states[index[i]] (index null: states[i]): k_observe's expression on rows that are
// not an environment's -- the s0 / s1 of a replay batch.  A negative index reads row 0.
template <int VARIANT>
__global__ __launch_bounds__(BLOCK) void k_observe_states(const uint8_t* __restrict__ states, const int64_t* __restrict__ index,
                                                          int64_t n, float4* __restrict__ out) {
  constexpr int P = VARIANT == 0 ? 4 : VARIANT == 1 ? 7 : VARIANT == 2 ? 9 : 6;
  const int64_t idx = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= n * (P * 15)) return;
  int64_t i;
  int rem;
  face_split<P>(idx, n, i, rem);
  int64_t src = index ? index[i] : i;
  if (src < 0) src = 0;
  store_stream(&out[idx], face_cell<VARIANT>(states + src * STATE_ROW_BYTES, rem));
}
