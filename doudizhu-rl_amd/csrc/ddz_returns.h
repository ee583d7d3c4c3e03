// ddz_returns.h -- Monte-Carlo return targets on the device (return spec v1): an episode log per table and a packed
// ring per role of (state row, action id, the episode's discounted return).  Included from ddz_engine.hip (inside its
// namespace, after ddz_replay.h: the scan of the block totals is k_tr_scan itself, the rings' overflow rule is its rule).
//
// A decision's return is known when its game ends, so ddz_mc_before appends (state row, action id, role, the role's decision
// ordinal) to the table's log and ddz_mc_after turns the log of every finished table into ring entries: entry (role k, ordinal
// j) of a table whose role k decided c[k] times has togo = c[k] - 1 - j decisions of the role behind it and
// ret = (+/-reward[k]) * gamma^togo, by togo f32 multiplications.
//
// Workspace (caller-owned, zero-filled = every log empty; ddz_mc_ws_bytes(T, log_cap), log_cap = L in 1..255, T * L <= 2^30):
//   rows  uint4  [T][L][11]  the state row of log entry p of table t
//   act   int32  [T][L]      its action id
//   who   u8     [T][L][2]   {role, ordinal}: the role that decided and how many decisions of that role came before it
//   cnt   u8     [T][4]      {n, c of up, c of lord, c of down}: n = entries in the log, c[k] = decisions of role k in the episode,
//                            logged or not (saturating at 255)
//   lost  uint32 [T]         cumulative: decisions that were not logged because the log was full (saturating)
//   rank  int32  [T][4]      per call: how many emits into ring up / lord / down the lower tables of the table's 256-block make
//   blk   int32  [nb][4]     per call: emits of each 256-block per ring, then (k_tr_scan) their exclusive prefix
//   hdr   int64  [8]         per call: [k] sequence number of the ring's emit 0, [4 + k] emits dropped in front (overflow)
// Ring of one role (caller-owned, zero-filled; ddz_mc_ring_bytes(capacity), fields at ddz_mc_ring_layout's offsets):
//   count int64 (total ever written), s0 uint4 [capacity][11], a0 int32, ret f32, table int32, togo u8;
//   the entry with sequence number s lives at entry s % capacity.
//
// A log is a prefix of its episode's decisions (once it is full every later decision is lost), so of a logged entry (k, j) the j
// earlier decisions of role k are logged too: j is also the entry's rank among the table's emits into ring k, and the entries
// of a log are independent of each other.
//
// ddz_mc_before is one launch, 16 lanes per table: lanes 0..10 move the row 16 bytes each, lane 11 the scalars, lane 12 the
// counters.  ddz_mc_after is three: k_mc_mark (a thread per table: the emits of a finished table per role -- c[k] itself unless
// the log overflowed, then a count over the log; ranks and block totals as int32, a table emits up to L), k_tr_scan (unchanged)
// and k_mc_emit.  The emit's work follows the finished tables (about 1 table in 65 per iteration): a block owns 16 tables, reads
// their done bytes, and its 16 lane groups share the entries of the block's finished tables -- entry p of a log goes to group
// p % 16, whose lanes 0..10 move the row and lane 11 the scalars; a block without a finished table leaves after one barrier.
// Weighed against (a) a launch of T * L lane groups, which finds the same entries with all but n lane groups per finished
// table idle, and (b) one lane group per table walking its own log, whose time is the longest log's chain of dependent loads
// and stores (measured: profiles/r20_notes.md).  Order and overflow as ddz_replay.h: emit g of a call into a ring (ascending
// table, then ascending log position) gets sequence number count + g; of E > capacity emits only the last `capacity` are
// written, so no two lanes store to one entry.  No atomics, nothing on the host, everything uniform across a lane group in
// plain C++.

struct McWs {
  uint4* rows;
  int32_t* act;
  uint8_t* who;
  uint32_t* cnt;
  uint32_t* lost;
  int32_t* rank;
  int32_t* blk;
  int64_t* hdr;
};
struct McWsLayout { int64_t rows, act, who, cnt, lost, rank, blk, hdr, bytes, nb; };
inline McWsLayout mc_ws_layout(int64_t T, int64_t L) {
  McWsLayout l;
  l.nb = (T + TR_BT - 1) / TR_BT;
  l.rows = 0;
  l.act = tr_align(l.rows + T * L * STATE_ROW_BYTES);
  l.who = tr_align(l.act + T * L * 4);
  l.cnt = tr_align(l.who + T * L * 2);
  l.lost = tr_align(l.cnt + T * 4);
  l.rank = tr_align(l.lost + T * 4);
  l.blk = tr_align(l.rank + T * 16);
  l.hdr = tr_align(l.blk + l.nb * 16);
  l.bytes = l.hdr + 256;
  return l;
}
inline McWs mc_bind(void* ws, const McWsLayout& l) {
  uint8_t* p = (uint8_t*)ws;
  return McWs{(uint4*)(p + l.rows), (int32_t*)(p + l.act), p + l.who, (uint32_t*)(p + l.cnt), (uint32_t*)(p + l.lost),
              (int32_t*)(p + l.rank), (int32_t*)(p + l.blk), (int64_t*)(p + l.hdr)};
}

struct McRing {
  int64_t* count;
  uint4* s0;
  int32_t* a0;
  float* ret;
  int32_t* table;
  uint8_t* togo;
};
struct McRings { McRing r[3]; int64_t cap; };
// offsets[6]: count, s0, a0, ret, table, togo; returns the bytes of a ring
inline int64_t mc_ring_layout(int64_t cap, int64_t* off) {
  int64_t o = 0;
  const int64_t sz[6] = {8, cap * STATE_ROW_BYTES, cap * 4, cap * 4, cap * 4, cap};
  for (int k = 0; k < 6; ++k) {
    if (off) off[k] = o;
    o = tr_align(o + sz[k]);
  }
  return o;
}
inline McRing mc_ring_bind(void* ring, int64_t cap) {
  McRing r{};
  if (!ring) return r;
  int64_t off[6];
  mc_ring_layout(cap, off);
  uint8_t* p = (uint8_t*)ring;
  r.count = (int64_t*)(p + off[0]); r.s0 = (uint4*)(p + off[1]); r.a0 = (int32_t*)(p + off[2]);
  r.ret = (float*)(p + off[3]); r.table = (int32_t*)(p + off[4]); r.togo = p + off[5];
  return r;
}

// the log of every active table whose actor is a trained role takes the decision, or counts it as lost
__global__ __launch_bounds__(BLOCK) void k_mc_append(const uint8_t* __restrict__ state, int64_t T, McWs ws, int L,
                                                     const int32_t* __restrict__ chosen, const uint8_t* __restrict__ active,
                                                     int trained) {
  const int64_t idx = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t t = idx >> 4;
  const int l = (int)(idx & 15);
  if (t >= T) return;
  const int role = state[t * STATE_ROW_BYTES + DDZ_F_META * 16];
  if (role > 2 || (active && !active[t]) || !((trained >> role) & 1)) return;
  // every lane of the group loads cnt[t] here and lane 12 stores it below with no barrier between: right only because the 16
  // lanes of a table sit in ONE wavefront (16 divides 64, BLOCK is a multiple of 64), where the load precedes the divergent store
  // in program order -- as k_tr_emit treats its meta word.  A group that spanned wavefronts would need k_mc_emit's block copy.
  const uint32_t cnt = ws.cnt[t];
  const int n = (int)(cnt & 255u);
  const uint32_t c = (cnt >> (8 + 8 * role)) & 255u;
  const bool room = n < L;
  const int64_t e = t * L + n;
  if (room && l < DDZ_NFIELDS) {
    ws.rows[e * DDZ_NFIELDS + l] = ((const uint4*)(state + t * STATE_ROW_BYTES))[l];
  } else if (room && l == 11) {
    ws.act[e] = chosen[t];
    ws.who[2 * e] = (uint8_t)role;
    ws.who[2 * e + 1] = (uint8_t)c;
  } else if (l == 12) {
    const uint32_t c1 = c < 255u ? c + 1u : 255u;
    ws.cnt[t] = ((cnt & ~(255u << (8 + 8 * role))) | (c1 << (8 + 8 * role))) + (room ? 1u : 0u);
    if (!room) {
      const uint32_t lost = ws.lost[t];
      ws.lost[t] = lost == 0xFFFFFFFFu ? lost : lost + 1u;
    }
  }
}

// how many entries per role the log of each finished table emits, its rank in the 256-block and the block's totals
__global__ __launch_bounds__(TR_BT) void k_mc_mark(int64_t T, McWs ws, int L, const uint8_t* __restrict__ done) {
  __shared__ int sh[3][TR_BT / 64];
  const int64_t t = (int64_t)blockIdx.x * TR_BT + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int e[3] = {0, 0, 0};
  if (t < T && done[t]) {
    const uint32_t cnt = ws.cnt[t];
    const int n = min((int)(cnt & 255u), L);              // (n <= L unless the caller scribbled on the workspace)
    e[0] = (cnt >> 8) & 255u; e[1] = (cnt >> 16) & 255u; e[2] = cnt >> 24;
    if (e[0] + e[1] + e[2] != n) {                        // the log overflowed: count what it holds
      e[0] = e[1] = e[2] = 0;
      const uint8_t* who = ws.who + 2 * t * L;
      for (int p = 0; p < n; ++p) {
        const int k = who[2 * p];
        e[0] += k == 0; e[1] += k == 1; e[2] += k == 2;
      }
    }
  }
  int incl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    incl[k] = wave_incl_scan(e[k], lane);
    if (lane == 63) sh[k][wv] = incl[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TR_BT / 64; ++w) {
      if (w < wv) wbase += sh[k][w];
      tot += sh[k][w];
    }
    if (t < T) ws.rank[4 * t + k] = wbase + incl[k] - e[k];
    if (threadIdx.x == 0) ws.blk[4 * (int64_t)blockIdx.x + k] = tot;      // (<= 256 * L)
  }
}

struct McAfter { float reward[3]; float gamma; };

constexpr int MC_BT = BLOCK / 16;   // tables per block of k_mc_emit = its lane groups

__global__ __launch_bounds__(BLOCK) void k_mc_emit(int64_t T, McWs ws, int L, McRings rings, const uint8_t* __restrict__ done,
                                                   const int8_t* __restrict__ r, McAfter af) {
  __shared__ uint32_t sh_cnt[MC_BT];                          // {n, c[3]} of the block's finished tables, 0 of the others
  const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int64_t t0 = (int64_t)blockIdx.x * MC_BT;
  uint32_t mine = 0;
  if (t0 + grp < T && done[t0 + grp]) mine = ws.cnt[t0 + grp];
  if (l == 0) sh_cnt[grp] = mine;
  __syncthreads();
  for (int i = 0; i < MC_BT; ++i) {
    const uint32_t cnt = sh_cnt[i];
    const int n = min((int)(cnt & 255u), L);
    if (n == 0) continue;                                     // not finished, or an empty log
    const int64_t t = t0 + i;
    const bool lord_won = r[t] < 0;
    for (int p = grp; p < n; p += MC_BT) {
      const int64_t src = t * L + p;
      const int k = ws.who[2 * src], j = ws.who[2 * src + 1];
      if (k > 2) continue;                                    // (a workspace the caller scribbled on)
      const McRing q = k == 0 ? rings.r[0] : k == 1 ? rings.r[1] : rings.r[2];
      const long long g = (long long)ws.blk[4 * (t / TR_BT) + k] + ws.rank[4 * t + k] + j;
      if (!q.count || g < ws.hdr[4 + k]) continue;            // no ring, or overflow: only the last `capacity` emits are written
      int64_t e = (int64_t)((ws.hdr[k] + g) % rings.cap);
      if (e < 0) e += rings.cap;                              // (a count the caller did not zero: still inside the ring)
      if (l < DDZ_NFIELDS) {
        q.s0[e * DDZ_NFIELDS + l] = ws.rows[src * DDZ_NFIELDS + l];
      } else if (l == 11) {
        const int togo = (int)((cnt >> (8 + 8 * k)) & 255u) - 1 - j;
        // winners +reward, losers -reward; the two farmers are one side (k_tr_emit)
        const float rew = k == 0 ? af.reward[0] : k == 1 ? af.reward[1] : af.reward[2];
        float ret = (lord_won == (k == 1)) ? rew : -rew;
        for (int s = 0; s < togo; ++s) ret *= af.gamma;
        q.a0[e] = ws.act[src];
        q.ret[e] = ret;
        q.table[e] = (int32_t)t;
        q.togo[e] = (uint8_t)togo;
      }
    }
  }
  if (mine && l == 12) ws.cnt[t0 + grp] = 0;                  // (the other groups read the block's copy)
}
