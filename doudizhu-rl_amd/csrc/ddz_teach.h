// ddz_teach.h -- teacher targets on the device (teacher spec v1): the root statistics of any evaluator (a wins
// count `num` and a denominator per entry of a slab list) become entries of the return rings of ddz_returns.h, one per
// qualifying move of every selected table: (the table's state row, ids[j], ret = reward[k] * (2 num - p) / p, table, togo 0)
// with p = (den - unknown) * scale.  Included from ddz_engine.hip (inside its namespace, after ddz_returns.h: the rings are
// McRing, the scan of the block totals is k_tr_scan itself, the overflow rule is ddz_replay.h's).
//
// Workspace (caller-owned, per call only, nothing in it has to be initialised; ddz_teach_ws_bytes(T)):
//   rank  int32 [T][4]    [k of the table's own role] how many emits into ring k the lower tables of the table's 256-block
//                         make; [3] the table's own emits (0: it takes no part); the other two are not written
//   blk   int32 [nb][4]   emits of each 256-block per ring, then (k_tr_scan) their exclusive prefix
//   hdr   int64 [8]       [k] sequence number of the ring's emit 0, [4 + k] emits dropped in front (overflow, or no ring)
//
// Three launches.  k_teach_mark: a block owns the 256 tables of one scan block; its first 256 threads read the tables' counts,
// role byte and active byte (one thread per table: the header, never the list), then each of the block's 16 wavefronts counts
// the qualifying entries of 16 tables, a wavefront per table, 64 entries of den / unknown per load, the count the popcount of
// the ballot (a uniform value: no reduction).  Where neither den nor unknown is given every entry of a table qualifies or
// none does and no list is read at all.  Then the block scan of k_mc_mark, for the table's own role alone.  k_tr_scan is
// unchanged.  k_teach_emit: a wavefront per table.  A table that takes no part leaves after its counts / role / active reads,
// one whose emits are all dropped (overflow, no ring) after its rank read.  Otherwise lanes 0..10 of each of the wavefront's
// four 16-lane groups hold the table's row (one load), and per 64 entries of the list: one coalesced load of den / unknown /
// num / ids, ret in the entry's own lane, the ballot of the qualifying lanes -- its mbcnt prefix plus the popcounts of the
// chunks in front is the entry's rank in the table, recomputed here, never stored -- and the set bits of the ballot go to the
// four groups in turn, four entries per round: the group fetches the entry's id and ret from its lane (a bpermute) and
// lanes 0..10 store the row, lane 11 the scalars.  Why a wavefront per table and not a block of 16 tables sharing its groups
// (k_mc_emit) or 16-lane groups per table: the ballot is a wavefront's, so the rank prefix is one instruction and the mask is
// uniform -- every group reads its entry out of scalar registers, no LDS, no barrier; lists are ragged (1..497, mostly a few
// dozen), a 64-entry chunk covers most of them in one 256-byte load per array, and four groups storing 4 x 189 bytes per
// round keep the stores, which are the bulk of the traffic, as wide as k_mc_emit's.  No atomics, nothing on the host; overflow
// drops by sequence number, so no two lanes store to one ring entry.

struct TeachWs {
  int32_t* rank;
  int32_t* blk;
  int64_t* hdr;
};
struct TeachWsLayout { int64_t rank, blk, hdr, bytes, nb; };
inline TeachWsLayout teach_ws_layout(int64_t T) {
  TeachWsLayout l;
  l.nb = (T + TR_BT - 1) / TR_BT;
  l.rank = 0;
  l.blk = tr_align(l.rank + T * 16);
  l.hdr = tr_align(l.blk + l.nb * 16);
  l.bytes = l.hdr + 256;
  return l;
}

struct TeachArgs {
  const int32_t* counts;
  const int32_t* ids;
  const int32_t* num;
  const int32_t* den;
  const int32_t* unknown;
  const uint8_t* active;
  int64_t stride;
  int32_t den_const, scale, min_den;
  int trained;
  float reward[3];
};

constexpr int TEACH_MARK_THREADS = 1024;                       // 16 wavefronts for the 256 tables of a scan block
constexpr int TEACH_MARK_TPW = TR_BT / (TEACH_MARK_THREADS / 64);   // tables per wavefront of k_teach_mark

// entries of table t's list that the call reads: min(counts, stride) where the table takes part, else 0; *role: its role
__device__ __forceinline__ int teach_list(const uint8_t* __restrict__ state, const TeachArgs& a, int64_t t, int* role) {
  const int n = a.counts[t];
  const int k = state[t * STATE_ROW_BYTES + DDZ_F_META * 16];
  *role = k;
  if (n <= 0 || k > 2 || !((a.trained >> k) & 1) || (a.active && !a.active[t])) return 0;
  return (int)min((int64_t)n, a.stride);
}

// d of entry i (an index into the slab arrays): the denominator the entry is judged and divided by
__device__ __forceinline__ int64_t teach_den(const TeachArgs& a, int64_t i) {
  return (int64_t)(a.den ? a.den[i] : a.den_const) - (a.unknown ? a.unknown[i] : 0);
}

__global__ __launch_bounds__(TEACH_MARK_THREADS) void k_teach_mark(const uint8_t* __restrict__ state, int64_t T, TeachWs ws,
                                                                   TeachArgs a) {
  __shared__ int sh_n[TR_BT], sh_e[TR_BT];
  __shared__ int sh[3][TR_BT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * TR_BT;
  const int64_t t = t0 + tid;
  int role = 3, n = 0;
  if (tid < TR_BT) {
    if (t < T) n = teach_list(state, a, t, &role);
    sh_n[tid] = n;
    // without a per-entry denominator a table's entries qualify together
    sh_e[tid] = (a.den || a.unknown) ? 0 : (a.den_const >= a.min_den ? n : 0);
  }
  __syncthreads();
  if (a.den || a.unknown) {
    for (int i = wv * TEACH_MARK_TPW; i < (wv + 1) * TEACH_MARK_TPW; ++i) {
      const int ni = sh_n[i];                                 // (uniform)
      if (ni == 0) continue;
      const int64_t o = (t0 + i) * a.stride;
      int e = 0;
      for (int c = 0; c < ni; c += 64) {
        const int j = c + lane;
        e += __popcll(__ballot(j < ni && teach_den(a, o + j) >= a.min_den));
      }
      if (lane == 0) sh_e[i] = e;
    }
    __syncthreads();
  }
  // the block scan of k_mc_mark over the first four wavefronts' tables (the others carry zeros: every thread meets the barrier)
  const bool head = tid < TR_BT;
  const int mine = head ? sh_e[tid] : 0;
  int e[3], incl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[k] = role == k ? mine : 0;
    incl[k] = wave_incl_scan(e[k], lane);
    if (head && lane == 63) sh[k][wv] = incl[k];
  }
  __syncthreads();
  if (!head) return;
  int before = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TR_BT / 64; ++w) {
      if (w < wv) wbase += sh[k][w];
      tot += sh[k][w];
    }
    if (role == k) before = wbase + incl[k] - e[k];
    if (tid == 0) ws.blk[4 * (int64_t)blockIdx.x + k] = tot;  // (<= 256 * stride: T * stride < 2^31)
  }
  if (t < T) {
    if (role <= 2) ws.rank[4 * t + role] = before;
    ws.rank[4 * t + 3] = mine;
  }
}

__global__ __launch_bounds__(BLOCK) void k_teach_emit(const uint8_t* __restrict__ state, int64_t T, TeachWs ws, McRings rings,
                                                      TeachArgs a) {
  const int lane = threadIdx.x & 63, grp = lane >> 4, l = lane & 15;
  const int64_t t = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (t >= T) return;
  int k;
  const int n = teach_list(state, a, t, &k);                  // (uniform: one table per wavefront)
  if (n == 0) return;
  const int total = ws.rank[4 * t + 3];
  const McRing q = k == 0 ? rings.r[0] : k == 1 ? rings.r[1] : rings.r[2];
  const long long base = (long long)ws.blk[4 * (t / TR_BT) + k] + ws.rank[4 * t + k];
  const long long drop = ws.hdr[4 + k], seq0 = ws.hdr[k];
  // nothing qualifies, no ring, or overflow: only the last `capacity` emits of a call are written
  if (total == 0 || !q.count || base + total <= drop) return;
  const float rew = k == 0 ? a.reward[0] : k == 1 ? a.reward[1] : a.reward[2];
  uint4 row = make_uint4(0, 0, 0, 0);
  if (l < DDZ_NFIELDS) row = ((const uint4*)(state + t * STATE_ROW_BYTES))[l];
  const int64_t o = t * a.stride;
  int done = 0;                                               // qualifying entries of the chunks in front
  for (int c = 0; c < n; c += 64) {
    const int j = c + lane;
    bool ok = false;
    int id = 0;
    float ret = 0.f;
    if (j < n) {
      const int64_t d = teach_den(a, o + j);
      if (d >= a.min_den) {
        ok = true;
        const int64_t p = d * a.scale;
        id = a.ids[o + j];
        ret = __fmul_rn(rew, __fdiv_rn(__ll2float_rn(2 * (int64_t)a.num[o + j] - p), __ll2float_rn(p)));
      }
    }
    uint64_t m = __ballot(ok);
    const int here = __popcll(m);
    for (int r = 0; r < here; r += 4) {                       // four entries per round, one per lane group
      int src = -1;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int s = m ? (int)__builtin_ctzll(m) : -1;
        m &= m - 1;
        if (g == grp) src = s;
      }
      const int id_s = __shfl(id, src < 0 ? 0 : src);
      const float ret_s = __shfl(ret, src < 0 ? 0 : src);
      const long long g = base + done + r + grp;
      if (src >= 0 && g >= drop) {
        int64_t e = (int64_t)((seq0 + g) % rings.cap);
        if (e < 0) e += rings.cap;                            // (a count the caller did not zero: still inside the ring)
        if (l < DDZ_NFIELDS) {
          q.s0[e * DDZ_NFIELDS + l] = row;
        } else if (l == 11) {
          q.a0[e] = id_s;
          q.ret[e] = ret_s;
          q.table[e] = (int32_t)t;
          q.togo[e] = 0;
        }
      }
    }
    done += here;
  }
}
