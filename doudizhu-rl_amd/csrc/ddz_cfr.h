// ddz_cfr.h -- k_cfr / k_cfr_choose: the CFR endgame solver ("CFR spec v1"; the reference's final_card /
// initiate_game / VanillaCFR, server/CFR.py, with everything it leaves to chance pinned).  Included by ddz_engine.hip behind
// ddz_ply.h, inside its anonymous namespace.  The entry into a table (table_enter), the root with the domain test
// (root_hands<true>), the legal lists (ply_list / ply_entry: the device keeps one statement of the rules) and the
// wavefront-scope accesses (rfl64 / sld / sst / search_fence) are ddz_ply.h's, shared with k_playout, k_search and k_solve.
//
// One wavefront per TABLE; a table inside the domain takes one workspace SLOT from a counter at the head of the workspace
// (zeroed by k_cfr_head, a one-wave launch in front of k_cfr) and keeps it for the launch.  Seats are the reference's player
// numbers: 0 lord, 1 down, 2 up = role (seat + 1) % 3; the turn order is seat 0, 1, 2.
//
// PHASES of a wave.
//   decode   the root as k_search<true> reads it (root_hands<true>): the actor's hand row, the taken row, the
//            recent rows with their category bytes, the meta row, byte 15 of the other two hand rows -- never the opponents'
//            count bytes.
//   deals    every assignment of pool = deck - taken to the seats by per-rank counts, in CFR.py:deal's order: the pool has
//            K <= 6 distinct ranks, a deal is a mixed-radix number over them (digit = (lord's count, down's count) in
//            lexicographic order, the lowest rank the most significant), a lane decodes one number per round and a ballot
//            ranks the valid ones.  Deal d is node d.
//   forest   built ONCE, breadth-first over all deals: node i is expanded in index order, its children are appended behind
//            the last node, so every level is deal-ordered.  Wave-uniform: one node per trip, ply_list for its list,
//            ply_entry per action.  While it is built, node i's state (three hands, the combination to beat and its owner,
//            its history id and deal) lies in the 32 bytes that hold its reaches and value afterwards: no record keeps a state.
//            THE BUILD IS THE COST: it is serial in the nodes (63 lanes idle outside the list code), and one worst-case table
//            (10,512 nodes) takes 20 ms of which the eight iterations' sweeps are the small part (profiles/r14_notes.md).  Do not
//            read the lane-per-node sweeps below as the cost model.
//   sweeps   per iteration, a lane per node: the reaches level by level downwards, the values level by level upwards, then a
//            lane per information set walks its members in ascending node index (= ascending deal order), adds their
//            regrets and rewrites sigma.  Lane 0 adds the roots' values in deal order.
//
// KEY TABLES (open addressing, linear probing, full-key compare, slot = (key * 2654435761) >> (32 - log), as ddz_search.h):
//   histories     key (parent history << 14 | action id) + 1 -> history id (0 = the empty history)
//   information   key history << 16 | the mover's hand IN THE DEAL as 16 bits (nibble j = 1 + rank of its j-th lowest card)
//   Table ids only address records; no id enters a number.  The members of an information set are chained (next[node]) as
//   the forest is built, in index order.
//
// ARITHMETIC.  IEEE double, every operation rounded on its own.  `value + sigma * u` and `R + reach * (u - value)` are the
// shapes the backend contracts into one fma whatever the pragma says (ddz_auto.h:90-101), so EVERY PRODUCT THAT FEEDS A SUM
// passes through cfr_rounded(), the register barrier of auto_rounded(): in the values sweep (sigma * u) and in the regrets sweep
// (reach * (u - value)).  No floating-point atomics: R of an information set is added by ONE lane in member order.
//
// LOOPS.  All counted: rounds of deals by the 729 numbers six ranks allow, nodes by DDZ_CFR_MAX_NODES, levels by
// DDZ_CFR_MAX_DEPTH, probes by the table size, members by DDZ_CFR_MAX_DEALS, iterations by DDZ_CFR_MAX_ITERATIONS.  A wave
// waits for no other wave.
//
// MEMORY ORDERING.  As ddz_search.h: a slot is written and read by ONE wavefront, through relaxed wavefront-scope atomic
// loads / stores (vector instructions), with search_fence() between the phases, between the levels of a sweep and behind
// every node of the build.  n / ids / sigma / value leave through plain stores, the totals through 64-bit integer atomics,
// the slot counter and the status word through 32-bit ones.
//
// CAPACITIES (include/ddz_env.h).  DDZ_CFR_MAX_NODES / _INFOSETS and CFR_MAX_PAIRS / CFR_MAX_HIST are the powers of two at
// or above twice the maxima tools/cfr_sweep.py measured (10,512 nodes, 2,835 information sets, 3,993 (set, action) pairs,
// 1,860 histories: profiles/r14_notes.md).  Anything that would not fit -- and a table that finds no slot -- gives n = -2 and
// status bit 7; nothing is stored out of bounds.
//
// SLOT, CFR_SLOT_BYTES = 1,728 KiB:  32 B x 32,768 nodes of reaches and value (the build's states before) = 1 MiB; 10 B per
// node of parent / set / first child / next member / action / kind = 320 KiB; 8 B x 8,192 set records, 2 x 8 B x 8,192 R and
// sigma, 8 B x 16,384 + 8 B x 8,192 table entries = 384 KiB.  (The 1 MB the design aimed at assumed 16,384 nodes; follow roots
// doubled the measured maximum.)
struct CfrArgs : PlyArgs {   // (no draw in the solver: the key is not read)
  uint32_t iterations, roles;
  int64_t slots;
  uint8_t* work;            // 256 bytes of head (the slot counter), then slots x CFR_SLOT_BYTES
  int32_t* n;
  int32_t* ids;             // [T][DDZ_CFR_STRIDE]
  double* sigma;            // [T][DDZ_CFR_STRIDE]
  double* value;            // [T]
  unsigned long long* totals;
};

constexpr int CFR_WAVES = 4;                      // 36,464 B of LDS per block
constexpr uint32_t CFR_N = DDZ_CFR_MAX_NODES, CFR_I = DDZ_CFR_MAX_INFOSETS;
constexpr uint32_t CFR_MAX_PAIRS = 8192, CFR_MAX_HIST = 4096;
constexpr uint32_t CFR_INFO_LOG = 14, CFR_HIST_LOG = 13;      // tables of twice the capacity
static_assert((1u << CFR_INFO_LOG) == 2 * CFR_I && (1u << CFR_HIST_LOG) == 2 * CFR_MAX_HIST, "tables at most half full");
static_assert(CFR_N <= 0x8000 && CFR_I <= 0x8000 && CFR_MAX_HIST <= 0x10000 && CFR_MAX_PAIRS <= 0x10000, "16-bit ids");
static_assert(DDZ_CFR_MAX_ACTIONS <= 15 && DDZ_CFR_MAX_DEALS <= 127 && DDZ_CFR_STRIDE >= DDZ_CFR_MAX_ACTIONS, "packed fields");
constexpr uint32_t CFR_NONE = 0xFFFFu;
constexpr uint32_t CFR_HEAD_BYTES = 256;
// offsets inside a slot
constexpr uint64_t CFR_O_RA = 0, CFR_O_RB = 8ull * CFR_N, CFR_O_RC = 16ull * CFR_N, CFR_O_U = 24ull * CFR_N;
constexpr uint64_t CFR_O_PARENT = 32ull * CFR_N, CFR_O_INFO = CFR_O_PARENT + 2ull * CFR_N, CFR_O_CHILD = CFR_O_INFO + 2ull * CFR_N;
constexpr uint64_t CFR_O_NEXT = CFR_O_CHILD + 2ull * CFR_N, CFR_O_ACT = CFR_O_NEXT + 2ull * CFR_N, CFR_O_KIND = CFR_O_ACT + 1ull * CFR_N;
constexpr uint64_t CFR_O_REC = CFR_O_KIND + 1ull * CFR_N, CFR_O_R = CFR_O_REC + 8ull * CFR_I, CFR_O_SIGMA = CFR_O_R + 8ull * CFR_MAX_PAIRS;
constexpr uint64_t CFR_O_ITAB = CFR_O_SIGMA + 8ull * CFR_MAX_PAIRS, CFR_O_HTAB = CFR_O_ITAB + (8ull << CFR_INFO_LOG);
constexpr uint64_t CFR_SLOT_BYTES = CFR_O_HTAB + (8ull << CFR_HIST_LOG);
static_assert(CFR_SLOT_BYTES % 16 == 0 && CFR_O_REC % 8 == 0, "aligned fields");
// kind byte of a node: its number of actions, or a finished game
constexpr uint32_t CFR_TERM_LORD = 0x40, CFR_TERM_FARMER = 0x80;

__device__ __forceinline__ double cfr_rounded(double x) {   // the product exists, rounded, before anything consumes it
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint32_t sld16(const uint16_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ uint32_t sld8(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void sst16(uint16_t* p, uint32_t v) { __hip_atomic_store(p, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void sst8(uint8_t* p, uint32_t v) { __hip_atomic_store(p, (uint8_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ double sldf(const double* p) { return __longlong_as_double((long long)sld64((const uint64_t*)p)); }
__device__ __forceinline__ void sstf(double* p, double v) { sst64((uint64_t*)p, (uint64_t)__double_as_longlong(v)); }

// a hand of at most 4 cards in 16 bits: nibble j = 1 + the rank of its j-th lowest card
__device__ __forceinline__ uint32_t cfr_hand16(uint64_t nib) {
  uint32_t w = 0, j = 0;
  for (int r = 0; r < 15; ++r) {
    const uint32_t c = (uint32_t)(nib >> (4 * r)) & 15u;
    for (uint32_t k = 0; k < 4; ++k)
      if (k < c && j < 4) { w |= (uint32_t)(r + 1) << (4 * j); ++j; }
  }
  return w;
}

// the canonical id of a list entry of a hand of at most 4 cards (card.py:34-159): pass, a group of 1 .. 4 of one rank, the
// rocket, a triple with one kicker; -1 for anything else (no such entry exists in the domain)
__device__ __forceinline__ int cfr_action_id(uint64_t snib, uint32_t scat, uint32_t svlv) {
  const int v = (int)(svlv & 0xFFu);
  if (scat == (uint32_t)EMPTY) return 0;
  if (scat == (uint32_t)SINGLE) return 1 + v;
  if (scat == (uint32_t)DOUBLE) return 16 + v;
  if (scat == (uint32_t)TRIPLE) return 29 + v;
  if (scat == (uint32_t)QUADRIC) return 42 + v;
  if (scat == (uint32_t)BIGBANG) return ID_BIGBANG;
  if (scat == (uint32_t)THREE_ONE && v < 13) {
    const uint64_t kick = snib - (3ull << (4 * v));
    if (kick == 0) return -1;
    const int k = __builtin_ctzll(kick) >> 2;
    return ID_THREE_ONE + v * 14 + (k < v ? k : k - 1);
  }
  return -1;
}

// the id stored under `key`; where there is none, `fresh` is stored and returned (created = true).  Wave-uniform: every lane
// probes, lane 0 stores.  CFR_NONE: the table is full (cannot happen: it has twice the capacity of what it indexes).
__device__ __forceinline__ uint32_t cfr_find_or_insert(uint64_t* tab, uint32_t log, uint32_t key, uint32_t fresh, bool insert,
                                                       int lane, bool& created) {
  const uint32_t hmask = (1u << log) - 1u;
  uint32_t h = (key * 2654435761u) >> (32u - log);
  created = false;
  for (uint32_t p = 0; p <= hmask; ++p) {
    const uint64_t e = rfl64(sld64(tab + h));
    if ((uint32_t)(e >> 32) == key) return (uint32_t)e;
    if (e == 0) {
      if (!insert) return CFR_NONE;
      if (lane == 0) sst64(tab + h, ((uint64_t)key << 32) | fresh);
      search_fence();
      created = true;
      return fresh;
    }
    h = (h + 1u) & hmask;
  }
  return CFR_NONE;
}

// the workspace's head (the slot counter and its padding) is zero before k_cfr runs: one wavefront, launched in front of it
__global__ __launch_bounds__(64) void k_cfr_head(uint32_t* __restrict__ head) {
  static_assert(CFR_HEAD_BYTES == 64 * sizeof(uint32_t), "a word per lane");
  head[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(CFR_WAVES * 64) void k_cfr(CfrArgs a) {
  __shared__ HotTabT<false> hot;
  __shared__ uint64_t s_stage[CFR_WAVES][STAGE_CAP];
  __shared__ uint16_t s_svl[CFR_WAVES][STAGE_CAP];
  __shared__ uint16_t s_deal[CFR_WAVES][DDZ_CFR_MAX_DEALS * 3 + 2];   // the hands of every deal, 16 bits each
  __shared__ uint32_t s_level[CFR_WAVES][DDZ_CFR_MAX_DEPTH + 4];      // the first node of every level
  const int lane = threadIdx.x & 63;
  const int wv = (int)rfl(threadIdx.x >> 6);
  const int64_t t = (int64_t)blockIdx.x * CFR_WAVES + wv;
  uint4 R;
  if (!table_enter<CFR_WAVES>(a, t, lane, hot, R)) return;
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  uint16_t* dl = s_deal[wv];
  uint32_t* level = s_level[wv];
  // every table's output rows are written whole: ids -1, sigma 0, value 0 where nothing is solved
  int32_t* const out_ids = a.ids + t * DDZ_CFR_STRIDE;
  double* const out_sigma = a.sigma + t * DDZ_CFR_STRIDE;
  if (lane < DDZ_CFR_STRIDE) { out_ids[lane] = -1; out_sigma[lane] = 0.0; }
  if (lane == 0) { a.value[t] = 0.0; a.n[t] = 0; }
  // ---- decode (as k_search<true>)
  const RootHands rh = root_hands<true>(R, a.roles, lane);
  if (rh.kind == ROOT_IDLE) return;   // not dealt, done, or not this call's seat
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const int rnext = role_next(role0);
  const uint64_t hc0 = root.hc0;
  const int n_me = rh.n_me, n_next = rh.n_next, n_prev = rh.n_prev;
  if (n_me + n_next + n_prev > DDZ_CFR_MAX_CARDS) {   // not an endgame
    if (lane == 0) a.n[t] = -1;
    return;
  }
  // unseen_pool is the domain of this spec too: per rank `taken > deck || hand > deck - taken` is `hand + taken > deck` for
  // counts that are not negative, and where that holds for no rank deck - taken = unseen + hand without a borrow, so
  // `sum(deck - taken) != n_me + n_next + n_prev` is `sum(unseen) != n_next + n_prev`.  The actor's own hand is not empty.
  if (rh.kind == ROOT_OUTSIDE || n_me < 1) {
    if (lane == 0) { a.n[t] = -1; atomicOr(a.status, DDZ_ST_DOMAIN); }
    return;
  }
  const uint64_t pool = rh.unseen + hc0;   // deck - taken
  // the combination to beat and its owner (final_card: the previous seat's, else the one before, else a lead of the actor's)
  const int first = role_prev(role0);   // the actor's seat
  const uint32_t trick0 = rfl(root.trick0);
  const int owner0 = root.lead0 ? first : root.passes0 ? role_next(first) : role_prev(first);
  // ---- a slot
  uint32_t slot = 0;
  if (lane == 0) slot = atomicAdd((uint32_t*)a.work, 1u);
  slot = rfl(slot);
  bool over = (int64_t)slot >= a.slots;
  uint8_t* const base = a.work + CFR_HEAD_BYTES + (uint64_t)(over ? 0u : slot) * CFR_SLOT_BYTES;
  double* const RA = (double*)(base + CFR_O_RA);
  double* const RB = (double*)(base + CFR_O_RB);
  double* const RC = (double*)(base + CFR_O_RC);
  double* const U = (double*)(base + CFR_O_U);
  uint64_t* const ST = (uint64_t*)base;                 // the build's states: 4 words per node
  uint16_t* const parent = (uint16_t*)(base + CFR_O_PARENT);
  uint16_t* const info = (uint16_t*)(base + CFR_O_INFO);
  uint16_t* const child0 = (uint16_t*)(base + CFR_O_CHILD);
  uint16_t* const next = (uint16_t*)(base + CFR_O_NEXT);
  uint8_t* const act = base + CFR_O_ACT;
  uint8_t* const kind = base + CFR_O_KIND;
  uint64_t* const rec = (uint64_t*)(base + CFR_O_REC);  // off | n << 16 | mover << 24 | head << 32 | tail << 48
  double* const Rg = (double*)(base + CFR_O_R);
  double* const Sg = (double*)(base + CFR_O_SIGMA);
  uint64_t* const itab = (uint64_t*)(base + CFR_O_ITAB);
  uint64_t* const htab = (uint64_t*)(base + CFR_O_HTAB);
  // ---- the root's list: n, the ids
  int n_root = 0;
  if (!over) {
    uint64_t okm; int n0;
    n_root = ply_list(hc0, trick0, hot, lane, stage, svl, okm, n0);
    __builtin_amdgcn_wave_barrier();
    if (n_root < 1 || n_root > DDZ_CFR_MAX_ACTIONS) over = true;
    for (int j = 0; j < DDZ_CFR_MAX_ACTIONS; ++j) {
      if (over || j >= n_root) break;
      uint64_t snib; uint32_t scat, svlv;
      ply_entry(okm, n0, j, trick0, stage, svl, snib, scat, svlv);
      const int id = cfr_action_id(snib, scat, svlv);
      if (id < 0) over = true;
      else if (lane == 0) out_ids[j] = id;
    }
  }
  // ---- the deals
  const int sz0 = first == 0 ? n_me : (rnext == 1 ? n_next : n_prev);   // the lord's cards (role 1)
  const int sz1 = first == 1 ? n_me : (rnext == 2 ? n_next : n_prev);   // down's (role 2)
  uint32_t D = 0;
  if (!over) {
    uint32_t rkw = 0, cw = 0, total = 1;
    int K = 0;
    for (int r = 0; r < 15; ++r) {
      const uint32_t c = (uint32_t)(pool >> (4 * r)) & 15u;
      if (c && K < 6) { rkw |= (uint32_t)r << (4 * K); cw |= c << (4 * K); total *= (c + 1u) * (c + 2u) / 2u; ++K; }
    }
    for (uint32_t b = 0; b < 729u; b += 64u) {
      if (b >= total) break;
      const uint32_t idx = b + (uint32_t)lane;
      uint32_t rem = idx;
      uint64_t h0 = 0, h1 = 0, h2 = 0;
      int s0 = 0, s1 = 0;
      for (int k = 5; k >= 0; --k) {
        if (k >= K) continue;
        const uint32_t c = (cw >> (4 * k)) & 15u, r = (rkw >> (4 * k)) & 15u;
        const uint32_t pk = (c + 1u) * (c + 2u) / 2u;
        uint32_t j = rem % pk, x = 0;
        rem /= pk;
        for (int q = 0; q < 4; ++q) {
          const uint32_t w = c + 1u - x;
          if (j >= w) { j -= w; ++x; }
        }
        h0 += (uint64_t)x << (4 * r);
        h1 += (uint64_t)j << (4 * r);
        h2 += (uint64_t)(c - x - j) << (4 * r);
        s0 += (int)x;
        s1 += (int)j;
      }
      const bool ok = idx < total && s0 == sz0 && s1 == sz1;
      const uint64_t okb = __ballot(ok);
      const uint32_t d = D + (uint32_t)__builtin_popcountll(okb & ((1ull << lane) - 1ull));
      if (ok && d < (uint32_t)DDZ_CFR_MAX_DEALS) {
        uint64_t* s = ST + 4ull * d;
        sst64(s + 0, h0 | ((uint64_t)owner0 << 60));
        sst64(s + 1, h1);
        sst64(s + 2, h2);
        sst64(s + 3, (uint64_t)trick0 | ((uint64_t)d << 40));   // history 0
        sst16(parent + d, CFR_NONE);
        sst8(act + d, 0u);
        sst16(next + d, CFR_NONE);
        dl[3 * d + 0] = (uint16_t)cfr_hand16(h0);
        dl[3 * d + 1] = (uint16_t)cfr_hand16(h1);
        dl[3 * d + 2] = (uint16_t)cfr_hand16(h2);
      }
      D += (uint32_t)__builtin_popcountll(okb);
    }
    if (D < 1 || D > (uint32_t)DDZ_CFR_MAX_DEALS) over = true;
  }
  // ---- the forest
  uint32_t nn = D, ninfo = 0, npairs = 0, nhist = 1, depth = 0;
  if (!over) {
    for (uint32_t i = (uint32_t)lane; i < (1u << CFR_INFO_LOG); i += 64) sst64(itab + i, 0ull);
    for (uint32_t i = (uint32_t)lane; i < (1u << CFR_HIST_LOG); i += 64) sst64(htab + i, 0ull);
    if (lane == 0) level[0] = 0;
    search_fence();
    uint32_t lvl_end = D;
    for (uint32_t i = 0; i < CFR_N; ++i) {
      if (i >= nn || over) break;
      if (i == lvl_end) {
        depth += 1;
        if (depth > (uint32_t)DDZ_CFR_MAX_DEPTH) { over = true; break; }
        if (lane == 0) level[depth] = i;
        lvl_end = nn;
      }
      const uint64_t q0 = rfl64(sld64(ST + 4ull * i)), q1 = rfl64(sld64(ST + 4ull * i + 1));
      const uint64_t q2 = rfl64(sld64(ST + 4ull * i + 2)), q3 = rfl64(sld64(ST + 4ull * i + 3));
      const uint64_t h0 = q0 & 0x0FFFFFFFFFFFFFFFull, h1 = q1, h2 = q2;
      const int owner = (int)(q0 >> 60);
      const uint32_t trick = (uint32_t)q3 & 0xFFFFFFu, hist = (uint32_t)(q3 >> 24) & 0xFFFFu, deal = (uint32_t)(q3 >> 40) & 0x7Fu;
      if (h0 == 0 || h1 == 0 || h2 == 0) {   // a hand is empty: the lord's +1, a farmer's -1
        if (lane == 0) sst8(kind + i, h0 == 0 ? CFR_TERM_LORD : CFR_TERM_FARMER);
        continue;
      }
      const int mover = (int)((uint32_t)first + depth) % 3;
      const uint64_t hand = mover == 0 ? h0 : mover == 1 ? h1 : h2;
      uint64_t okm; int n0;
      const int n = ply_list(hand, trick, hot, lane, stage, svl, okm, n0);
      __builtin_amdgcn_wave_barrier();
      if (n < 1 || n > DDZ_CFR_MAX_ACTIONS || nn + (uint32_t)n > CFR_N) { over = true; break; }
      // the information set: (history, the mover's hand in the deal)
      const uint32_t ikey = (hist << 16) | rfl((uint32_t)dl[3 * deal + mover]);
      bool created;
      const uint32_t I = cfr_find_or_insert(itab, CFR_INFO_LOG, ikey, ninfo, true, lane, created);
      if (I == CFR_NONE) { over = true; break; }
      if (created) {
        if (ninfo >= CFR_I || npairs + (uint32_t)n > CFR_MAX_PAIRS) { over = true; break; }
        if (lane == 0) sst64(rec + I, (uint64_t)npairs | ((uint64_t)n << 16) | ((uint64_t)mover << 24) | ((uint64_t)i << 32) | ((uint64_t)i << 48));
        ninfo += 1;
        npairs += (uint32_t)n;
      } else {
        const uint64_t rc = rfl64(sld64(rec + I));
        const uint32_t tail = (uint32_t)(rc >> 48);
        if (((uint32_t)(rc >> 16) & 0xFFu) != (uint32_t)n || tail >= i) { over = true; break; }   // (cannot happen)
        if (lane == 0) {
          sst16(next + tail, i);
          sst64(rec + I, (rc & 0x0000FFFFFFFFFFFFull) | ((uint64_t)i << 48));
        }
      }
      if (lane == 0) {
        sst16(info + i, I);
        sst16(child0 + i, nn);
        sst8(kind + i, (uint32_t)n);
      }
      for (int j = 0; j < DDZ_CFR_MAX_ACTIONS; ++j) {
        if (j >= n) break;
        uint64_t snib; uint32_t scat, svlv;
        ply_entry(okm, n0, j, trick, stage, svl, snib, scat, svlv);
        const int id = cfr_action_id(snib, scat, svlv);
        if (id < 0) { over = true; break; }
        bool hnew;
        const uint32_t h2id = cfr_find_or_insert(htab, CFR_HIST_LOG, ((hist << 14) | (uint32_t)id) + 1u, nhist, nhist < CFR_MAX_HIST, lane, hnew);
        if (h2id == CFR_NONE) { over = true; break; }
        if (hnew) nhist += 1;
        uint64_t c0 = h0, c1 = h1, c2 = h2;
        uint32_t ctrick = trick;
        int cowner = owner;
        if (snib) {
          if (mover == 0) c0 -= snib; else if (mover == 1) c1 -= snib; else c2 -= snib;
          ctrick = scat | (svlv << 8);
          cowner = mover;
        } else if ((mover == 2 ? 0 : mover + 1) == owner) {
          ctrick = mk_info(EMPTY, 0, 1);   // both others passed: the owner leads
        }
        const uint32_t c = nn + (uint32_t)j;
        if (lane == 0) {
          uint64_t* s = ST + 4ull * c;
          sst64(s + 0, c0 | ((uint64_t)cowner << 60));
          sst64(s + 1, c1);
          sst64(s + 2, c2);
          sst64(s + 3, (uint64_t)(ctrick & 0xFFFFFFu) | ((uint64_t)h2id << 24) | ((uint64_t)deal << 40));
          sst16(parent + c, i);
          sst8(act + c, (uint32_t)j);
          sst16(next + c, CFR_NONE);
        }
      }
      nn += (uint32_t)n;
      search_fence();
    }
  }
  if (over) {   // no slot, or a capacity: nothing was stored out of bounds
    if (lane < DDZ_CFR_STRIDE) out_ids[lane] = -1;
    if (lane == 0) { a.n[t] = -2; atomicOr(a.status, DDZ_ST_CFR_CAPACITY); }
    return;
  }
  const uint32_t nlev = depth + 1;
  if (lane == 0) level[nlev] = nn;
  search_fence();
  // ---- sigma = 1 / n, R = 0; the roots' reaches
  for (uint32_t b = 0; b < CFR_I; b += 64) {
    const uint32_t I = b + (uint32_t)lane;
    if (b >= ninfo) break;
    if (I < ninfo) {
      const uint64_t rc = sld64(rec + I);
      const uint32_t off = (uint32_t)rc & 0xFFFFu, n = (uint32_t)(rc >> 16) & 0xFFu;
      const double s = 1.0 / (double)n;
      for (uint32_t j = 0; j < (uint32_t)DDZ_CFR_MAX_ACTIONS; ++j)
        if (j < n) { sstf(Sg + off + j, s); sstf(Rg + off + j, 0.0); }
    }
  }
  search_fence();   // (the states of the build are dead: their bytes become reaches and values)
  for (uint32_t b = 0; b < (uint32_t)DDZ_CFR_MAX_DEALS + 64u; b += 64) {
    const uint32_t i = b + (uint32_t)lane;
    if (b >= D) break;
    if (i < D) { sstf(RA + i, 1.0); sstf(RB + i, 1.0); sstf(RC + i, 1.0); }
  }
  search_fence();
  double value = 0.0;
  for (uint32_t it = 0; it < (uint32_t)DDZ_CFR_MAX_ITERATIONS; ++it) {
    if (it >= a.iterations) break;
    // the reaches, downwards: the parent's, the parent's mover's multiplied by sigma of the action taken
    for (uint32_t d = 1; d <= (uint32_t)DDZ_CFR_MAX_DEPTH; ++d) {
      if (d >= nlev) break;
      const uint32_t lo = rfl(level[d]), hi = rfl(level[d + 1]);
      const int pm = (int)((uint32_t)first + d - 1u) % 3;
      for (uint32_t b = lo; b < hi; b += 64) {
        const uint32_t i = b + (uint32_t)lane;
        if (i < hi) {
          const uint32_t p = sld16(parent + i);
          const uint32_t off = (uint32_t)sld64(rec + sld16(info + p)) & 0xFFFFu;
          const double s = sldf(Sg + off + sld8(act + i));
          double ra = sldf(RA + p), rb = sldf(RB + p), rc = sldf(RC + p);
          if (pm == 0) ra = ra * s; else if (pm == 1) rb = rb * s; else rc = rc * s;
          sstf(RA + i, ra); sstf(RB + i, rb); sstf(RC + i, rc);
        }
      }
      search_fence();
    }
    // the values, upwards: value = ((0 + s0 * u0) + s1 * u1) + ...
    for (uint32_t dd = 0; dd <= (uint32_t)DDZ_CFR_MAX_DEPTH; ++dd) {
      if (dd >= nlev) break;
      const uint32_t d = nlev - 1u - dd;
      const uint32_t lo = rfl(level[d]), hi = rfl(level[d + 1]);
      for (uint32_t b = lo; b < hi; b += 64) {
        const uint32_t i = b + (uint32_t)lane;
        if (i < hi) {
          const uint32_t k = sld8(kind + i);
          double v = 0.0;
          if (k & (CFR_TERM_LORD | CFR_TERM_FARMER)) v = (k & CFR_TERM_LORD) ? 1.0 : -1.0;
          else {
            const uint32_t off = (uint32_t)sld64(rec + sld16(info + i)) & 0xFFFFu, c0 = sld16(child0 + i);
            for (uint32_t j = 0; j < (uint32_t)DDZ_CFR_MAX_ACTIONS; ++j)
              if (j < k) v = v + cfr_rounded(sldf(Sg + off + j) * sldf(U + c0 + j));
          }
          sstf(U + i, v);
        }
      }
      search_fence();
    }
    // the regrets: a lane per information set, its members in ascending node index; then sigma
    for (uint32_t b = 0; b < CFR_I; b += 64) {
      if (b >= ninfo) break;
      const uint32_t I = b + (uint32_t)lane;
      if (I < ninfo) {
        const uint64_t rc_ = sld64(rec + I);
        const uint32_t off = (uint32_t)rc_ & 0xFFFFu, n = (uint32_t)(rc_ >> 16) & 0xFFu, mover = (uint32_t)(rc_ >> 24) & 3u;
        uint32_t m = (uint32_t)(rc_ >> 32) & 0xFFFFu;
        for (int g = 0; g < DDZ_CFR_MAX_DEALS; ++g) {
          if (m == CFR_NONE) break;
          const double ra = sldf(RA + m), rb = sldf(RB + m), rc = sldf(RC + m);
          const double cr = mover == 0 ? rb * rc : mover == 1 ? ra * rc : ra * rb;
          const double um = sldf(U + m);
          const uint32_t c0 = sld16(child0 + m);
          for (uint32_t j = 0; j < (uint32_t)DDZ_CFR_MAX_ACTIONS; ++j) {
            if (j < n) {
              const double diff = sldf(U + c0 + j) - um;
              const double reg = cfr_rounded(cr * diff);
              const double r0 = sldf(Rg + off + j);
              sstf(Rg + off + j, mover == 0 ? r0 + reg : r0 - reg);
            }
          }
          m = sld16(next + m);
        }
        double S = 0.0;
        for (uint32_t j = 0; j < (uint32_t)DDZ_CFR_MAX_ACTIONS; ++j) {
          if (j < n) {
            const double r = sldf(Rg + off + j);
            if (r > 0.0) S = S + r;
          }
        }
        const double uni = 1.0 / (double)n;
        for (uint32_t j = 0; j < (uint32_t)DDZ_CFR_MAX_ACTIONS; ++j) {
          if (j < n) {
            const double r = sldf(Rg + off + j);
            sstf(Sg + off + j, S > 0.0 ? (r > 0.0 ? r : 0.0) / S : uni);
          }
        }
      }
    }
    // value_t = (1 / D) * (u_root(0) + u_root(1) + ...)
    double tot = 0.0;
    for (uint32_t d = 0; d < (uint32_t)DDZ_CFR_MAX_DEALS; ++d) {
      if (d >= D) break;
      tot = tot + sldf(U + d);
    }
    value = (1.0 / (double)D) * tot;
    search_fence();
  }
  // ---- the row of (the actor, its actual hand, the empty history)
  bool dummy;
  const uint32_t I0 = cfr_find_or_insert(itab, CFR_INFO_LOG, cfr_hand16(hc0), 0u, false, lane, dummy);
  uint32_t off0 = 0, nI0 = 0;
  if (I0 != CFR_NONE) {
    const uint64_t rc = rfl64(sld64(rec + I0));
    off0 = (uint32_t)rc & 0xFFFFu;
    nI0 = (uint32_t)(rc >> 16) & 0xFFu;
  }
  if (I0 == CFR_NONE || nI0 != (uint32_t)n_root) {   // (cannot happen: the actual hand is the actor's hand of some deal)
    if (lane < DDZ_CFR_STRIDE) out_ids[lane] = -1;
    if (lane == 0) { a.n[t] = -2; atomicOr(a.status, DDZ_ST_CFR_CAPACITY); }
    return;
  }
  if (lane < n_root) out_sigma[lane] = sldf(Sg + off0 + (uint32_t)lane);
  if (lane == 0) {
    a.n[t] = n_root;
    a.value[t] = value;
    if (a.totals) {
      atomicAdd(a.totals + 0, (unsigned long long)D);
      atomicAdd(a.totals + 1, (unsigned long long)nn);
      atomicAdd(a.totals + 2, (unsigned long long)ninfo);
      atomicAdd(a.totals + 3, (unsigned long long)npairs);
    }
  }
}

// ddz_cfr_choose: one lane per table.  greedy: the first maximum of sigma; else u = x * 2^-32 with x = the first word of
// rng_draw(gid, 0, RNG_CFR_CHOOSE, 0, key), the first j with u below the running sum of sigma in list
// order, falling back to the last j with sigma_j > 0.  -1 where n <= 0.
__global__ __launch_bounds__(BLOCK) void k_cfr_choose(const int32_t* __restrict__ n, const int32_t* __restrict__ ids,
                                                      const double* __restrict__ sigma, uint32_t k0, uint32_t k1, uint64_t gid_base,
                                                      int greedy, int32_t* __restrict__ choice, int64_t T) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= T) return;
  int k = n[t];
  if (k > DDZ_CFR_STRIDE) k = DDZ_CFR_STRIDE;
  if (k <= 0) { choice[t] = -1; return; }
  const double* s = sigma + t * DDZ_CFR_STRIDE;
  int pick = -1;
  if (greedy) {
    double best = 0.0;
    for (int j = 0; j < k; ++j)
      if (pick < 0 || s[j] > best) { best = s[j]; pick = j; }
  } else {
    const uint64_t gid = gid_base + (uint64_t)t;
    const uint32_t x = rng_draw(gid, 0u, RNG_CFR_CHOOSE, 0u, k0, k1).x;
    const double u = (double)x * (1.0 / 4294967296.0);
    double acc = 0.0;
    int last = k - 1;
    for (int j = 0; j < k; ++j) {
      acc = acc + s[j];
      if (s[j] > 0.0) last = j;
      if (pick < 0 && u < acc) pick = j;
    }
    if (pick < 0) pick = last;
  }
  choice[t] = ids[t * DDZ_CFR_STRIDE + pick];
}
