// ddz_search.h -- k_search / k_search_choose: UCT tree search around the playouts ("search spec v1 (UCT)"; the
// reference's MCTS player: server/mcts/interface.py:37-43 with tree_policy / get_bestchild.py / tree.py:33-51 / backup.py).
// Included by ddz_engine.hip behind ddz_playout.h, inside its anonymous namespace: k_rollout and k_playout are not touched, the
// ply below is k_playout's restated on the same device functions (the rank-mask tests, round_pre / round_src / round_entry,
// plan_scan_t<EM_STAGE> into the wave's LDS list, the packed apply, the 64-draw Philox refill, redeal_wave).
//
// One wavefront per WORK ITEM (table t, tree c).  The wave decodes the root once into wave-uniform values (as k_playout), then
// runs `budget` iterations of {descent, expansion, playout, backup} on its own tree.  The descent RE-APPLIES stored moves from
// the root: a node stores the move that made it (the 60-bit nibble word, the category and the value byte: a staging-list
// entry), so only the node being expanded enumerates a list, and the new child's n falls out of the first ply of its playout.
//
// WORKSPACE.  The tree lives in global memory handed in by the caller, search_tree_bytes(budget) per (table, tree), a function
// of the budget alone:
//   nodes  [budget + 1] x 24 bytes: move u64 | V u32 | W u32 | meta u32 | children created u32
//          meta = value/len of the move (16 bits) | n << 16 (10 bits) | terminal << 26 | winner << 27 (2 bits)
//   table  [H] x 8 bytes, H = the power of two >= 2 * (budget + 1): open addressing with linear probing, entry =
//          (parent * 512 + list index + 1) << 32 | child, 0 = empty; slot of a key = (key * 2654435761) >> (32 - log2 H).
// One iteration creates at most one node, so budget + 1 nodes and budget entries are all there can be: the table is never more
// than half full and there is no overflow mode.  The wave zeroes its own table before the first iteration.
//
// LOOPS.  Every loop is counted: iterations by budget, the descent by DDZ_SEARCH_MAX_DEPTH, a probe by H, the rounds over a
// list by n <= STAGE_CAP, the playout by DDZ_PLAYOUT_MAX_PLIES.  A wave waits for no other wave.
//
// MEMORY ORDERING.  A tree is written and read by ONE wavefront: records written by one lane (lane 0 creates nodes and table
// entries, lane l backs up the l-th node of the path) are read by other lanes of the same wave in later iterations.  What orders
// them is __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront") (with a wave barrier) at the end of every iteration and behind
// the zeroing -- as redeal_wave orders its LDS keys.  Wavefront scope is enough because the vector memory instructions of one
// wavefront are issued in order through the one vector L1 of its CU, which cannot tell the lanes of an instruction apart: a
// load behind a store of the same wave sees it exactly as a lane sees its own store.  No other wave, on this CU or another,
// ever reads the tree, so nothing has to become visible at workgroup or agent scope before the kernel ends.  Every access to
// the tree is a relaxed wavefront-scope atomic load / store: these are vector instructions, never scalar-cache loads (the
// scalar cache is not coherent with vector stores).  The root statistics leave through 32-bit atomicAdd, the totals through 64-bit.
struct SearchArgs {
  const uint8_t* state;
  int64_t T;
  uint32_t k0, k1;          // Philox key: (seed_lo ^ salt, seed_hi)
  uint64_t gid_base;
  uint32_t budget, trees, mode;
  float c;
  int64_t stride;           // visits / wins are [T][stride]
  int32_t* visits;
  int32_t* wins;
  unsigned long long* totals;  // {moves applied, iterations run, iterations scored unfinished, nodes created} or null
  int32_t* status;
  uint32_t roles;           // hidden form: bit r = tables whose actor is role r take part
  uint8_t* work;
  uint64_t tree_bytes;
  uint32_t hash_log;
  const float* ln;          // LN[N] = (float)log((double)N), N <= DDZ_SEARCH_MAX_BUDGET
};

constexpr int SEARCH_WAVES = 12;  // 79 KB of LDS per block: two blocks per CU = 6 waves per SIMD (as k_playout)
constexpr int SEARCH_PATH = DDZ_SEARCH_MAX_DEPTH + 8;   // nodes of a path: the root and at most DDZ_SEARCH_MAX_DEPTH below it
constexpr uint32_t SEARCH_NONE = 0xFFFFFFFFu;
constexpr uint32_t NODE_BYTES = 24;

inline uint32_t search_hash_log(int64_t budget) {
  uint32_t l = 1;
  while ((1ll << l) < 2 * (budget + 1)) ++l;
  return l;
}
inline uint64_t search_nodes_bytes(int64_t budget) { return ((uint64_t)(budget + 1) * NODE_BYTES + 15) & ~15ull; }
inline uint64_t search_tree_bytes(int64_t budget) { return search_nodes_bytes(budget) + (8ull << search_hash_log(budget)); }

__device__ float g_search_ln[DDZ_SEARCH_MAX_BUDGET + 1];   // filled from libm with the record table (build_table_locked)

__device__ __forceinline__ uint64_t sld64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ uint32_t sld32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void sst64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void sst32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void search_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the child of (parent, list index j), SEARCH_NONE where none was created.  Per lane; at most H probes.
__device__ __forceinline__ uint32_t search_find(const uint64_t* tab, uint32_t hlog, uint32_t key) {
  const uint32_t hmask = (1u << hlog) - 1u;
  uint32_t h = (key * 2654435761u) >> (32u - hlog);
  for (uint32_t p = 0; p <= hmask; ++p) {
    const uint64_t e = sld64(tab + h);
    if ((uint32_t)(e >> 32) == key) return (uint32_t)e;
    if (e == 0) return SEARCH_NONE;
    h = (h + 1u) & hmask;
  }
  return SEARCH_NONE;
}
__device__ __forceinline__ void search_insert(uint64_t* tab, uint32_t hlog, uint32_t key, uint32_t child) {
  const uint32_t hmask = (1u << hlog) - 1u;
  uint32_t h = (key * 2654435761u) >> (32u - hlog);
  for (uint32_t p = 0; p <= hmask; ++p) {
    if (sld64(tab + h) == 0) {
      sst64(tab + h, ((uint64_t)key << 32) | child);
      return;
    }
    h = (h + 1u) & hmask;
  }
}

// value = W / V + c * sqrt((2 * LN[N]) / V): five correctly rounded fp32 operations, nothing fused (get_bestchild.py:9-18)
__device__ __forceinline__ float search_value(uint32_t w, uint32_t v, float two_ln, float c) {
#pragma clang fp contract(off)
  const float fv = (float)v;
  const float mean = (float)w / fv;
  const float q = two_ln / fv;
  const float r = __builtin_sqrtf(q);
  const float bonus = c * r;
  return mean + bonus;
}

// the legal list of the state (hand, info) as k_playout's ply sees it: the closed-form round's legal lanes as a mask, the
// planner's tail staged into the wave's LDS list; returns the list's size (n0 = the round's share)
template <typename HT>
__device__ __forceinline__ int search_list(uint64_t hand, uint32_t info, const HT& hot, int lane, uint64_t* stage, uint16_t* svl,
                                           uint64_t& okm_out, int& n0_out) {
  const int lc0 = (int)(info & 0xFF);
  const bool lead = lc0 == EMPTY;
  const int cntr = lane < 15 ? (int)((hand >> (4 * (lane & 15))) & 15) : 0;
  const uint32_t b1 = (uint32_t)__ballot(cntr >= 1), b4 = (uint32_t)__ballot(cntr >= 4);
  uint64_t okm = 0;
  bool tail = false;
  if ((b1 & M15) == 0) {
    // an empty hand on a running state (outside the domain): the empty list
  } else if (!lead && lc0 <= TRIPLE) {
    const int lv0 = (int)((info >> 8) & 0xFF);
    const uint32_t mlc = (uint32_t)__ballot(cntr >= lc0) & (lc0 == SINGLE ? M15 : M13);
    const bool rocket = (b1 & JOKERS) == JOKERS;
    okm = 1u | ((mlc & gt_mask(lv0)) << 1) | ((b4 & M13) << 16) | (rocket ? 1u << 29 : 0u);
  } else {
    const uint32_t m1 = b1 & M15, m2 = (uint32_t)__ballot(cntr >= 2) & M13;
    const uint32_t m3 = (uint32_t)__ballot(cntr >= 3) & M13, m4 = b4 & M13;
    const bool jokers = (m1 & JOKERS) == JOKERS;
    if (lead) {
      tail = m3 != 0 || run_starts(m1 & M12, 5) != 0 || run_starts(m2 & M12, 3) != 0;
      okm = (uint64_t)m1 | (uint64_t)m2 << 15 | (uint64_t)m3 << 28 | (uint64_t)m4 << 41 | (jokers && !tail ? 1ull << 54 : 0ull);
    } else {
      const int lv0 = (int)((info >> 8) & 0xFF), ll0 = (int)((info >> 16) & 0xFF);
      const uint32_t ab = gt_mask(lv0);
      uint32_t cand = 0, bombs = m4, may = 0;
      bool rocket = jokers;
      if (lc0 == QUADRIC) { cand = m4 & ab; bombs = 0; }
      else if (lc0 == BIGBANG) { bombs = 0; rocket = false; }
      else if (lc0 == THREE_ONE || lc0 == THREE_TWO) may = m3 & ab;
      else if (lc0 == SINGLE_LINE) may = run_starts(m1 & M12, ll0) & ab;
      else if (lc0 == DOUBLE_LINE) may = run_starts(m2 & M12, ll0) & ab;
      else if (lc0 == TRIPLE_LINE || lc0 == THREE_ONE_LINE || lc0 == THREE_TWO_LINE) may = run_starts(m3 & M12, ll0) & ab;
      else if (lc0 == FOUR_TAKE_ONE || lc0 == FOUR_TAKE_TWO) may = m4 & ab;
      tail = may != 0;
      okm = 1u | (cand << 1) | (bombs << 16) | (rocket && !tail ? 1u << 29 : 0u);
    }
  }
  const int n0 = __builtin_popcountll(okm);
  int n = n0;
  if (tail) {
    const Out o{nullptr, nullptr, 0, 0, stage, svl, nullptr};
    Pick pk{-1, 0, 0, 0, 0};
    const Follow f = follow_of(info);
    const int n1 = lead ? plan_scan_t<EM_STAGE, false, true, HT, false>(hand, f, hot, lane, o, pk)
                        : plan_scan_t<EM_STAGE, false, false, HT, false>(hand, f, hot, lane, o, pk);
    __builtin_amdgcn_wave_barrier();
    n = (int)rfl((uint32_t)(n0 + n1));
  }
  okm_out = okm;
  n0_out = n0;
  return n;
}

// entry idx < n of the list search_list left: the nibble word, the category and the value/len byte pair (wave-uniform)
__device__ __forceinline__ void search_entry(uint64_t okm, int n0, int idx, uint32_t info, const uint64_t* stage, const uint16_t* svl,
                                             uint64_t& snib, uint32_t& scat, uint32_t& svlv) {
  const int lc0 = (int)(info & 0xFF);
  const bool lead = lc0 == EMPTY;
  uint32_t ncards = 0;
  snib = 0; scat = 0; svlv = 0;
  if (idx < n0) {
    if (lead) round_entry<true>(round_src<true>(okm, round_pre(okm), idx), 0u, snib, scat, svlv, ncards);
    else round_entry<false>(round_src<false>((uint32_t)okm, round_pre((uint32_t)okm), idx), (uint32_t)lc0, snib, scat, svlv, ncards);
  } else {
    const uint64_t e = stage[idx - n0];
    const uint64_t anib = e & 0x0FFFFFFFFFFFFFFFull;
    snib = (uint64_t)rfl((uint32_t)anib) | ((uint64_t)rfl((uint32_t)(anib >> 32)) << 32);
    scat = rfl((uint32_t)(e >> 60));
    svlv = rfl((uint32_t)svl[idx - n0]);
  }
  (void)ncards;
}

template <bool HIDDEN>
__global__ __launch_bounds__(SEARCH_WAVES * 64, 6) void k_search(SearchArgs a) {
  __shared__ HotTabT<false> hot;
  __shared__ uint64_t s_stage[SEARCH_WAVES][STAGE_CAP];
  __shared__ uint16_t s_svl[SEARCH_WAVES][STAGE_CAP];
  __shared__ uint16_t s_path[SEARCH_WAVES][SEARCH_PATH];
  const int lane = threadIdx.x & 63;
  const int wv = (int)rfl(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * SEARCH_WAVES + wv;
  const int64_t t = item / a.trees;
  const uint32_t tree = (uint32_t)(item - t * a.trees);
  uint4 R = make_uint4(0, 0, 0, 0);
  if (t < a.T && lane < DDZ_NFIELDS) R = ((const uint4*)(a.state + t * STATE_ROW_BYTES))[lane];
  hot_fill<SEARCH_WAVES * 64>(hot);
  __syncthreads();   // the block's only barrier: a wave may leave behind it
  if (t >= a.T) return;
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  uint16_t* path = s_path[wv];
  // the root, decoded once (as k_playout decodes it)
  const uint64_t P = pack_row(R);
  const uint32_t aux = R.w >> 24;
  const uint32_t mx = rl(R.x, DDZ_F_META), my = rl(R.y, DDZ_F_META);
  int role0 = mx & 0xFF;
  if (role0 > 2) role0 = 0;
  if (!(((my >> 16) & 0xFF) && !((mx >> 8) & 0xFF))) return;  // not dealt, or done: nothing runs
  const uint32_t ply0 = my & 0xFFFF;
  const uint64_t hc0 = rl64(P, DDZ_F_HAND0 + role0);
  uint64_t hn0 = 0, hp0 = 0;
  if constexpr (!HIDDEN) {
    hn0 = rl64(P, DDZ_F_HAND0 + (role0 == 2 ? 0 : role0 + 1));
    hp0 = rl64(P, DDZ_F_HAND0 + (role0 == 0 ? 2 : role0 - 1));
  }
  uint32_t trick0 = mk_info(EMPTY, 0, 1);
  int passes0 = 0;
  {
    const int rm1 = role0 == 0 ? 2 : role0 - 1, rp1 = role0 == 2 ? 0 : role0 + 1;
    const uint64_t n1 = rl64(P, DDZ_F_RECENT0 + rm1), n2 = rl64(P, DDZ_F_RECENT0 + rp1);
    if (n1) trick0 = info_of_row(n1, (int)rl(aux, DDZ_F_RECENT0 + rm1));
    else if (n2) { trick0 = info_of_row(n2, (int)rl(aux, DDZ_F_RECENT0 + rp1)); passes0 = 1; }
  }
  const uint64_t gid = a.gid_base + (uint64_t)t;
  if constexpr (HIDDEN) {   // tree c plays on world k = c of playout spec v2: the same pool, the same domain, the same deal
    if (!((a.roles >> role0) & 1u)) return;
    const uint64_t taken = rl64(P, DDZ_F_TAKEN);
    const int n_next = (int)rl(aux, DDZ_F_HAND0 + (role0 == 2 ? 0 : role0 + 1));
    const int n_prev = (int)rl(aux, DDZ_F_HAND0 + (role0 == 0 ? 2 : role0 - 1));
    const int sh = 4 * (lane & 15);
    const int deck = lane < 13 ? 4 : lane < 15 ? 1 : 0;
    const bool over = (int)((hc0 >> sh) & 15) + (int)((taken >> sh) & 15) > deck;
    const bool bad = __ballot(lane < 15 && over) != 0ull;
    const uint64_t unseen = DECK_NIB - hc0 - taken;
    if (bad || n_next < 1 || n_prev < 1 || nib_sum(unseen) != n_next + n_prev) {
      if (lane == 0 && tree == 0) atomicOr(a.status, 64);
      return;
    }
    const int rank = lane < 52 ? lane >> 2 : lane - 39;
    const int cnt = (int)((unseen >> (4 * (rank & 15))) & 15);
    const bool pool = lane < 52 ? (lane & 3) < cnt : (lane < 54 && cnt == 1);
    redeal_wave(gid, tree, a.k0, a.k1, lane, pool, n_next, stage, hn0, hp0);
  }
  const bool root_lord = role0 == 1;
  const uint32_t hlog = a.hash_log;
  uint8_t* const base = a.work + (uint64_t)item * a.tree_bytes;
  uint8_t* const nodes = base;
  uint64_t* const tab = (uint64_t*)(base + (((uint64_t)(a.budget + 1) * NODE_BYTES + 15) & ~15ull));
  // the root's list: its size is the root's n; an empty list (or one the slab cannot hold) runs nothing
  int n_root;
  {
    uint64_t okm; int n0;
    const uint32_t info = rfl((passes0 >= 2) ? mk_info(EMPTY, 0, 1) : trick0);
    n_root = search_list(hc0, info, hot, lane, stage, svl, okm, n0);
    __builtin_amdgcn_wave_barrier();
    if (n_root > STAGE_CAP || n_root > a.stride) {
      if (lane == 0) atomicOr(a.status, 2);
      return;
    }
    if (n_root <= 0) return;
  }
  for (uint32_t i = (uint32_t)lane; i < (1u << hlog); i += 64) sst64(tab + i, 0ull);
  if (lane == 0) {   // node 0: no move, nothing visited
    sst64((uint64_t*)nodes, 0ull);
    sst64((uint64_t*)(nodes + 8), 0ull);
    sst32((uint32_t*)(nodes + 16), (uint32_t)n_root << 16);
    sst32((uint32_t*)(nodes + 20), 0u);
  }
  search_fence();
  uint32_t nnodes = 1;
  unsigned long long s_moves = 0;
  uint32_t s_unfinished = 0;
  for (uint32_t it = 0; it < a.budget; ++it) {
    uint64_t hc = hc0, hn = hn0, hp = hp0;
    uint32_t trick = trick0, ply = ply0;
    int passes = passes0, role = role0;
    uint32_t node = 0;
    int depth = 0;          // path[0 .. depth] are the nodes backed up
    int winner = -1;
    uint32_t made = SEARCH_NONE;   // the node this iteration creates: its record is written whole behind the playout
    uint64_t made_move = 0;
    uint32_t made_meta = 0;
    if (lane == 0) path[0] = 0;
    for (int d = 0; d <= DDZ_SEARCH_MAX_DEPTH; ++d) {
      const uint8_t* nr = nodes + (uint64_t)node * NODE_BYTES;
      const uint32_t meta = rfl(sld32((const uint32_t*)(nr + 16)));
      if ((meta >> 26) & 1u) {   // the move into this node emptied a hand: scored without a playout
        winner = (int)((meta >> 27) & 3u);
        break;
      }
      const int n = (int)((meta >> 16) & 0x3FFu);
      if (n <= 0 || d == DDZ_SEARCH_MAX_DEPTH) break;   // outside the domain: reward 0, unfinished
      const uint32_t nchild = rfl(sld32((const uint32_t*)(nr + 20)));
      const uint32_t info = rfl((passes >= 2) ? mk_info(EMPTY, 0, 1) : trick);
      if ((int)nchild < n) {
        // ---- expansion: the (draw_e * u) >> 32-th untried list index, ascending
        uint64_t okm; int n0;
        const int nn = search_list(hc, info, hot, lane, stage, svl, okm, n0);
        if (nn != n) break;   // (cannot happen: the state of a node is a function of its path)
        const uint32_t u = (uint32_t)n - nchild;
        const uint32_t de = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), (tree << 16) | it, 6u << 16), a.k0, a.k1).x;
        uint32_t r = rfl(__umulhi(de, u));
        int idx = -1;
        if (nchild == 0) idx = (int)r;
        else {
          for (int b = 0; b < n; b += 64) {
            const int j = b + lane;
            bool untried = false;
            if (j < n) untried = search_find(tab, hlog, node * 512u + (uint32_t)j + 1u) == SEARCH_NONE;
            const uint64_t um = __ballot(untried);
            const uint32_t cnt = (uint32_t)__builtin_popcountll(um);
            if (r < cnt) {
              const uint64_t below = um & ((1ull << lane) - 1ull);
              const uint64_t hit = __ballot(untried && (uint32_t)__builtin_popcountll(below) == r);
              idx = b + (int)__builtin_ctzll(hit);
              break;
            }
            r -= cnt;
          }
        }
        if (idx < 0 || idx >= n) break;   // (cannot happen: u untried indices exist)
        uint64_t snib; uint32_t scat, svlv;
        search_entry(okm, n0, idx, info, stage, svl, snib, scat, svlv);
        made = nnodes++;
        made_move = snib | ((uint64_t)scat << 60);
        made_meta = svlv & 0xFFFFu;
        if (lane == 0) {
          search_insert(tab, hlog, node * 512u + (uint32_t)idx + 1u, made);
          sst32((uint32_t*)(nodes + (uint64_t)node * NODE_BYTES + 20), nchild + 1u);
        }
        const uint64_t hnew = hc - snib;
        if (snib) { trick = scat | (svlv << 8); passes = 0; } else { passes += 1; }
        s_moves += 1;
        ply += 1;
        __builtin_amdgcn_wave_barrier();
        if (rfl((uint32_t)hnew | (uint32_t)(hnew >> 32)) == 0u) {
          winner = role;
          made_meta |= (1u << 26) | ((uint32_t)role << 27);
          break;
        }
        role = role == 2 ? 0 : role + 1;
        hc = hn; hn = hp; hp = hnew;
        // ---- playout from the new child: k_playout's ply, draws of domain 7 keyed by (gid, tree, iteration, ply)
        uint32_t draws = 0, dnext = 64;
        for (int s = 0; s < DDZ_PLAYOUT_MAX_PLIES; ++s) {
          uint32_t dn = rfl(dnext);
          if (dn >= 64u) {
            dn = 0;
            dnext = 0;
            draws = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), (tree << 16) | it,
                                             (7u << 16) | ((ply + (uint32_t)lane) & 0xFFFFu)), a.k0, a.k1).x;
          }
          const uint32_t draw = rl(draws, (int)dn);
          const uint64_t hand = hc;
          const uint32_t pinfo = rfl((passes >= 2) ? mk_info(EMPTY, 0, 1) : trick);
          uint64_t pokm; int pn0;
          int pn = search_list(hand, pinfo, hot, lane, stage, svl, pokm, pn0);
          if (pn > STAGE_CAP) {
            if (lane == 0) atomicOr(a.status, 2);
            pn = 0;
          }
          if (s == 0) made_meta |= (uint32_t)pn << 16;   // the child's n
          if (pn <= 0) break;   // stopped unfinished
          const int pidx = (int)rfl(__umulhi(draw, (uint32_t)pn));
          uint64_t pnib; uint32_t pcat, pvl;
          search_entry(pokm, pn0, pidx, pinfo, stage, svl, pnib, pcat, pvl);
          const uint64_t hnew2 = hand - pnib;
          if (pnib) { trick = pcat | (pvl << 8); passes = 0; } else { passes += 1; }
          s_moves += 1;
          ply += 1;
          dnext += 1;
          __builtin_amdgcn_wave_barrier();
          if (rfl((uint32_t)hnew2 | (uint32_t)(hnew2 >> 32)) == 0u) {
            winner = role;
            break;
          }
          role = role == 2 ? 0 : role + 1;
          hc = hn; hn = hp; hp = hnew2;
        }
        break;
      }
      // ---- selection at a fully expanded node (get_bestchild.py:20-32)
      const uint32_t N = rfl(sld32((const uint32_t*)(nr + 8)));
      const float two_ln = 2.0f * a.ln[N <= (uint32_t)DDZ_SEARCH_MAX_BUDGET ? N : (uint32_t)DDZ_SEARCH_MAX_BUDGET];
      const bool own = a.mode == (uint32_t)DDZ_SEARCH_SIDES ? ((role == 1) == root_lord) : (role == role0);
      const bool take_max = own || a.mode == (uint32_t)DDZ_SEARCH_SIDES;
      uint32_t best = 0, at = SEARCH_NONE, bchild = SEARCH_NONE;
      for (int b = 0; b < n; b += 64) {
        const int j = b + lane;
        if (j < n) {
          const uint32_t ch = search_find(tab, hlog, node * 512u + (uint32_t)j + 1u);
          if (ch != SEARCH_NONE && ch < nnodes) {
            const uint64_t vw = sld64((const uint64_t*)(nodes + (uint64_t)ch * NODE_BYTES + 8));
            const uint32_t V = (uint32_t)vw, W = (uint32_t)(vw >> 32);
            if (V > 0) {
              // (values are non-negative floats: their bit patterns order as they do)
              const uint32_t bits = __float_as_uint(search_value(own ? W : (a.mode == (uint32_t)DDZ_SEARCH_SIDES ? V - W : W), V, two_ln, a.c));
              if (at == SEARCH_NONE || (take_max ? bits > best : bits < best)) { best = bits; at = (uint32_t)j; bchild = ch; }
            }
          }
        }
      }
      uint32_t m;
      if (take_max) m = (uint32_t)wave_max_i32(at == SEARCH_NONE ? (int)0x80000000 : (int)best);
      else m = wave_min_u32(at == SEARCH_NONE ? 0xFFFFFFFFu : best);
      const uint32_t first = wave_min_u32((at != SEARCH_NONE && best == m) ? at : SEARCH_NONE);   // ties: the lowest index
      if (first == SEARCH_NONE) break;   // (cannot happen: a fully expanded node has n visited children)
      const uint32_t child = rl(bchild, (int)(first & 63u));
      const uint8_t* cr = nodes + (uint64_t)child * NODE_BYTES;
      const uint64_t mv = sld64((const uint64_t*)cr);
      const uint32_t cmeta = sld32((const uint32_t*)(cr + 16));
      const uint64_t anib = mv & 0x0FFFFFFFFFFFFFFFull;
      const uint64_t snib = (uint64_t)rfl((uint32_t)anib) | ((uint64_t)rfl((uint32_t)(anib >> 32)) << 32);
      const uint32_t scat = rfl((uint32_t)(mv >> 60)), svlv = rfl(cmeta & 0xFFFFu);
      const uint64_t hnew = hc - snib;
      if (snib) { trick = scat | (svlv << 8); passes = 0; } else { passes += 1; }
      s_moves += 1;
      ply += 1;
      role = role == 2 ? 0 : role + 1;
      hc = hn; hn = hp; hp = hnew;
      node = child;
      depth += 1;
      if (lane == 0) path[depth] = (uint16_t)child;
    }
    // ---- backup: V += 1, W += score on every node of the path; the new node's record is written whole
    const uint32_t score = (winner >= 0 && ((winner == 1) == root_lord)) ? 1u : 0u;
    if (winner < 0) s_unfinished += 1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the path is written
    for (int b = 0; b <= depth; b += 64) {
      const int l = b + lane;
      if (l <= depth) {
        uint64_t* p = (uint64_t*)(nodes + (uint64_t)path[l] * NODE_BYTES + 8);
        const uint64_t vw = sld64(p);
        sst64(p, vw + 1ull + ((uint64_t)score << 32));
      }
    }
    if (made != SEARCH_NONE && lane == 0) {
      uint8_t* q = nodes + (uint64_t)made * NODE_BYTES;
      sst64((uint64_t*)q, made_move);
      sst64((uint64_t*)(q + 8), 1ull | ((uint64_t)score << 32));
      sst32((uint32_t*)(q + 16), made_meta);
      sst32((uint32_t*)(q + 20), 0u);
    }
    search_fence();
  }
  // ---- the root's children leave: visits / wins += V / W at their list index
  for (int b = 0; b < n_root; b += 64) {
    const int j = b + lane;
    if (j < n_root) {
      const uint32_t ch = search_find(tab, hlog, (uint32_t)j + 1u);
      if (ch != SEARCH_NONE && ch < nnodes) {
        const uint64_t vw = sld64((const uint64_t*)(nodes + (uint64_t)ch * NODE_BYTES + 8));
        atomicAdd(a.visits + t * a.stride + j, (int32_t)(uint32_t)vw);
        if ((uint32_t)(vw >> 32)) atomicAdd(a.wins + t * a.stride + j, (int32_t)(uint32_t)(vw >> 32));
      }
    }
  }
  if (lane == 0 && a.totals) {
    atomicAdd(a.totals + 0, s_moves);
    atomicAdd(a.totals + 1, (unsigned long long)a.budget);
    if (s_unfinished) atomicAdd(a.totals + 2, (unsigned long long)s_unfinished);
    atomicAdd(a.totals + 3, (unsigned long long)(nnodes - 1u));
  }
}

// ddz_search_choose: the canonical id of the first maximum of wins / visits over the entries with visits > 0 of
// [0 .. counts[t]) (get_bestchild_: the win ratio alone), compared exactly as w_a * v_b > w_b * v_a in 64-bit integers, ties
// to the lowest index; -1 where nothing was visited.  One wavefront per table.
__global__ __launch_bounds__(BLOCK) void k_search_choose(const int32_t* __restrict__ counts, const int32_t* __restrict__ ids,
                                                         int64_t stride, const int32_t* __restrict__ visits,
                                                         const int32_t* __restrict__ wins, int32_t* __restrict__ choice, int64_t T) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (t >= T) return;   // (whole waves)
  int64_t c = counts[t];
  if (c > stride) c = stride;
  int64_t bw = 0, bv = 0;   // this lane's best (first maximum over its ascending j); bv = 0: none
  uint32_t at = SEARCH_NONE;
  for (int64_t j = lane; j < c; j += 64) {
    const int64_t v = visits[t * stride + j], w = wins[t * stride + j];
    if (v > 0 && (bv == 0 || w * bv > bw * v)) { bw = w; bv = v; at = (uint32_t)j; }
  }
  // the wave's first maximum: a butterfly over (w, v, at) with the same exact comparison, ties to the lower index
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t ow = (int64_t)(((uint64_t)(uint32_t)__shfl_xor((int)(bw >> 32), off) << 32) | (uint32_t)__shfl_xor((int)bw, off));
    const int64_t ov = (int64_t)(((uint64_t)(uint32_t)__shfl_xor((int)(bv >> 32), off) << 32) | (uint32_t)__shfl_xor((int)bv, off));
    const uint32_t oat = (uint32_t)__shfl_xor((int)at, off);
    if (ov > 0) {
      const bool better = bv == 0 || ow * bv > bw * ov || (ow * bv == bw * ov && oat < at);
      if (better) { bw = ow; bv = ov; at = oat; }
    }
  }
  if (lane == 0) choice[t] = at == SEARCH_NONE ? -1 : ids[t * stride + at];
}
