// ddz_search.h -- k_search / k_search_choose: UCT tree search around the playouts ("search spec v1 (UCT)"; the
// reference's MCTS player: server/mcts/interface.py:37-43 with tree_policy / get_bestchild.py / tree.py:33-51 / backup.py).
// Included by ddz_engine.hip behind ddz_ply.h and ddz_playout.h, inside its anonymous namespace.  The entry into a table
// (table_enter, root_hands: the root, its hands, the hidden-hand domain), the redeal, every piece of a ply and the wavefront-scope
// accesses to the tree (sld / sst / search_fence) are ddz_ply.h's, shared with the other three; this header holds the tree.
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
struct SearchArgs : PlyArgs {
  uint32_t budget, trees, mode;
  float c;
  int64_t stride;           // visits / wins are [T][stride]
  int32_t* visits;
  int32_t* wins;
  unsigned long long* totals;  // {moves applied, iterations run, iterations scored unfinished, nodes created} or null
  uint32_t roles;           // bit r = tables whose actor is role r take part; 7 in the open form
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

// value = W / V + c * sqrt((2 * LN[N]) / V): five correctly rounded fp32 operations, nothing fused (get_bestchild.py:9-18).
// ONE: the unit W is counted in (1 here; DDZ_GUIDED_ONE in ddz_guided.h, whose mean is scaled by the exact 1 / ONE)
template <uint32_t ONE = 1>
__device__ __forceinline__ float search_value(uint32_t w, uint32_t v, float two_ln, float c) {
#pragma clang fp contract(off)
  const float fv = (float)v;
  float mean = (float)w / fv;
  if constexpr (ONE != 1) mean = mean * (1.0f / (float)ONE);
  const float q = two_ln / fv;
  const float r = __builtin_sqrtf(q);
  const float bonus = c * r;
  return mean + bonus;
}

// the expansion's list index at a node with n entries of which nchild have a child: the r-th untried one, ascending
// (r < n - nchild, wave-uniform); -1 where there is none (cannot happen)
__device__ __forceinline__ int search_untried(const uint64_t* tab, uint32_t hlog, uint32_t node, int n, uint32_t nchild, uint32_t r,
                                              int lane) {
  if (nchild == 0) return (int)r;
  for (int b = 0; b < n; b += 64) {
    const int j = b + lane;
    bool untried = false;
    if (j < n) untried = search_find(tab, hlog, node * 512u + (uint32_t)j + 1u) == SEARCH_NONE;
    const uint64_t um = __ballot(untried);
    const uint32_t cnt = (uint32_t)__builtin_popcountll(um);
    if (r < cnt) {
      const uint64_t below = um & ((1ull << lane) - 1ull);
      const uint64_t hit = __ballot(untried && (uint32_t)__builtin_popcountll(below) == r);
      return b + (int)__builtin_ctzll(hit);
    }
    r -= cnt;
  }
  return -1;
}

// selection at a fully expanded node with n entries (get_bestchild.py:20-32): the child with the maximum (take_max) or the
// minimum value, ties to the lowest list index; SEARCH_NONE where no child was visited (cannot happen).  own: the node's
// actor counts W as it stands; otherwise `sides` counts V * ONE - W.  Wave-uniform result.
template <uint32_t ONE = 1>
__device__ __forceinline__ uint32_t search_select(const uint8_t* nodes, const uint64_t* tab, uint32_t hlog, uint32_t node, int n,
                                                  uint32_t nnodes, float two_ln, float c, bool own, bool sides, int lane) {
  const bool take_max = own || sides;
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
          const uint32_t bits = __float_as_uint(search_value<ONE>(own ? W : (sides ? V * ONE - W : W), V, two_ln, c));
          if (at == SEARCH_NONE || (take_max ? bits > best : bits < best)) { best = bits; at = (uint32_t)j; bchild = ch; }
        }
      }
    }
  }
  uint32_t m;
  if (take_max) m = (uint32_t)wave_max_i32(at == SEARCH_NONE ? (int)0x80000000 : (int)best);
  else m = wave_min_u32(at == SEARCH_NONE ? 0xFFFFFFFFu : best);
  const uint32_t first = wave_min_u32((at != SEARCH_NONE && best == m) ? at : SEARCH_NONE);   // ties: the lowest index
  if (first == SEARCH_NONE) return SEARCH_NONE;
  return rl(bchild, (int)(first & 63u));
}

// the backup of the later specs (k_ismcts, k_guided, k_gismcts): V += 1, W += score on path[0 .. depth] (the wave's LDS copy),
// lane l the l-th node.  The V | W word stands at byte 8 of a record of either size.  The caller's fences stand around it.
template <uint32_t NODE_STRIDE>
__device__ __forceinline__ void path_backup(uint8_t* nodes, const uint16_t* path, int depth, uint32_t score, int lane) {
  for (int b = 0; b <= depth; b += 64) {
    const int l = b + lane;
    if (l <= depth) {
      uint64_t* p = (uint64_t*)(nodes + (uint64_t)path[l] * NODE_STRIDE + 8);
      const uint64_t vw = sld64(p);
      sst64(p, vw + 1ull + ((uint64_t)score << 32));
    }
  }
}

// the totals of one work item leave (the same kernels'): {moves applied, iterations run, scored unfinished, nodes created}
__device__ __forceinline__ void search_totals_out(unsigned long long* totals, unsigned long long moves, uint32_t iterations,
                                                  uint32_t unfinished, uint32_t nnodes, int lane) {
  if (lane == 0 && totals) {
    atomicAdd(totals + 0, moves);
    atomicAdd(totals + 1, (unsigned long long)iterations);
    if (unfinished) atomicAdd(totals + 2, (unsigned long long)unfinished);
    atomicAdd(totals + 3, (unsigned long long)(nnodes - 1u));
  }
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
  uint4 R;
  if (!table_enter<SEARCH_WAVES>(a, t, lane, hot, R)) return;
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  uint16_t* path = s_path[wv];
  const RootHands rh = root_hands<HIDDEN>(R, a.roles, lane);
  if (rh.kind == ROOT_IDLE) return;   // not dealt, done, or not this call's seat: nothing runs
  if (rh.kind == ROOT_OUTSIDE) {      // outside the domain: nothing runs, the workspace is not touched
    if (lane == 0 && tree == 0) atomicOr(a.status, DDZ_ST_DOMAIN);
    return;
  }
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  uint64_t hn0 = rh.hn0, hp0 = rh.hp0;
  const uint64_t gid = a.gid_base + (uint64_t)t;
  // hidden form: tree c plays on world k = c of playout spec v2: the same pool, the same domain, the same deal
  if constexpr (HIDDEN) redeal_wave(gid, tree, a.k0, a.k1, lane, rh.pool, rh.n_next, stage, hn0, hp0);
  const uint32_t hlog = a.hash_log;
  uint8_t* const base = a.work + (uint64_t)item * a.tree_bytes;
  uint8_t* const nodes = base;
  uint64_t* const tab = (uint64_t*)(base + (((uint64_t)(a.budget + 1) * NODE_BYTES + 15) & ~15ull));
  // the root's list: its size is the root's n; an empty list (or one the slab cannot hold) runs nothing
  int n_root;
  {
    uint64_t okm; int n0;
    n_root = ply_list(root.hc0, ply_info(root.trick0, root.passes0), hot, lane, stage, svl, okm, n0);
    __builtin_amdgcn_wave_barrier();
    if (n_root > STAGE_CAP || n_root > a.stride) {
      if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
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
    uint64_t hc = root.hc0, hn = hn0, hp = hp0;
    uint32_t trick = root.trick0, ply = root.ply0;
    int passes = root.passes0, role = role0;
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
      const uint32_t info = ply_info(trick, passes);
      if ((int)nchild < n) {
        // ---- expansion: the (draw_e * u) >> 32-th untried list index, ascending
        uint64_t okm; int n0;
        const int nn = ply_list(hc, info, hot, lane, stage, svl, okm, n0);
        if (nn != n) break;   // (cannot happen: the state of a node is a function of its path)
        const uint32_t u = (uint32_t)n - nchild;
        const uint32_t de = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), (tree << 16) | it, RNG_EXPAND << 16), a.k0, a.k1).x;
        const int idx = search_untried(tab, hlog, node, n, nchild, rfl(__umulhi(de, u)), lane);
        if (idx < 0 || idx >= n) break;   // (cannot happen: u untried indices exist)
        uint64_t snib; uint32_t scat, svlv;
        ply_entry(okm, n0, idx, info, stage, svl, snib, scat, svlv);
        made = nnodes++;
        made_move = snib | ((uint64_t)scat << 60);
        made_meta = svlv & 0xFFFFu;
        if (lane == 0) {
          search_insert(tab, hlog, node * 512u + (uint32_t)idx + 1u, made);
          sst32((uint32_t*)(nodes + (uint64_t)node * NODE_BYTES + 20), nchild + 1u);
        }
        s_moves += 1;
        if (ply_apply(snib, scat, svlv, hc, hn, hp, trick, passes, role, ply)) {
          winner = role;
          made_meta |= (1u << 26) | ((uint32_t)role << 27);
          break;
        }
        // ---- playout from the new child: draws of domain 7 keyed by (gid, tree, iteration, ply)
        uint32_t draws = 0, dnext = 64;
        for (int s = 0; s < DDZ_PLAYOUT_MAX_PLIES; ++s) {
          uint32_t dn = rfl(dnext);
          if (dn >= 64u) {
            dn = 0;
            dnext = 0;
            draws = ply_draw(gid, (tree << 16) | it, RNG_TREE_PLAYOUT, ply, lane, a.k0, a.k1);
          }
          const uint32_t draw = rl(draws, (int)dn);
          const uint32_t pinfo = ply_info(trick, passes);
          uint64_t pokm; int pn0;
          int pn = ply_list(hc, pinfo, hot, lane, stage, svl, pokm, pn0);
          if (pn > STAGE_CAP) {
            if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
            pn = 0;
          }
          if (s == 0) made_meta |= (uint32_t)pn << 16;   // the child's n
          if (pn <= 0) break;   // stopped unfinished
          const int pidx = (int)rfl(__umulhi(draw, (uint32_t)pn));
          uint64_t pnib; uint32_t pcat, pvl;
          ply_entry(pokm, pn0, pidx, pinfo, stage, svl, pnib, pcat, pvl);
          s_moves += 1;
          dnext += 1;
          if (ply_apply(pnib, pcat, pvl, hc, hn, hp, trick, passes, role, ply)) {
            winner = role;
            break;
          }
        }
        break;
      }
      // ---- selection at a fully expanded node (get_bestchild.py:20-32)
      const uint32_t N = rfl(sld32((const uint32_t*)(nr + 8)));
      const float two_ln = 2.0f * a.ln[N <= (uint32_t)DDZ_SEARCH_MAX_BUDGET ? N : (uint32_t)DDZ_SEARCH_MAX_BUDGET];
      const bool own = a.mode == (uint32_t)DDZ_SEARCH_SIDES ? same_side(role, role0) : (role == role0);
      const uint32_t child = search_select(nodes, tab, hlog, node, n, nnodes, two_ln, a.c, own, a.mode == (uint32_t)DDZ_SEARCH_SIDES, lane);
      if (child == SEARCH_NONE) break;   // (cannot happen: a fully expanded node has n visited children)
      const uint8_t* cr = nodes + (uint64_t)child * NODE_BYTES;
      const uint64_t mv = sld64((const uint64_t*)cr);
      const uint32_t cmeta = sld32((const uint32_t*)(cr + 16));
      const uint64_t snib = rfl64(mv & 0x0FFFFFFFFFFFFFFFull);
      const uint32_t scat = rfl((uint32_t)(mv >> 60)), svlv = rfl(cmeta & 0xFFFFu);
      s_moves += 1;
      ply_turn(ply_play(snib, scat, svlv, hc, trick, passes, ply), hc, hn, hp, role);   // (an emptied hand: the child is terminal, the next trip scores it)
      node = child;
      depth += 1;
      if (lane == 0) path[depth] = (uint16_t)child;
    }
    // ---- backup: V += 1, W += score on every node of the path; the new node's record is written whole
    const uint32_t score = (winner >= 0 && same_side(winner, role0)) ? 1u : 0u;
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
