// ddz_ismcts.h -- k_ismcts: single-observer information-set MCTS ("search spec v2 (ISMCTS)"; Whitehouse, Powley,
// Cowling, CIG 2011; Cowling, Powley, Whitehouse, TCIAIG 4(2), 2012).  Included by ddz_engine.hip behind ddz_search.h, inside
// its anonymous namespace: SearchArgs, search_value, the LN table, SEARCH_WAVES / SEARCH_PATH / SEARCH_NONE and the choose
// kernel are ddz_search.h's, the entry into a table, the redeal, the ply and the wavefront-scope accesses are ddz_ply.h's.
//
// One wavefront per WORK ITEM (table t, tree c), always the hidden form.  Where k_search<true> builds tree c on world c for
// its whole budget, k_ismcts builds ONE tree over all its worlds: iteration i deals world k = c * budget + i (redeal_wave,
// playout spec v2) and every step of the descent ENUMERATES the list of the state in that world (k_search re-applies stored
// moves and enumerates only where it expands).  A node is (parent, the move into it); a step sees the children whose moves
// are in this world's list and no others.
//
// WORKSPACE.  ismcts_tree_bytes(budget) per (table, tree), a function of the budget alone:
//   nodes  [budget + 1] x 32 bytes: move u64 (count word | category << 60) | V u32 | W u32 | A u32 | parent u32 |
//          meta u32 (terminal << 26 | winner << 27, as k_search's) | 0 u32
//   table  [H] x 8 bytes, H = the power of two >= 2 * (budget + 1): open addressing with linear probing, entry =
//          mix(parent, count word) << 32 | child, 0 = empty (a child is never node 0).  The 32-bit mix only filters: a hit
//          is a child whose STORED parent and count word both match, so two keys never merge.
// One iteration creates at most one node: the table is never more than half full.  The wave zeroes its own table.
//
// A LIST IN LANES.  ply_list leaves the closed-form round as the mask okm (entry round_pre(lane) of the list in every lane of
// okm, n0 entries) and the tail staged in LDS (entries n0 ..).  Trip 0 of a pass looks up the round, lane by lane; trips 1 ..
// look up 64 staged entries each.  Both orders ascend with the lane, so a ballot ranks the entries without a child.  Pass 1
// counts them, keeps each lane's best selectable child and raises A of every child it finds (each child is found by one lane,
// once per iteration: the values use the counts of before); only then the wave decides.  Expansion runs the lookups a second
// time to find the r-th entry without a child.  Pass 1, that ranking and the selection's reduce are the functions ismcts_pass1
// / ismcts_untried / ismcts_select below: k_gismcts (ddz_gismcts.h) calls them too, with W in 1024ths.  So it does the other
// pieces of spec v2 a descent is made of, stated here once: a new node's record and table entry (ismcts_make_node), the
// selection step (ismcts_descend) and the root's children leaving (ismcts_root_out).  The backup of a path and the totals
// (path_backup<INODE_BYTES>, search_totals_out) are ddz_search.h's.
//
// LOOPS, MEMORY ORDERING: as ddz_search.h.  Every loop is counted (iterations by budget, the descent by
// DDZ_SEARCH_MAX_DEPTH, a probe by H, the trips by n <= STAGE_CAP, the playout by DDZ_PLAYOUT_MAX_PLIES); a wave waits for no
// other; the tree is touched by relaxed wavefront-scope vector loads and stores, ordered by search_fence at the end of every
// iteration, behind the zeroing and ahead of the backup.  Atomics: the root sums, the totals, the status word.
constexpr uint32_t INODE_BYTES = 32;

inline uint64_t ismcts_nodes_bytes(int64_t budget) { return (uint64_t)(budget + 1) * INODE_BYTES; }
inline uint64_t ismcts_tree_bytes(int64_t budget) { return ismcts_nodes_bytes(budget) + (8ull << search_hash_log(budget)); }

constexpr uint64_t NIB60 = 0x0FFFFFFFFFFFFFFFull;

__device__ __forceinline__ uint32_t ismcts_mix(uint32_t parent, uint64_t nib) {
  uint32_t h = parent * 0x9E3779B1u + (uint32_t)nib * 0x85EBCA6Bu + (uint32_t)(nib >> 32) * 0xC2B2AE35u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 13;
  return h;
}
// the child of (parent, count word nib), SEARCH_NONE where none was created.  Per lane; at most H probes.
__device__ __forceinline__ uint32_t ismcts_find(const uint8_t* nodes, const uint64_t* tab, uint32_t hlog, uint32_t nnodes,
                                                uint32_t parent, uint64_t nib) {
  const uint32_t hmask = (1u << hlog) - 1u;
  const uint32_t mix = ismcts_mix(parent, nib);
  uint32_t h = mix >> (32u - hlog);
  for (uint32_t p = 0; p <= hmask; ++p) {
    const uint64_t e = sld64(tab + h);
    if (e == 0) return SEARCH_NONE;
    const uint32_t ch = (uint32_t)e;
    if ((uint32_t)(e >> 32) == mix && ch < nnodes) {
      const uint8_t* cr = nodes + (uint64_t)ch * INODE_BYTES;
      if (sld32((const uint32_t*)(cr + 20)) == parent && (sld64((const uint64_t*)cr) & NIB60) == nib) return ch;
    }
    h = (h + 1u) & hmask;
  }
  return SEARCH_NONE;
}
__device__ __forceinline__ void ismcts_insert(uint64_t* tab, uint32_t hlog, uint32_t parent, uint64_t nib, uint32_t child) {
  const uint32_t hmask = (1u << hlog) - 1u;
  const uint32_t mix = ismcts_mix(parent, nib);
  uint32_t h = mix >> (32u - hlog);
  for (uint32_t p = 0; p <= hmask; ++p) {
    if (sld64(tab + h) == 0) {
      sst64(tab + h, ((uint64_t)mix << 32) | child);
      return;
    }
    h = (h + 1u) & hmask;
  }
}

// this lane's entry of trip `trip` of the list ply_list left: trip 0 = the round (lane in okm -> entry round_pre), trip k >= 1
// = staged entries 64 (k - 1) ...  -> its index in the list, -1 where the lane holds none; nib = its count word.
__device__ __forceinline__ int ismcts_lane_entry(int trip, uint64_t okm, int n0, int n, uint32_t info, const uint64_t* stage,
                                                 int lane, uint64_t& nib) {
  nib = 0;
  if (trip == 0) {
    if (!((okm >> lane) & 1ull)) return -1;
    const bool lead = (info & 0xFF) == EMPTY;
    uint32_t scat, svlv, ncards;
    if (lead) round_entry<true>(lane, 0u, nib, scat, svlv, ncards);
    else round_entry<false>(lane, info & 0xFF, nib, scat, svlv, ncards);
    return lead ? round_pre(okm) : round_pre((uint32_t)okm);
  }
  const int k = (trip - 1) * 64 + lane;
  if (k >= n - n0) return -1;
  nib = stage[k] & NIB60;
  return n0 + k;
}

// pass 1 of a descent step at `node`, over the list ply_list left (trips = 1 + the staged trips): the child of every entry is
// looked up; the entries without one are counted (-> untried, wave-uniform), every child found has its A raised, and each
// lane keeps the best of its selectable children (value on the counts of BEFORE; bits, list index, child: at = SEARCH_NONE
// where the lane has none).  ONE: the unit W is counted in (search_value's).  Shared by k_ismcts and k_gismcts.
template <uint32_t ONE = 1>
__device__ __forceinline__ uint32_t ismcts_pass1(uint8_t* nodes, const uint64_t* tab, uint32_t hlog, uint32_t nnodes, uint32_t node,
                                                 int trips, uint64_t okm, int n0, int n, uint32_t info, const uint64_t* stage, int lane,
                                                 const float* ln, float c, bool own, bool sides, uint32_t& best, uint32_t& at,
                                                 uint32_t& bchild) {
  const bool take_max = own || sides;
  uint32_t untried = 0;
  best = 0; at = SEARCH_NONE; bchild = SEARCH_NONE;
  for (int trip = 0; trip < trips; ++trip) {
    uint64_t nib;
    const int j = ismcts_lane_entry(trip, okm, n0, n, info, stage, lane, nib);
    uint32_t ch = SEARCH_NONE;
    if (j >= 0) ch = ismcts_find(nodes, tab, hlog, nnodes, node, nib);
    untried += (uint32_t)__builtin_popcountll(__ballot(j >= 0 && ch == SEARCH_NONE));
    if (ch != SEARCH_NONE) {
      uint8_t* cr = nodes + (uint64_t)ch * INODE_BYTES;
      const uint64_t vw = sld64((const uint64_t*)(cr + 8));
      const uint32_t V = (uint32_t)vw, W = (uint32_t)(vw >> 32);
      const uint32_t A = sld32((const uint32_t*)(cr + 16));
      sst32((uint32_t*)(cr + 16), A + 1u);
      if (V > 0) {
        const float two_ln = 2.0f * ln[A <= (uint32_t)DDZ_SEARCH_MAX_BUDGET ? A : (uint32_t)DDZ_SEARCH_MAX_BUDGET];
        // (values are non-negative floats: their bit patterns order as they do)
        const uint32_t bits = __float_as_uint(search_value<ONE>(own ? W : (sides ? V * ONE - W : W), V, two_ln, c));
        if (at == SEARCH_NONE || (take_max ? bits > best : bits < best)) { best = bits; at = (uint32_t)j; bchild = ch; }
      }
    }
  }
  return rfl(untried);
}

// the expansion's list index: the r-th entry without a child, ascending (r < untried, wave-uniform: a second run of the
// lookups); -1 where there is none (cannot happen)
__device__ __forceinline__ int ismcts_untried(const uint8_t* nodes, const uint64_t* tab, uint32_t hlog, uint32_t nnodes, uint32_t node,
                                              int trips, uint64_t okm, int n0, int n, uint32_t info, const uint64_t* stage, int lane,
                                              uint32_t untried, uint32_t r) {
  if (untried == (uint32_t)n) return (int)r;
  for (int trip = 0; trip < trips; ++trip) {
    uint64_t nib;
    const int j = ismcts_lane_entry(trip, okm, n0, n, info, stage, lane, nib);
    bool open = false;
    if (j >= 0) open = ismcts_find(nodes, tab, hlog, nnodes, node, nib) == SEARCH_NONE;
    const uint64_t um = __ballot(open);
    const uint32_t cnt = (uint32_t)__builtin_popcountll(um);
    if (r < cnt) {
      const uint64_t below = um & ((1ull << lane) - 1ull);
      const uint64_t hit = __ballot(open && (uint32_t)__builtin_popcountll(below) == r);
      return (int)rl((uint32_t)j, (int)__builtin_ctzll(hit));
    }
    r -= cnt;
  }
  return -1;
}

// the selection among the lanes' bests of pass 1 (get_bestchild.py:20-32 with A for N): the maximum (take_max) or the minimum,
// ties to the lowest index of the list -> that index, SEARCH_NONE where no lane holds one; child: its node (wave-uniform)
__device__ __forceinline__ uint32_t ismcts_select(bool take_max, uint32_t best, uint32_t at, uint32_t bchild, uint32_t& child) {
  uint32_t m;
  if (take_max) m = (uint32_t)wave_max_i32(at == SEARCH_NONE ? (int)0x80000000 : (int)best);
  else m = wave_min_u32(at == SEARCH_NONE ? 0xFFFFFFFFu : best);
  const uint32_t first = wave_min_u32((at != SEARCH_NONE && best == m) ? at : SEARCH_NONE);   // ties: the lowest index
  child = first == SEARCH_NONE ? SEARCH_NONE : rfl(wave_min_u32((at == first) ? bchild : SEARCH_NONE));
  return first;
}

// expansion: the child `made` of `node` by the move (snib, scat) of `mover` (over: it emptied the hand).  Lane 0 writes the
// record whole (V = W = 0 until the backup, A = 1), then its table entry, and puts it on the path below `depth`.
__device__ __forceinline__ void ismcts_make_node(uint8_t* nodes, uint64_t* tab, uint32_t hlog, uint32_t node, uint32_t made,
                                                 uint64_t snib, uint32_t scat, bool over, int mover, uint16_t* path, int depth, int lane) {
  if (lane == 0) {
    uint64_t* q = (uint64_t*)(nodes + (uint64_t)made * INODE_BYTES);
    sst64(q, snib | ((uint64_t)scat << 60));
    sst64(q + 1, 0ull);
    sst64(q + 2, 1ull | ((uint64_t)node << 32));
    sst64(q + 3, over ? (1u << 26) | ((uint32_t)mover << 27) : 0u);
    ismcts_insert(tab, hlog, node, snib, made);
    path[depth + 1] = (uint16_t)made;
  }
}

// the selection step: the selected entry (snib, scat, svlv: as ply_entry gives it) is played, the turn passes on and `child`
// goes on the path one level down.  (An emptied hand: the child is terminal, the next trip of the descent scores it.)
__device__ __forceinline__ void ismcts_descend(uint64_t snib, uint32_t scat, uint32_t svlv, uint32_t child, uint64_t& hc, uint64_t& hn,
                                               uint64_t& hp, uint32_t& trick, int& passes, uint32_t& ply, int& role, uint16_t* path,
                                               int& depth, int lane) {
  const uint64_t hnew = ply_play(snib, scat, svlv, hc, trick, passes, ply);
  __builtin_amdgcn_wave_barrier();   // the staging list is reused by the next level
  ply_turn(hnew, hc, hn, hp, role);
  depth += 1;
  if (lane == 0) path[depth] = (uint16_t)child;
}

// the root's children leave: visits / wins of table t += V / W at their index j < bound of the root's list (okm, n0, n, info:
// as ply_list left it, the same in every world)
template <class Bound>
__device__ __forceinline__ void ismcts_root_out(const SearchArgs& a, int64_t t, const uint8_t* nodes, const uint64_t* tab,
                                                uint32_t nnodes, uint64_t okm, int n0, int n, uint32_t info, const uint64_t* stage,
                                                Bound bound, int lane) {
  const int trips = 1 + (n - n0 + 63) / 64;
  for (int trip = 0; trip < trips; ++trip) {
    uint64_t nib;
    const int j = ismcts_lane_entry(trip, okm, n0, n, info, stage, lane, nib);
    if (j >= 0 && j < bound) {
      const uint32_t ch = ismcts_find(nodes, tab, a.hash_log, nnodes, 0u, nib);
      if (ch != SEARCH_NONE) {
        const uint64_t vw = sld64((const uint64_t*)(nodes + (uint64_t)ch * INODE_BYTES + 8));
        atomicAdd(a.visits + t * a.stride + j, (int32_t)(uint32_t)vw);
        if ((uint32_t)(vw >> 32)) atomicAdd(a.wins + t * a.stride + j, (int32_t)(uint32_t)(vw >> 32));
      }
    }
  }
}

__global__ __launch_bounds__(SEARCH_WAVES * 64, 6) void k_ismcts(SearchArgs a) {
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
  const RootHands rh = root_hands<true>(R, a.roles, lane);
  if (rh.kind == ROOT_IDLE) return;   // not dealt, done, or not this call's seat: nothing runs
  if (rh.kind == ROOT_OUTSIDE) {      // outside the domain: nothing runs, the workspace is not touched
    if (lane == 0 && tree == 0) atomicOr(a.status, DDZ_ST_DOMAIN);
    return;
  }
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const uint64_t gid = a.gid_base + (uint64_t)t;
  const uint32_t hlog = a.hash_log;
  uint8_t* const nodes = a.work + (uint64_t)item * a.tree_bytes;
  uint64_t* const tab = (uint64_t*)(nodes + (uint64_t)(a.budget + 1) * INODE_BYTES);
  // the root actor's list is the same in every world: an empty one (or one the slab cannot hold) runs nothing
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
  if (lane < 4) sst64((uint64_t*)nodes + lane, lane == 2 ? (uint64_t)SEARCH_NONE << 32 : 0ull);   // node 0: no move, no parent
  search_fence();
  uint32_t nnodes = 1;
  unsigned long long s_moves = 0;
  uint32_t s_unfinished = 0;
  for (uint32_t it = 0; it < a.budget; ++it) {
    // this iteration's world: k = c * budget + i of playout spec v2 (the staging list serves as the redeal's keys)
    uint64_t hc = root.hc0, hn, hp;
    redeal_wave(gid, tree * a.budget + it, a.k0, a.k1, lane, rh.pool, rh.n_next, stage, hn, hp);
    uint32_t trick = root.trick0, ply = root.ply0;
    int passes = root.passes0, role = role0;
    uint32_t node = 0;
    int depth = 0;          // path[0 .. depth] are the nodes backed up
    int winner = -1;
    if (lane == 0) path[0] = 0;
    for (int d = 0; d <= DDZ_SEARCH_MAX_DEPTH; ++d) {
      const uint32_t meta = rfl(sld32((const uint32_t*)(nodes + (uint64_t)node * INODE_BYTES + 24)));
      if ((meta >> 26) & 1u) {   // the move into this node emptied a hand: scored without a playout
        winner = (int)((meta >> 27) & 3u);
        break;
      }
      if (d == DDZ_SEARCH_MAX_DEPTH) break;   // reward 0, unfinished
      const uint32_t info = ply_info(trick, passes);
      uint64_t okm; int n0;
      const int n = ply_list(hc, info, hot, lane, stage, svl, okm, n0);
      __builtin_amdgcn_wave_barrier();
      if (n > STAGE_CAP) {
        if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
        break;
      }
      if (n <= 0) break;   // outside the domain: unfinished
      const int trips = 1 + (n - n0 + 63) / 64;
      // ---- pass 1: every entry's child; the entries without one counted, the best of the others kept, their A raised
      const bool sides = a.mode == (uint32_t)DDZ_SEARCH_SIDES;
      const bool own = sides ? same_side(role, role0) : (role == role0);
      uint32_t best, at, bchild;
      const uint32_t untried = ismcts_pass1(nodes, tab, hlog, nnodes, node, trips, okm, n0, n, info, stage, lane, a.ln, a.c, own, sides,
                                            best, at, bchild);
      if (untried > 0) {
        // ---- expansion: the (draw_e * |U|) >> 32-th entry without a child, ascending
        const uint32_t de = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), (tree << 16) | it, RNG_EXPAND << 16), a.k0, a.k1).x;
        const int idx = ismcts_untried(nodes, tab, hlog, nnodes, node, trips, okm, n0, n, info, stage, lane, untried,
                                       rfl(__umulhi(de, untried)));
        if (idx < 0 || idx >= n) break;   // (cannot happen: `untried` entries without a child exist)
        uint64_t snib; uint32_t scat, svlv;
        ply_entry(okm, n0, idx, info, stage, svl, snib, scat, svlv);
        const uint32_t made = nnodes++;
        s_moves += 1;
        const int mover = role;
        const bool over = ply_apply(snib, scat, svlv, hc, hn, hp, trick, passes, role, ply);
        ismcts_make_node(nodes, tab, hlog, node, made, snib, scat, over, mover, path, depth, lane);
        depth += 1;
        if (over) {
          winner = mover;
          break;
        }
        // ---- playout from the new child: draws of domain 7 keyed by (gid, tree, iteration, ply), as k_search's
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
      // ---- selection among the children whose moves are in this world's list (get_bestchild.py:20-32 with A for N)
      uint32_t child;
      const uint32_t first = ismcts_select(own || sides, best, at, bchild, child);
      if (first == SEARCH_NONE) break;   // (cannot happen: every child was backed up when it was made)
      uint64_t snib; uint32_t scat, svlv;
      ply_entry(okm, n0, (int)first, info, stage, svl, snib, scat, svlv);
      s_moves += 1;
      ismcts_descend(snib, scat, svlv, child, hc, hn, hp, trick, passes, ply, role, path, depth, lane);
      node = child;
    }
    // ---- backup: V += 1, W += score on every node of the path, the new node included
    const uint32_t score = (winner >= 0 && same_side(winner, role0)) ? 1u : 0u;
    if (winner < 0) s_unfinished += 1;
    search_fence();   // the path, the new record and the raised A's are written
    path_backup<INODE_BYTES>(nodes, path, depth, score, lane);
    search_fence();
  }
  // ---- the root's children leave: visits / wins += V / W at their index of the root's list
  {
    const uint32_t info = ply_info(root.trick0, root.passes0);
    uint64_t okm; int n0;
    const int n = ply_list(root.hc0, info, hot, lane, stage, svl, okm, n0);
    __builtin_amdgcn_wave_barrier();
    ismcts_root_out(a, t, nodes, tab, nnodes, okm, n0, n, info, stage, n_root, lane);
  }
  search_totals_out(a.totals, s_moves, a.budget, s_unfinished, nnodes, lane);
}
