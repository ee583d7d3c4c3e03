// ddz_guided.h -- k_guided / k_guided_value: UCT with leaf values from outside the kernel ("search spec v3 (guided UCT)",
// DESIGN.md 4).  Included by ddz_engine.hip behind ddz_search.h, inside its anonymous namespace.  Spec v1's tree, hash table,
// selection (search_select), expansion pick (search_untried) and value (search_value, with the unit's exact 1 / ONE factor)
// are ddz_search.h's, the entry into a table, the redeal and every piece of a ply are ddz_ply.h's; this header holds the
// PHASED form: where k_search runs its whole budget in one launch with a playout under every new leaf, one launch of
// k_guided runs ONE iteration of every (table, tree) and leaves a new non-terminal leaf PENDING: its 176-byte state row goes
// out, its value comes back as an int32 in 1024ths with the next launch, which backs it up before it descends again.
//
// One wavefront per WORK ITEM (table t, tree c), 12-wave blocks as k_search.  Phases of a launch, wave-uniform:
//   OPEN   the root's list is sized, the hash table and the header are zeroed, node 0 is written.  Nothing else.
//   STEP   a pending leaf is backed up with values[item]; then, if it < budget, one iteration.
//   CLOSE  a pending leaf is backed up with values[item]; the root's children and the totals leave.
// The root is re-read (and, hidden, re-dealt) by every launch: the environment must not be stepped between OPEN and CLOSE.
//
// WORKSPACE per (table, tree), guided_tree_bytes(budget), a function of the budget alone:
//   header [16] u32: 0 live, 1 iteration number, 2 node count, 3 pending node (SEARCH_NONE: none), 4 pending depth, 5 the leaf
//          actor is on the root actor's side, 6 unfinished, 7 the pending node's meta, 8..9 its move, 10..11 moves applied
//   path   [SEARCH_PATH] u16, two to a word: the nodes of the pending iteration's descent, the root first
//   nodes, table: spec v1's (ddz_search.h)
// A table outside the hidden-hand domain raises status bit 6 and its workspace is never touched; an idle table's neither.
//
// LOOPS.  Every loop is counted, as in k_search; the iterations are the caller's launches.  A wave waits for no other wave.
//
// MEMORY ORDERING.  Kernel boundaries order the launches: what a launch stored is what the next one loads.  Inside a launch a
// tree, its header and its path are written and read by ONE wavefront through the relaxed wavefront-scope accesses and the
// fence of ddz_search.h (MEMORY ORDERING, there): vector instructions of one wave issued in order through one vector L1.
// values is read, leaf_rows and need are written with plain vector accesses: no wave reads what another wrote in a launch.
//
// THE PHASED SCAFFOLD is stated here once, for k_guided and for k_gismcts (ddz_gismcts.h), which keeps spec v2's tree in the same
// workspace: the view of a tree (GuidedTree, guided_tree), OPEN (guided_open, guided_open_header; node 0 is each kernel's), the
// check of a header (guided_header_live), the pending leaf's score and path (guided_pending_score), the rows a descent carries
// and the leaf's row (DescentRows), a leaf left pending (guided_leave_pending), the header at the end of a launch
// (guided_store_header) and the launch's outputs (guided_emit).  The backup of a path and the totals (path_backup,
// search_totals_out) are ddz_search.h's.  A kernel keeps its prologue, its descent loop and the order of these calls.
constexpr uint32_t GUIDED_ONE = DDZ_GUIDED_ONE;
constexpr int GUIDED_OPEN = 0, GUIDED_STEP = 1, GUIDED_CLOSE = 2;
constexpr uint32_t GUIDED_HDR_BYTES = 64;
constexpr uint32_t GUIDED_PATH_BYTES = (SEARCH_PATH * 2 + 15) & ~15;
enum { GH_LIVE = 0, GH_IT, GH_NNODES, GH_PENDING, GH_PDEPTH, GH_PSIDE, GH_UNFINISHED, GH_PMETA, GH_PMOVE, GH_MOVES = 10 };

struct GuidedArgs : SearchArgs {
  int phase;
  const int32_t* values;   // [T * trees] or null (the first step)
  uint8_t* leaf_rows;      // [T * trees][176]
  int32_t* need;           // [T * trees]
};

inline uint64_t guided_tree_bytes(int64_t budget) { return GUIDED_HDR_BYTES + GUIDED_PATH_BYTES + search_tree_bytes(budget); }

// one item's workspace.  The table starts at the first multiple of 16 behind the nodes: spec v1's 24-byte records are rounded
// up to it, spec v2's 32-byte records end on it.
struct GuidedTree {
  uint32_t* hdr;     // [16]
  uint32_t* gpath;   // [SEARCH_PATH / 2]
  uint8_t* nodes;    // [budget + 1] records of node_stride bytes
  uint64_t* tab;     // [1 << hash_log]
};
__device__ __forceinline__ GuidedTree guided_tree(uint8_t* work, int64_t item, uint64_t tree_bytes, uint32_t budget,
                                                  uint32_t node_stride) {
  uint8_t* const base = work + (uint64_t)item * tree_bytes;
  uint8_t* const nodes = base + GUIDED_HDR_BYTES + GUIDED_PATH_BYTES;
  return {(uint32_t*)base, (uint32_t*)(base + GUIDED_HDR_BYTES), nodes,
          (uint64_t*)(nodes + (((uint64_t)(budget + 1) * node_stride + 15) & ~15ull))};
}

// OPEN: the root's list is sized -> its n, 0 where the item stays dead (an empty list, or one the slab cannot hold: status bit
// 1); a live item's hash table is zeroed.  The kernel writes its node 0 behind this, then guided_open_header.
__device__ __forceinline__ int guided_open(const GuidedTree& g, const GuidedArgs& a, const PlayRoot& root, const HotTabT<false>& hot,
                                           int lane, uint64_t* stage, uint16_t* svl) {
  uint64_t okm; int n0;
  int n_root = ply_list(root.hc0, ply_info(root.trick0, root.passes0), hot, lane, stage, svl, okm, n0);
  __builtin_amdgcn_wave_barrier();
  if (n_root > STAGE_CAP || n_root > a.stride) {
    if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
    n_root = 0;
  }
  if (n_root > 0)
    for (uint32_t i = (uint32_t)lane; i < (1u << a.hash_log); i += 64) sst64(g.tab + i, 0ull);
  return n_root;
}
__device__ __forceinline__ void guided_open_header(uint32_t* hdr, bool live, int lane) {
  if (lane < 16) sst32(hdr + lane, lane == GH_LIVE ? (live ? 1u : 0u) : lane == GH_NNODES ? 1u : lane == GH_PENDING ? SEARCH_NONE : 0u);
  search_fence();
}

// a header OPEN did not write (a workspace of another budget, or none), or one whose fields are out of range, is dead: with a
// live one every index a STEP or a CLOSE computes stays inside the tree.  A dead item reads these header words and nothing else.
__device__ __forceinline__ bool guided_header_live(const uint32_t* hdr, uint32_t budget) {
  if (rfl(sld32(hdr + GH_LIVE)) != 1u) return false;
  const uint32_t it = rfl(sld32(hdr + GH_IT)), nnodes = rfl(sld32(hdr + GH_NNODES)), pending = rfl(sld32(hdr + GH_PENDING));
  return it <= budget && nnodes >= 1u && nnodes <= it + 1u &&
         (pending == SEARCH_NONE || (pending < nnodes && rfl(sld32(hdr + GH_PDEPTH)) <= (uint32_t)DDZ_SEARCH_MAX_DEPTH));
}

// the pending leaf's value -> its score: the chance in 1024ths that the LEAF actor's side wins (values[item], clamped), seen
// from the root's side.  The stored path is reloaded into LDS (every entry a node of this tree, whatever the words hold) and
// fenced; pdepth: the leaf's depth.
__device__ __forceinline__ uint32_t guided_pending_score(const GuidedTree& g, const int32_t* values, int64_t item, uint32_t nnodes,
                                                         uint16_t* path, int lane, int& pdepth) {
  pdepth = (int)rfl(sld32(g.hdr + GH_PDEPTH));
  int32_t v = values ? values[item] : 0;
  v = v < 0 ? 0 : v > (int32_t)GUIDED_ONE ? (int32_t)GUIDED_ONE : v;
  const uint32_t score = rfl(sld32(g.hdr + GH_PSIDE)) ? (uint32_t)v : GUIDED_ONE - (uint32_t)v;
  for (int w = lane; w < SEARCH_PATH / 2; w += 64) {
    const uint32_t two = sld32(g.gpath + w);
    path[2 * w] = (uint16_t)((two & 0xFFFFu) < nnodes ? two : 0u);
    path[2 * w + 1] = (uint16_t)((two >> 16) < nnodes ? two >> 16 : 0u);
  }
  search_fence();
  return score;
}

// the rows the hands' words do not carry along a descent, as lane f's row f (k_rollout's form): history, recent + category,
// taken, and byte 15 of every row (a hand row's: the cards left)
struct DescentRows {
  uint64_t P;
  uint32_t aux;
  // a move of `role` (envi.py:39-43 on the packed rows), before the turn passes on
  __device__ __forceinline__ void track(uint64_t snib, uint32_t scat, int role, int lane) {
    const int d = lane - role;
    const uint64_t add = (d == DDZ_F_HIST0 || lane == DDZ_F_TAKEN) ? snib : 0ull;
    P = d == DDZ_F_RECENT0 ? snib : P + add;
    aux = d == DDZ_F_RECENT0 ? scat : d == DDZ_F_HAND0 ? aux - (uint32_t)nib_sum(snib) : aux;
  }
  // this lane's 16 bytes of the leaf's 176-byte row, as state_import reads it: the hands back by role, the meta row as ddz_step
  // leaves it on a running table (my, mz, mw: the words of the root's meta row a leaf keeps)
  __device__ __forceinline__ uint4 leaf_row(uint64_t hc, uint64_t hn, uint64_t hp, int role, uint32_t ply, uint32_t my, uint32_t mz,
                                            uint32_t mw, int lane) const {
    const int rp1 = role_next(role), rm1 = role_prev(role);
    const uint64_t Pf = lane == role ? hc : lane == rp1 ? hn : lane == rm1 ? hp : P;
    uint4 r = unpack_row(Pf, aux);
    if (lane == DDZ_F_META) r = meta_after_ply(role, false, 0, 0u, my, ply, mz, mw);
    return r;
  }
};

// a leaf is left pending: the path[0 .. depth] of its descent is stored, two nodes to a word
__device__ __forceinline__ void guided_leave_pending(uint32_t* gpath, const uint16_t* path, int depth, int lane) {
  for (int w = lane; w < SEARCH_PATH / 2; w += 64) {
    const uint32_t lo = 2 * w <= depth ? path[2 * w] : 0u, hi = 2 * w + 1 <= depth ? path[2 * w + 1] : 0u;
    sst32(gpath + w, lo | (hi << 16));
  }
}

// the header at the end of a STEP or a CLOSE (k_guided stores GH_PMETA / GH_PMOVE on top); the caller's fence stands behind it
__device__ __forceinline__ void guided_store_header(uint32_t* hdr, uint32_t it, uint32_t nnodes, uint32_t pending, int depth,
                                                    uint32_t pside, uint32_t unfinished, unsigned long long moves, int lane) {
  if (lane == 0) {
    sst32(hdr + GH_IT, it);
    sst32(hdr + GH_NNODES, nnodes);
    sst32(hdr + GH_PENDING, pending);
    sst32(hdr + GH_PDEPTH, (uint32_t)depth);
    sst32(hdr + GH_PSIDE, pside);
    sst32(hdr + GH_UNFINISHED, unfinished);
    sst64((uint64_t*)(hdr + GH_MOVES), moves);
  }
}

// what a STEP leaves of every running item: its leaf's row (all zero without a pending leaf) and its need flag
__device__ __forceinline__ void guided_emit(const GuidedArgs& a, int64_t item, const uint4& Rleaf, int32_t needs, int lane) {
  if (a.phase == GUIDED_STEP) {
    if (lane < DDZ_NFIELDS) ((uint4*)(a.leaf_rows + (uint64_t)item * STATE_ROW_BYTES))[lane] = Rleaf;
    if (lane == 0) a.need[item] = needs;
  }
}

// path_backup on path[0 .. depth] and the new node's record, written whole
__device__ __forceinline__ void guided_backup(uint8_t* nodes, const uint16_t* path, int depth, uint32_t score, uint32_t made,
                                              uint64_t made_move, uint32_t made_meta, int lane) {
  path_backup<NODE_BYTES>(nodes, path, depth, score, lane);
  if (made != SEARCH_NONE && lane == 0) {
    uint8_t* q = nodes + (uint64_t)made * NODE_BYTES;
    sst64((uint64_t*)q, made_move);
    sst64((uint64_t*)(q + 8), 1ull | ((uint64_t)score << 32));
    sst32((uint32_t*)(q + 16), made_meta);
    sst32((uint32_t*)(q + 20), 0u);
  }
}

template <bool HIDDEN>
__global__ __launch_bounds__(SEARCH_WAVES * 64, 6) void k_guided(GuidedArgs a) {
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
  const uint32_t my = rl(R.y, DDZ_F_META), mz = rl(R.z, DDZ_F_META), mw = rl(R.w, DDZ_F_META);   // the meta row's words a leaf keeps
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  uint16_t* path = s_path[wv];
  // what a STEP leaves of an item without a pending leaf: a row with dealt = 0 (a leaf environment freezes it), need 0
  uint4 Rleaf = make_uint4(0, 0, 0, 0);
  int32_t needs = 0;
  const RootHands rh = root_hands<HIDDEN>(R, a.roles, lane);
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const GuidedTree g = guided_tree(a.work, item, a.tree_bytes, a.budget, NODE_BYTES);
  uint32_t* const hdr = g.hdr;
  uint8_t* const nodes = g.nodes;
  uint64_t* const tab = g.tab;
  const uint32_t hlog = a.hash_log;
  if (rh.kind == ROOT_OUTSIDE && lane == 0 && tree == 0) atomicOr(a.status, DDZ_ST_DOMAIN);   // outside the domain: nothing runs
  if (rh.kind == ROOT_INSIDE && a.phase == GUIDED_OPEN) {
    // ---- OPEN: the root's list is node 0's n
    const int n_root = guided_open(g, a, root, hot, lane, stage, svl);
    if (n_root > 0 && lane == 0) {   // node 0: no move, nothing visited
      sst64((uint64_t*)nodes, 0ull);
      sst64((uint64_t*)(nodes + 8), 0ull);
      sst32((uint32_t*)(nodes + 16), (uint32_t)n_root << 16);
      sst32((uint32_t*)(nodes + 20), 0u);
    }
    guided_open_header(hdr, n_root > 0, lane);
    return;
  }
  if (rh.kind == ROOT_INSIDE && guided_header_live(hdr, a.budget)) {
    uint32_t it = rfl(sld32(hdr + GH_IT)), nnodes = rfl(sld32(hdr + GH_NNODES));
    uint32_t s_unfinished = rfl(sld32(hdr + GH_UNFINISHED));
    unsigned long long s_moves = rfl64(sld64((const uint64_t*)(hdr + GH_MOVES)));
    const uint32_t pending = rfl(sld32(hdr + GH_PENDING));
    if (pending != SEARCH_NONE) {
      // ---- the pending leaf is backed up, its record written whole
      int pdepth;
      const uint32_t score = guided_pending_score(g, a.values, item, nnodes, path, lane, pdepth);
      guided_backup(nodes, path, pdepth, score, pending, sld64((const uint64_t*)(hdr + GH_PMOVE)), sld32(hdr + GH_PMETA), lane);
      search_fence();
    }
    uint32_t made = SEARCH_NONE;   // the node this launch creates and, where it is not terminal, leaves pending
    bool wait = false;
    int depth = 0;
    uint64_t made_move = 0;
    uint32_t made_meta = 0, pside = 0;
    if (a.phase == GUIDED_STEP && it < a.budget) {
      uint64_t hn0 = rh.hn0, hp0 = rh.hp0;
      const uint64_t gid = a.gid_base + (uint64_t)t;
      if constexpr (HIDDEN) redeal_wave(gid, tree, a.k0, a.k1, lane, rh.pool, rh.n_next, stage, hn0, hp0);
      uint64_t hc = root.hc0, hn = hn0, hp = hp0;
      uint32_t trick = root.trick0, ply = root.ply0;
      int passes = root.passes0, role = role0;
      DescentRows rows = {root.P, root.aux};
      const auto track = [&](uint64_t snib, uint32_t scat) { rows.track(snib, scat, role, lane); };   // (the mover: before the turn)
      uint32_t node = 0;
      int winner = -1;
      if (lane == 0) path[0] = 0;
      for (int d = 0; d <= DDZ_SEARCH_MAX_DEPTH; ++d) {
        const uint8_t* nr = nodes + (uint64_t)node * NODE_BYTES;
        const uint32_t meta = rfl(sld32((const uint32_t*)(nr + 16)));
        if ((meta >> 26) & 1u) {   // a terminal node reached by selection: scored at once
          winner = (int)((meta >> 27) & 3u);
          break;
        }
        const int n = (int)((meta >> 16) & 0x3FFu);
        if (n <= 0 || d == DDZ_SEARCH_MAX_DEPTH) break;   // outside the domain: score 0, unfinished
        const uint32_t nchild = rfl(sld32((const uint32_t*)(nr + 20)));
        const uint32_t info = ply_info(trick, passes);
        if ((int)nchild < n) {
          // ---- expansion: spec v1's draw and pick
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
          track(snib, scat);
          if (ply_apply(snib, scat, svlv, hc, hn, hp, trick, passes, role, ply)) {
            winner = role;
            made_meta |= (1u << 26) | ((uint32_t)role << 27);
            break;
          }
          // ---- a pending leaf: its n is the size of its state's list, its value is the caller's
          uint64_t pokm; int pn0;
          int pn = ply_list(hc, ply_info(trick, passes), hot, lane, stage, svl, pokm, pn0);
          __builtin_amdgcn_wave_barrier();
          if (pn > STAGE_CAP) {
            if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
            pn = 0;
          }
          made_meta |= (uint32_t)pn << 16;
          pside = same_side(role, role0) ? 1u : 0u;
          wait = true;
          break;
        }
        // ---- selection at a fully expanded node: spec v1's, W in 1024ths
        const uint32_t N = rfl(sld32((const uint32_t*)(nr + 8)));
        const float two_ln = 2.0f * a.ln[N <= (uint32_t)DDZ_SEARCH_MAX_BUDGET ? N : (uint32_t)DDZ_SEARCH_MAX_BUDGET];
        const bool sides = a.mode == (uint32_t)DDZ_SEARCH_SIDES;
        const bool own = sides ? same_side(role, role0) : (role == role0);
        const uint32_t child = search_select<GUIDED_ONE>(nodes, tab, hlog, node, n, nnodes, two_ln, a.c, own, sides, lane);
        if (child == SEARCH_NONE) break;   // (cannot happen: a fully expanded node has n visited children)
        const uint8_t* cr = nodes + (uint64_t)child * NODE_BYTES;
        const uint64_t mv = sld64((const uint64_t*)cr);
        const uint32_t cmeta = sld32((const uint32_t*)(cr + 16));
        const uint64_t snib = rfl64(mv & 0x0FFFFFFFFFFFFFFFull);
        const uint32_t scat = rfl((uint32_t)(mv >> 60)), svlv = rfl(cmeta & 0xFFFFu);
        s_moves += 1;
        track(snib, scat);
        ply_turn(ply_play(snib, scat, svlv, hc, trick, passes, ply), hc, hn, hp, role);
        node = child;
        depth += 1;
        if (lane == 0) path[depth] = (uint16_t)child;
      }
      it += 1;
      search_fence();   // the path is written
      if (wait) {
        Rleaf = rows.leaf_row(hc, hn, hp, role, ply, my, mz, mw, lane);
        needs = 1;
        guided_leave_pending(g.gpath, path, depth, lane);
      } else {
        const uint32_t score = (winner >= 0 && same_side(winner, role0)) ? GUIDED_ONE : 0u;
        if (winner < 0) s_unfinished += 1;
        guided_backup(nodes, path, depth, score, made, made_move, made_meta, lane);
      }
    }
    guided_store_header(hdr, it, nnodes, wait ? made : SEARCH_NONE, depth, pside, s_unfinished, s_moves, lane);
    if (lane == 0) {   // the record guided_backup writes when the leaf's value is there
      sst32(hdr + GH_PMETA, made_meta);
      sst64((uint64_t*)(hdr + GH_PMOVE), made_move);
    }
    search_fence();
    if (a.phase == GUIDED_CLOSE) {
      // ---- the root's children leave: visits / wins += V / W (1024ths) at their list index
      const int n_root = (int)((rfl(sld32((const uint32_t*)(nodes + 16))) >> 16) & 0x3FFu);
      for (int b = 0; b < n_root; b += 64) {
        const int j = b + lane;
        if (j < n_root && j < a.stride) {
          const uint32_t ch = search_find(tab, hlog, (uint32_t)j + 1u);
          if (ch != SEARCH_NONE && ch < nnodes) {
            const uint64_t vw = sld64((const uint64_t*)(nodes + (uint64_t)ch * NODE_BYTES + 8));
            atomicAdd(a.visits + t * a.stride + j, (int32_t)(uint32_t)vw);
            if ((uint32_t)(vw >> 32)) atomicAdd(a.wins + t * a.stride + j, (int32_t)(uint32_t)(vw >> 32));
          }
        }
      }
      search_totals_out(a.totals, s_moves, it, s_unfinished, nnodes, lane);
    }
  }
  guided_emit(a, item, Rleaf, needs, lane);
}

// k_guided_value: leaf values from a q slab.  One wavefront per leaf i with a running row whose actor's role is in
// net_roles: qmax = the maximum of q[i][0 .. n[i]), p = qmax * inv_reward[role], v = (int)rintf((p + 1) * 512) clamped to
// [0, ONE]; single fp32 operations, nothing fused; n = 0 or a NaN maximum gives ONE / 2.  Every other entry of values is left
// as it is (a second evaluator fills them).
struct GuidedValueArgs {
  const uint8_t* rows;     // [n_leaves][176]
  const int32_t* counts;   // [n_leaves]
  const float* q;          // [n_leaves][stride]
  int64_t stride, n_leaves;
  float inv_reward[3];
  uint32_t net_roles;
  int32_t* values;
};

__global__ __launch_bounds__(BLOCK) void k_guided_value(GuidedValueArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (i >= a.n_leaves) return;   // (whole waves)
  const uint8_t* meta = a.rows + i * STATE_ROW_BYTES + DDZ_F_META * 16;
  uint32_t role = meta[0];
  if (role > 2) role = 0;
  if (!meta[6] || meta[1] || !((a.net_roles >> role) & 1u)) return;
  int64_t n = a.counts[i];
  if (n > a.stride) n = a.stride;
  float m = -__builtin_inff();
  bool nan = false;
  for (int64_t j = lane; j < n; j += 64) {
    const float x = a.q[i * a.stride + j];
    nan = nan || x != x;
    m = x > m ? x : m;
  }
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  int32_t v = (int32_t)(GUIDED_ONE / 2);
  if (n > 0 && __ballot(nan) == 0ull) {
    const float p = m * (role == 0 ? a.inv_reward[0] : role == 1 ? a.inv_reward[1] : a.inv_reward[2]);
    const float s = p + 1.0f;
    const float x = s * 512.0f;
    const float r = __builtin_rintf(x);
    v = r <= 0.0f ? 0 : r >= (float)GUIDED_ONE ? (int32_t)GUIDED_ONE : (int32_t)r;
    if (r != r) v = (int32_t)(GUIDED_ONE / 2);   // (inf * 0)
  }
  if (lane == 0) a.values[i] = v;
}
