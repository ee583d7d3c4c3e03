// ddz_gismcts.h -- k_gismcts: information-set MCTS with leaf values from outside the kernel ("search spec v4 (guided ISMCTS)",
// DESIGN.md 4).  Included by ddz_engine.hip behind ddz_ismcts.h and ddz_guided.h, inside its anonymous namespace.  Spec v2's
// tree (a node is (parent, the move into it) with V, W and the availability count A), its hash table (ismcts_find /
// ismcts_insert), its list in lanes (ismcts_lane_entry), pass 1, the expansion ranking and the selection (ismcts_pass1 /
// ismcts_untried / ismcts_select), a new node's record (ismcts_make_node), the selection step (ismcts_descend) and the root's
// children leaving (ismcts_root_out) are ddz_ismcts.h's; spec v3's phases, unit (W in 1024ths, search_value<1024>), header
// words (GH_*), GuidedArgs and the phased scaffold -- the view of a tree, OPEN, the check of a header, the pending leaf's score
// and path, the rows a descent carries with the leaf's row, the header store and the outputs (guided_tree, guided_open,
// guided_header_live, guided_pending_score, DescentRows, guided_leave_pending, guided_store_header, guided_emit) -- are
// ddz_guided.h's; the backup of a path and the totals (path_backup, search_totals_out) are ddz_search.h's; the entry into a
// table, the redeal, every piece of a ply and the wavefront-scope accesses are ddz_ply.h's.  This header holds their
// composition: the kernel below is its prologue, node 0, and the descent loop between those calls.
//
// One wavefront per WORK ITEM (table t, tree c), 12-wave blocks as k_search, always the hidden form.  Phases of a launch,
// wave-uniform, as k_guided's:
//   OPEN   the root's list is sized, the hash table and the header are zeroed, node 0 is written.  Nothing else.
//   STEP   a pending leaf is backed up with values[item]; then, if it < budget, iteration `it` on world c * budget + it of
//          playout spec v2, dealt by this launch (redeal_wave): k_ismcts's descent, every level enumerating the list of the
//          state in that world.  A new child that ends the game is scored and backed up at once; any other is left PENDING: its
//          176-byte state row (the opponents' hands are this world's) goes out with need = 1.  No playout, no playout draws.
//   CLOSE  a pending leaf is backed up with values[item]; the root's children (looked up by the root's own list, the same in
//          every world) and the totals leave.
// The backup stands ahead of the descent, so every count a descent reads is what the one-launch k_ismcts would read.
//
// WORKSPACE per (table, tree), gismcts_tree_bytes(budget), a function of the budget alone:
//   header [16] u32: 0 live, 1 iteration number, 2 node count, 3 pending node (SEARCH_NONE: none), 4 pending depth, 5 the leaf
//          actor is on the root actor's side, 6 unfinished, 7..9 zero, 10..11 moves applied
//   path   [SEARCH_PATH] u16, two to a word: the nodes of the pending iteration's descent, the root first, the new node last
//   nodes, table: spec v2's (ddz_ismcts.h).  A new node's record is whole when it is made (V = W = 0, A = 1): the backup, in
//          this launch or the next, counts it with its path.
// A table outside the hidden-hand domain raises status bit 6 and its workspace is never touched; an idle table's neither.  A
// launch that finds a header OPEN did not write, or one whose fields are out of range, runs nothing on that tree; a stored
// path names nodes of this tree whatever its words hold, a child found in the table is below the node count.
//
// LOOPS, MEMORY ORDERING: as ddz_guided.h.  Every loop is counted (the descent by DDZ_SEARCH_MAX_DEPTH, a probe by H, the trips
// by n <= STAGE_CAP); the iterations are the caller's launches; a wave waits for no other.  Kernel boundaries order the
// launches; inside one, tree, header and path are one wavefront's, through the relaxed wavefront-scope accesses and
// search_fence.  values is read, leaf_rows and need are written with plain vector accesses.  Atomics: the root sums, the
// totals, the status word.
inline uint64_t gismcts_tree_bytes(int64_t budget) { return GUIDED_HDR_BYTES + GUIDED_PATH_BYTES + ismcts_tree_bytes(budget); }

__global__ __launch_bounds__(SEARCH_WAVES * 64, 6) void k_gismcts(GuidedArgs a) {
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
  const RootHands rh = root_hands<true>(R, a.roles, lane);
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const GuidedTree g = guided_tree(a.work, item, a.tree_bytes, a.budget, INODE_BYTES);
  uint32_t* const hdr = g.hdr;
  uint8_t* const nodes = g.nodes;
  uint64_t* const tab = g.tab;
  const uint32_t hlog = a.hash_log;
  if (rh.kind == ROOT_OUTSIDE && lane == 0 && tree == 0) atomicOr(a.status, DDZ_ST_DOMAIN);   // outside the domain: nothing runs
  if (rh.kind == ROOT_INSIDE && a.phase == GUIDED_OPEN) {
    // ---- OPEN: the root actor's list is the same in every world
    const bool live = guided_open(g, a, root, hot, lane, stage, svl) > 0;
    if (live && lane < 4) sst64((uint64_t*)nodes + lane, lane == 2 ? (uint64_t)SEARCH_NONE << 32 : 0ull);   // node 0: no move, no parent
    guided_open_header(hdr, live, lane);
    return;
  }
  if (rh.kind == ROOT_INSIDE && guided_header_live(hdr, a.budget)) {
    uint32_t it = rfl(sld32(hdr + GH_IT)), nnodes = rfl(sld32(hdr + GH_NNODES));
    uint32_t s_unfinished = rfl(sld32(hdr + GH_UNFINISHED));
    unsigned long long s_moves = rfl64(sld64((const uint64_t*)(hdr + GH_MOVES)));
    const uint32_t pending = rfl(sld32(hdr + GH_PENDING));
    if (pending != SEARCH_NONE) {
      // ---- the pending leaf is backed up with its path (its record is whole since it was made)
      int pdepth;
      const uint32_t score = guided_pending_score(g, a.values, item, nnodes, path, lane, pdepth);
      path_backup<INODE_BYTES>(nodes, path, pdepth, score, lane);
      search_fence();
    }
    uint32_t made = SEARCH_NONE;   // the node this launch creates and, where it is not terminal, leaves pending
    bool wait = false;
    int depth = 0;
    uint32_t pside = 0;
    if (a.phase == GUIDED_STEP && it < a.budget) {
      // this iteration's world: k = c * budget + i of playout spec v2 (the staging list serves as the redeal's keys)
      const uint64_t gid = a.gid_base + (uint64_t)t;
      uint64_t hc = root.hc0, hn, hp;
      redeal_wave(gid, tree * a.budget + it, a.k0, a.k1, lane, rh.pool, rh.n_next, stage, hn, hp);
      uint32_t trick = root.trick0, ply = root.ply0;
      int passes = root.passes0, role = role0;
      DescentRows rows = {root.P, root.aux};   // (the cards left of a hand row are the same in every world)
      const auto track = [&](uint64_t snib, uint32_t scat) { rows.track(snib, scat, role, lane); };   // (the mover: before the turn)
      uint32_t node = 0;
      int winner = -1;
      if (lane == 0) path[0] = 0;
      for (int d = 0; d <= DDZ_SEARCH_MAX_DEPTH; ++d) {
        const uint32_t meta = rfl(sld32((const uint32_t*)(nodes + (uint64_t)node * INODE_BYTES + 24)));
        if ((meta >> 26) & 1u) {   // a terminal node reached by selection: scored at once
          winner = (int)((meta >> 27) & 3u);
          break;
        }
        if (d == DDZ_SEARCH_MAX_DEPTH) break;   // score 0, unfinished
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
        // ---- pass 1: spec v2's, W in 1024ths
        const bool sides = a.mode == (uint32_t)DDZ_SEARCH_SIDES;
        const bool own = sides ? same_side(role, role0) : (role == role0);
        uint32_t best, at, bchild;
        const uint32_t untried = ismcts_pass1<GUIDED_ONE>(nodes, tab, hlog, nnodes, node, trips, okm, n0, n, info, stage, lane, a.ln,
                                                          a.c, own, sides, best, at, bchild);
        if (untried > 0) {
          // ---- expansion: spec v2's draw and pick
          const uint32_t de = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), (tree << 16) | it, RNG_EXPAND << 16), a.k0, a.k1).x;
          const int idx = ismcts_untried(nodes, tab, hlog, nnodes, node, trips, okm, n0, n, info, stage, lane, untried,
                                         rfl(__umulhi(de, untried)));
          if (idx < 0 || idx >= n) break;   // (cannot happen: `untried` entries without a child exist)
          uint64_t snib; uint32_t scat, svlv;
          ply_entry(okm, n0, idx, info, stage, svl, snib, scat, svlv);
          made = nnodes++;
          s_moves += 1;
          const int mover = role;
          track(snib, scat);
          const bool over = ply_apply(snib, scat, svlv, hc, hn, hp, trick, passes, role, ply);
          ismcts_make_node(nodes, tab, hlog, node, made, snib, scat, over, mover, path, depth, lane);
          depth += 1;
          if (over) winner = mover;
          else {   // ---- a pending leaf: its value is the caller's (its list is not enumerated: a node keeps no n)
            pside = same_side(role, role0) ? 1u : 0u;
            wait = true;
          }
          break;
        }
        // ---- selection among the children whose moves are in this world's list: spec v2's
        uint32_t child;
        const uint32_t first = ismcts_select(own || sides, best, at, bchild, child);
        if (first == SEARCH_NONE) break;   // (cannot happen: every child was backed up before this descent)
        uint64_t snib; uint32_t scat, svlv;
        ply_entry(okm, n0, (int)first, info, stage, svl, snib, scat, svlv);
        s_moves += 1;
        track(snib, scat);
        ismcts_descend(snib, scat, svlv, child, hc, hn, hp, trick, passes, ply, role, path, depth, lane);
        node = child;
      }
      it += 1;
      search_fence();   // the path, the new record and the raised A's are written
      if (wait) {
        Rleaf = rows.leaf_row(hc, hn, hp, role, ply, my, mz, mw, lane);
        needs = 1;
        guided_leave_pending(g.gpath, path, depth, lane);
      } else {
        const uint32_t score = (winner >= 0 && same_side(winner, role0)) ? GUIDED_ONE : 0u;
        if (winner < 0) s_unfinished += 1;
        path_backup<INODE_BYTES>(nodes, path, depth, score, lane);
      }
    }
    guided_store_header(hdr, it, nnodes, wait ? made : SEARCH_NONE, depth, pside, s_unfinished, s_moves, lane);
    search_fence();
    if (a.phase == GUIDED_CLOSE) {
      // ---- the root's children leave: visits / wins += V / W (1024ths) at their index of the root's list
      const uint32_t info = ply_info(root.trick0, root.passes0);
      uint64_t okm; int n0;
      const int n = ply_list(root.hc0, info, hot, lane, stage, svl, okm, n0);
      __builtin_amdgcn_wave_barrier();
      if (n > 0 && n <= STAGE_CAP) ismcts_root_out(a, t, nodes, tab, nnodes, okm, n0, n, info, stage, a.stride, lane);
      search_totals_out(a.totals, s_moves, it, s_unfinished, nnodes, lane);
    }
  }
  guided_emit(a, item, Rleaf, needs, lane);
}
