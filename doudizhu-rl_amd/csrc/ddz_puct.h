// ddz_puct.h -- k_puct / k_puct_priors: guided UCT with move priors ("search spec v5 (guided PUCT)").  Included by
// ddz_engine.hip behind ddz_guided.h, inside its anonymous namespace.  Spec v3's phases, unit (W in 1024ths), header words (GH_*),
// GuidedArgs and the phased scaffold (guided_tree, guided_open, guided_open_header, guided_header_live, guided_pending_score,
// DescentRows, guided_leave_pending, guided_store_header, guided_emit) are ddz_guided.h's; the hash table, the backup of a path and
// the totals (search_find / search_insert, path_backup, search_totals_out) are ddz_search.h's; the entry into a table, the redeal,
// every piece of a ply and the wavefront-scope accesses are ddz_ply.h's.  This header holds what v5 changes: every evaluated node
// keeps a PRIOR WEIGHT (u8) for each index of its list, the descent selects over ALL indices of a node, visited or not, by the
// PUCT rule, and nothing is expanded at random: no draw of any RNG domain but the redeal's.
//
// One wavefront per WORK ITEM (table t, tree c), 12-wave blocks as k_guided.  Only DDZ_SEARCH_SIDES: a node's actor maximises
// its own side's mean.  Phases of a launch, wave-uniform:
//   OPEN   the root's list is sized, the hash table and the header are zeroed, node 0 is written.  Nothing else.
//   STEP   a pending node is backed up with values[item] and priors[item]; then, if it < budget, one iteration.  Iteration 0
//          descends nowhere: it leaves node 0 PENDING with the root's row (hidden: on the tree's world) and need = 1, so the
//          root has its priors before the first selection and `budget` iterations grow at most budget - 1 nodes below it.
//   CLOSE  a pending node is backed up; the root's children and the totals (five of them) leave.
//
// WORKSPACE per (table, tree), puct_tree_bytes(budget, pool), a function of the two alone:
//   header [16] u32: spec v3's words 0..11; 12 pool bytes used, 13 nodes that fell back to uniform priors
//   path   [SEARCH_PATH] u16, two to a word
//   nodes  [budget + 1] x 32 bytes: spec v1's 24 | prior-pool offset u32 (SEARCH_NONE: no stored priors) | weight sum S u32
//   table  spec v1's
//   pool   [pool] bytes: the run of a node with list size n is n bytes, one weight per list index in the order of ply_list, at the
//          next multiple of 4 (PUCT_RUN_ALIGN) in the order the nodes are backed up = created; a run the pool has no room for is
//          not stored: offset SEARCH_NONE, word 13 += 1.  A terminal node and a node with n = 0 take no run and are not counted.
// A node without a run, or with S = 0, is UNIFORM: p_j = 1 / n.
//
// SELECTION at a node with n > 0 entries, N = its V >= 1 (it was evaluated), over every list index j (a lane each, rounds of 64),
// single fp32 operations, nothing fused:
//   mean_j = ((float)Wside_j / (float)V_j) * 2^-10 where child j exists (V_j > 0), else the node's own ((float)Wside / (float)N) *
//            2^-10; Wside = W where the node's actor is on the root actor's side, else V * 1024 - W
//   p_j = (float)w_j / (float)S, or 1.0f / (float)n at a uniform node
//   value_j = mean_j + ((c * p_j) * sqrtf((float)N)) / (float)(1 + V_j);   the maximum, ties to the lowest index.
// The selected index has a child: go to it.  It has none: EXPAND it (the node's list is enumerated for the entry); a move that
// empties a hand makes a terminal child, scored at once; any other child is left pending as spec v3 leaves a leaf.
//
// BOUNDS.  puct_header_live adds "pool bytes used <= pool, a multiple of 4" to guided_header_live; an offset read from a
// record is used only where offset + the run fits the pool (else the node is uniform); a child found in the table is below the
// node count.  With these every index a STEP or a CLOSE computes stays inside the tree and the pool whatever the bytes hold.
// An idle, masked or out-of-domain item touches no byte of its workspace.
//
// LOOPS, MEMORY ORDERING: as ddz_guided.h.  Every loop is counted (the descent by DDZ_SEARCH_MAX_DEPTH, a probe by H, the rounds
// by n <= STAGE_CAP, a run by 1024 bytes); a wave waits for no other.  Tree, header, path and pool are one wavefront's, through
// the relaxed wavefront-scope accesses and search_fence.  values and priors are read, leaf_rows and need are written with
// plain vector accesses.  Atomics: the root sums, the totals, the status word.
constexpr uint32_t PNODE_BYTES = 32;
constexpr uint32_t PUCT_RUN_ALIGN = 4;
constexpr int64_t PUCT_POOL_MAX = 1 << 24;
enum { GH_POOL_USED = 12, GH_FALLBACK = 13 };

struct PuctArgs : GuidedArgs {
  const uint8_t* priors;   // [T * trees][stride] or null (the first step)
  uint32_t pool;           // bytes of a tree's prior pool
};

inline uint64_t puct_tree_bytes(int64_t budget, int64_t pool) {
  return GUIDED_HDR_BYTES + GUIDED_PATH_BYTES + (uint64_t)(budget + 1) * PNODE_BYTES + (8ull << search_hash_log(budget)) + (uint64_t)pool;
}

__device__ __forceinline__ uint32_t puct_run_bytes(uint32_t n) { return (n + PUCT_RUN_ALIGN - 1u) & ~(PUCT_RUN_ALIGN - 1u); }

__device__ __forceinline__ bool puct_header_live(const uint32_t* hdr, uint32_t budget, uint32_t pool) {
  if (!guided_header_live(hdr, budget)) return false;
  const uint32_t used = rfl(sld32(hdr + GH_POOL_USED));
  return used <= pool && (used & (PUCT_RUN_ALIGN - 1u)) == 0u;
}

// the pending node's value and priors arrive: path_backup on path[0 .. pdepth]; a node below the root is not on its own path and
// gets its record written whole (V = 1, W = score), the root (pending = 0, path = {0}) was counted with the path; then the
// node's n weights go into the pool and (offset, S) into its record.  used / fallback: header words 12 / 13, kept by the caller.
__device__ __forceinline__ void puct_backup(uint8_t* nodes, uint8_t* pool, const PuctArgs& a, int64_t item, const uint16_t* path,
                                            int pdepth, uint32_t score, uint32_t pending, uint64_t move, uint32_t meta,
                                            uint32_t& used, uint32_t& fallback, int lane) {
  path_backup<PNODE_BYTES>(nodes, path, pdepth, score, lane);
  uint32_t n = (meta >> 16) & 0x3FFu;
  if ((int64_t)n > a.stride) n = (uint32_t)a.stride;
  uint32_t off = SEARCH_NONE, S = 0;
  if (n > 0) {
    const uint32_t run = puct_run_bytes(n);
    if (run <= a.pool - used) {   // (used <= pool: puct_header_live)
      off = used;
      used += run;
      const uint8_t* pr = a.priors ? a.priors + (uint64_t)item * (uint64_t)a.stride : nullptr;
      int sum = 0;
      for (uint32_t b = 0; b < run; b += 256u) {   // a lane packs four weights to a word; entries at or beyond n are not read
        const uint32_t j = b + 4u * (uint32_t)lane;
        if (j < run) {
          uint32_t word = 0;
          for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t w = (pr && j + k < n) ? (uint32_t)pr[j + k] : 0u;
            word |= w << (8u * k);
            sum += (int)w;
          }
          sst32((uint32_t*)(pool + off + j), word);
        }
      }
      S = (uint32_t)wave_sum_i32(sum);
    } else {
      fallback += 1;
    }
  }
  if (lane == 0) {
    uint8_t* q = nodes + (uint64_t)pending * PNODE_BYTES;
    if (pending != 0u) {
      sst64((uint64_t*)q, move);
      sst64((uint64_t*)(q + 8), 1ull | ((uint64_t)score << 32));
      sst64((uint64_t*)(q + 16), (uint64_t)meta);   // (children created: 0)
    }
    sst64((uint64_t*)(q + 24), (uint64_t)off | ((uint64_t)S << 32));
  }
}

// selection over all n list indices of `node` (SELECTION above) -> the list index, wave-uniform; child: the node behind it,
// SEARCH_NONE where none was created.  own: the node's actor is on the root actor's side.
__device__ __forceinline__ uint32_t puct_select(const uint8_t* nodes, const uint64_t* tab, uint32_t hlog, const uint8_t* pool,
                                                uint32_t pool_bytes, uint32_t node, int n, uint32_t nnodes, float c, bool own, int lane,
                                                uint32_t& child) {
#pragma clang fp contract(off)
  const uint8_t* nr = nodes + (uint64_t)node * PNODE_BYTES;
  const uint64_t vw0 = rfl64(sld64((const uint64_t*)(nr + 8))), os = rfl64(sld64((const uint64_t*)(nr + 24)));
  const uint32_t N = (uint32_t)vw0, W0 = (uint32_t)(vw0 >> 32), off = (uint32_t)os, S = (uint32_t)(os >> 32);
  const bool weighted = off != SEARCH_NONE && S > 0u && (off & (PUCT_RUN_ALIGN - 1u)) == 0u && off <= pool_bytes &&
                        puct_run_bytes((uint32_t)n) <= pool_bytes - off;
  const float fN = (float)N, fS = (float)S;
  const float mean0 = ((float)(own ? W0 : N * GUIDED_ONE - W0) / fN) * (1.0f / (float)GUIDED_ONE);
  const float root_n = __builtin_sqrtf(fN);
  const float uniform = 1.0f / (float)n;
  uint32_t best = 0, at = SEARCH_NONE, bchild = SEARCH_NONE;
  for (int b = 0; b < n; b += 64) {
    const int j = b + lane;
    if (j < n) {
      uint32_t ch = search_find(tab, hlog, node * 512u + (uint32_t)j + 1u);
      uint32_t V = 0, W = 0;
      if (ch != SEARCH_NONE && ch < nnodes) {
        const uint64_t vw = sld64((const uint64_t*)(nodes + (uint64_t)ch * PNODE_BYTES + 8));
        V = (uint32_t)vw;
        W = (uint32_t)(vw >> 32);
      } else {
        ch = SEARCH_NONE;
      }
      float mean = mean0;
      if (V > 0u) mean = ((float)(own ? W : V * GUIDED_ONE - W) / (float)V) * (1.0f / (float)GUIDED_ONE);
      float p = uniform;
      if (weighted) {
        const uint32_t word = sld32((const uint32_t*)(pool + off + ((uint32_t)j & ~3u)));
        p = (float)((word >> (8u * ((uint32_t)j & 3u))) & 0xFFu) / fS;
      }
      const float cp = c * p;
      const float num = cp * root_n;
      const float u = num / (float)(1u + V);
      const uint32_t bits = __float_as_uint(mean + u);   // (values are non-negative floats: their bit patterns order as they do)
      if (at == SEARCH_NONE || bits > best) { best = bits; at = (uint32_t)j; bchild = ch; }
    }
  }
  const uint32_t m = (uint32_t)wave_max_i32(at == SEARCH_NONE ? (int)0x80000000 : (int)best);
  const uint32_t first = wave_min_u32((at != SEARCH_NONE && best == m) ? at : SEARCH_NONE);   // ties: the lowest index
  child = first == SEARCH_NONE ? SEARCH_NONE : rl(bchild, (int)(first & 63u));
  return first;
}

template <bool HIDDEN>
__global__ __launch_bounds__(SEARCH_WAVES * 64, 6) void k_puct(PuctArgs a) {
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
  // what a STEP leaves of an item without a pending node: a row with dealt = 0 (a leaf environment freezes it), need 0
  uint4 Rleaf = make_uint4(0, 0, 0, 0);
  int32_t needs = 0;
  const RootHands rh = root_hands<HIDDEN>(R, a.roles, lane);
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const GuidedTree g = guided_tree(a.work, item, a.tree_bytes, a.budget, PNODE_BYTES);
  uint32_t* const hdr = g.hdr;
  uint8_t* const nodes = g.nodes;
  uint64_t* const tab = g.tab;
  const uint32_t hlog = a.hash_log;
  uint8_t* const pool = (uint8_t*)(tab + (1ull << hlog));
  if (rh.kind == ROOT_OUTSIDE && lane == 0 && tree == 0) atomicOr(a.status, DDZ_ST_DOMAIN);   // outside the domain: nothing runs
  if (rh.kind == ROOT_INSIDE && a.phase == GUIDED_OPEN) {
    // ---- OPEN: the root's list is node 0's n; node 0 has no move, no visit, no priors yet
    const int n_root = guided_open(g, a, root, hot, lane, stage, svl);
    if (n_root > 0 && lane < 4)
      sst64((uint64_t*)nodes + lane, lane == 2 ? (uint64_t)((uint32_t)n_root << 16) : lane == 3 ? (uint64_t)SEARCH_NONE : 0ull);
    guided_open_header(hdr, n_root > 0, lane);
    return;
  }
  if (rh.kind == ROOT_INSIDE && puct_header_live(hdr, a.budget, a.pool)) {
    uint32_t it = rfl(sld32(hdr + GH_IT)), nnodes = rfl(sld32(hdr + GH_NNODES));
    uint32_t s_unfinished = rfl(sld32(hdr + GH_UNFINISHED));
    uint32_t used = rfl(sld32(hdr + GH_POOL_USED)), fallback = rfl(sld32(hdr + GH_FALLBACK));
    unsigned long long s_moves = rfl64(sld64((const uint64_t*)(hdr + GH_MOVES)));
    const uint32_t pending = rfl(sld32(hdr + GH_PENDING));
    if (pending != SEARCH_NONE) {
      // ---- the pending node is backed up, its priors stored
      int pdepth;
      const uint32_t score = guided_pending_score(g, a.values, item, nnodes, path, lane, pdepth);
      puct_backup(nodes, pool, a, item, path, pdepth, score, pending, rfl64(sld64((const uint64_t*)(hdr + GH_PMOVE))),
                  rfl(sld32(hdr + GH_PMETA)), used, fallback, lane);
      search_fence();
    }
    uint32_t made = SEARCH_NONE;   // the node this launch creates (iteration 0: the root itself) and, where it is not terminal, leaves pending
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
      if (it == 0) {
        // ---- iteration 0 evaluates the root: node 0 pending with the root's own row
        made = 0;
        made_meta = rfl(sld32((const uint32_t*)(nodes + 16))) & (0x3FFu << 16);
        pside = 1u;
        wait = true;
      }
      for (int d = 0; d <= DDZ_SEARCH_MAX_DEPTH && it != 0; ++d) {
        const uint8_t* nr = nodes + (uint64_t)node * PNODE_BYTES;
        const uint32_t meta = rfl(sld32((const uint32_t*)(nr + 16)));
        if ((meta >> 26) & 1u) {   // a terminal node reached by selection: scored at once
          winner = (int)((meta >> 27) & 3u);
          break;
        }
        const int n = (int)((meta >> 16) & 0x3FFu);
        if (n <= 0 || d == DDZ_SEARCH_MAX_DEPTH) break;   // outside the domain: score 0, unfinished
        const uint32_t info = ply_info(trick, passes);
        uint32_t child;
        const uint32_t first = puct_select(nodes, tab, hlog, pool, a.pool, node, n, nnodes, a.c, same_side(role, role0), lane, child);
        if (first == SEARCH_NONE) break;   // (cannot happen: n > 0)
        if (child == SEARCH_NONE) {
          // ---- expansion of the selected index: the node's list is enumerated for its entry
          uint64_t okm; int n0;
          const int nn = ply_list(hc, info, hot, lane, stage, svl, okm, n0);
          if (nn != n) break;   // (cannot happen: the state of a node is a function of its path)
          uint64_t snib; uint32_t scat, svlv;
          ply_entry(okm, n0, (int)first, info, stage, svl, snib, scat, svlv);
          made = nnodes++;
          made_move = snib | ((uint64_t)scat << 60);
          made_meta = svlv & 0xFFFFu;
          if (lane == 0) {
            search_insert(tab, hlog, node * 512u + first + 1u, made);
            uint32_t* created = (uint32_t*)(nodes + (uint64_t)node * PNODE_BYTES + 20);
            sst32(created, sld32(created) + 1u);
          }
          s_moves += 1;
          track(snib, scat);
          if (ply_apply(snib, scat, svlv, hc, hn, hp, trick, passes, role, ply)) {
            winner = role;
            made_meta |= (1u << 26) | ((uint32_t)role << 27);
            break;
          }
          // ---- a pending leaf: its n is the size of its state's list, its value and priors are the caller's
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
        // ---- the selected index has a child: its stored move is re-applied
        const uint8_t* cr = nodes + (uint64_t)child * PNODE_BYTES;
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
        path_backup<PNODE_BYTES>(nodes, path, depth, score, lane);
        if (made != SEARCH_NONE && lane == 0) {   // a terminal child: its record written whole, no priors
          uint8_t* q = nodes + (uint64_t)made * PNODE_BYTES;
          sst64((uint64_t*)q, made_move);
          sst64((uint64_t*)(q + 8), 1ull | ((uint64_t)score << 32));
          sst64((uint64_t*)(q + 16), (uint64_t)made_meta);
          sst64((uint64_t*)(q + 24), (uint64_t)SEARCH_NONE);
        }
      }
    }
    guided_store_header(hdr, it, nnodes, wait ? made : SEARCH_NONE, depth, pside, s_unfinished, s_moves, lane);
    if (lane == 0) {   // the record puct_backup writes when the node's value is there; the pool's state
      sst32(hdr + GH_PMETA, made_meta);
      sst64((uint64_t*)(hdr + GH_PMOVE), made_move);
      sst32(hdr + GH_POOL_USED, used);
      sst32(hdr + GH_FALLBACK, fallback);
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
            const uint64_t vw = sld64((const uint64_t*)(nodes + (uint64_t)ch * PNODE_BYTES + 8));
            atomicAdd(a.visits + t * a.stride + j, (int32_t)(uint32_t)vw);
            if ((uint32_t)(vw >> 32)) atomicAdd(a.wins + t * a.stride + j, (int32_t)(uint32_t)(vw >> 32));
          }
        }
      }
      search_totals_out(a.totals, s_moves, it, s_unfinished, nnodes, lane);
      if (lane == 0 && a.totals && fallback) atomicAdd(a.totals + 4, (unsigned long long)fallback);
    }
  }
  guided_emit(a, item, Rleaf, needs, lane);
}

// k_puct_priors: prior weights from a q slab, beside k_guided_value.  One wavefront per leaf i with a running row whose actor's
// role is in net_roles: qmax = the maximum of q[i][0 .. n[i]), w_j = clamp((int)rintf(255 * expf(((q_j - qmax) * inv_reward[role])
// * inv_tau)), 0, 255) for j < n[i]; single fp32 operations, nothing fused, the library expf.  An entry equal to qmax gets 255
// (it would anyway: expf(0) = 1; said so that an infinite maximum gets it too); a NaN anywhere in the row gives all ones.  Every
// other row, and every entry at or beyond n[i], is left as it is.  Weights are not normalised: nothing is summed in fp32.
struct PuctPriorsArgs : GuidedValueArgs {
  float inv_tau;
  uint8_t* priors;   // [n_leaves][stride]
};

__global__ __launch_bounds__(BLOCK) void k_puct_priors(PuctPriorsArgs a) {
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
  const bool ones = __ballot(nan) != 0ull;
  const float inv = role == 0 ? a.inv_reward[0] : role == 1 ? a.inv_reward[1] : a.inv_reward[2];
  for (int64_t j = lane; j < n; j += 64) {
    const float x = a.q[i * a.stride + j];
    const float d = x - m;
    const float s = d * inv;
    const float e = expf(s * a.inv_tau);
    const float r = __builtin_rintf(255.0f * e);
    uint32_t w = r >= 255.0f ? 255u : r >= 1.0f ? (uint32_t)r : 0u;   // (a NaN compares false: 0)
    if (x == m) w = 255u;
    a.priors[i * a.stride + j] = (uint8_t)(ones ? 1u : w);
  }
}
