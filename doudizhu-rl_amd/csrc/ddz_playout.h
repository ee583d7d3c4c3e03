// ddz_playout.h -- k_playout / k_playout_choose: win counts of uniformly random playouts for every legal move of every
// running table ("playout spec v1"; the reference's Monte-Carlo player: server/mcts/interface.py:15-45 with
// default_policy.py:4-10 and the reward of tree.py:71-81, as flat Monte Carlo over perfect information).
// Included by ddz_engine.hip behind ddz_ply.h, inside its anonymous namespace.  The entry into a table (table_enter,
// root_hands), the hidden-hand domain, the redeal and every piece of a ply (ply_list, ply_entry, ply_apply, ply_draw) are
// ddz_ply.h's, shared with k_search, k_cfr and k_solve; this header holds the playout loop with its probe pass, and the choice.
//
// One wavefront per WORK ITEM (table t, chunk c).  With n = the size of t's legal list and K playouts per move, the n * K
// playouts of a table are numbered w = j * K + k (move index j, playout number k); chunk c of `chunks` runs w = c, c + chunks,
// c + 2 chunks, ...: a table with a long list is spread over its chunks whatever K is, and no playout depends on the split (its
// draws are keyed by (gid, k, j, ply) alone).  n is found by the wave itself -- the first pass of the playout loop stops behind
// the list of the root (`probe`) -- so nothing is read back by the host.
//
// The wave decodes the 176-byte root once and keeps what a playout needs of it as wave-uniform values: the three hands as nibble
// words in turn order, the combo to beat with the passes since, the role and the ply.  A playout copies those seven values, and
// every ply of it is: the closed-form round's legal lanes as a mask (never emitted: a playout needs the list's SIZE and its
// idx-th ENTRY only), the planner's tail into the LDS staging list where the rank masks allow one, the pick -- index j on the
// first ply, (draw * A) >> 32 afterwards -- from the round by lane number or from the staged tail, and the apply on the packed
// hands.  No list is stored; global traffic is the root read, one atomicAdd per (item, move) with wins and three for the totals.
// The playout loop is a counted `for` over DDZ_PLAYOUT_MAX_PLIES: no state, however inconsistent, makes a wavefront spin.
//
// k_playout<true> is "playout spec v2 (hidden hands)", DESIGN.md 4: the two opponents' count bytes are never read.  The wave
// decodes once what the actor has not seen (deck - own hand - taken) as a 54-lane pool mask and the opponents' hand SIZES, checks
// the domain once (status bit 6 and nothing runs outside it), and redeals at the top of a playout whose playout number k differs
// from the one before: lane c draws the key of card c (RNG domain 5, keyed by (gid, k) alone: every root move of a table sees the
// same K worlds), the pool is ranked by (key, c) through LDS as deal_wave_lds ranks a deal -- the wave's staging list is dead
// between two playouts, its first 64 words hold the keys -- and two ballots give the hands (unseen_pool and redeal_wave of
// ddz_ply.h).  The ply loop is the open one; everything of the hidden form stands under `if constexpr (HIDDEN)`.
struct PlayoutArgs {   // PlyArgs' six fields by name, not as a base: derived, the ply loop was 0.8 % slower (profiles/r18_notes.md 3)
  const uint8_t* state;
  int64_t T;
  uint32_t k0, k1;          // Philox key: (seed_lo ^ salt, seed_hi)
  uint64_t gid_base;
  uint32_t K;               // playouts per root move, 1 .. 2^23 - 1
  uint32_t chunks;          // work items per table
  int64_t stride;           // wins is [T][stride]
  int32_t* wins;
  unsigned long long* totals;  // {moves applied, playouts run, playouts stopped unfinished, -} or null
  int32_t* status;
  uint32_t roles;           // bit r: tables whose actor is role r take part (the others are idle); 7 in the open form
  // hidden form only
  uint8_t* worlds;          // null, or [T][K][2][16]: the worlds alone (ddz_playout_worlds), no playout runs
};

constexpr int PLAYOUT_WAVES = 12;  // 74 KB of LDS per block: two blocks per CU = 6 waves per SIMD (as k_rollout's dense variants)

template <bool HIDDEN>
__global__ __launch_bounds__(PLAYOUT_WAVES * 64, 6) void k_playout(PlayoutArgs a) {
  __shared__ HotTabT<false> hot;
  __shared__ uint64_t s_stage[PLAYOUT_WAVES][STAGE_CAP];
  __shared__ uint16_t s_svl[PLAYOUT_WAVES][STAGE_CAP];
  const int lane = threadIdx.x & 63;
  const int wv = (int)rfl(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * PLAYOUT_WAVES + wv;
  const int64_t t = item / a.chunks;
  const uint32_t chunk = (uint32_t)(item - t * a.chunks);
  uint4 R;
  if (!table_enter<PLAYOUT_WAVES>(a, t, lane, hot, R)) return;
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  // the decode and the `roles` gate, in both forms.  (What root_hands<false> derives from the opponents' hand rows -- hn0, hp0,
  // n_next, n_prev -- the hidden instance discards unread: the compiler drops those reads, the count bytes are never read.)
  const RootHands rh = root_hands<false>(R, a.roles, lane);
  if (rh.kind == ROOT_IDLE) return;   // not dealt, done, or not this call's seat: nothing runs, wins stay as they are
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const uint64_t hn0 = HIDDEN ? 0 : rh.hn0, hp0 = HIDDEN ? 0 : rh.hp0;
  const uint64_t gid = a.gid_base + (uint64_t)t;
  bool pool = false;
  int n_next = 0, n_prev = 0;
  uint32_t world_k = 0xFFFFFFFFu;   // the playout number the world below was dealt for (K < 2^23: none yet)
  uint64_t wn = 0, wp = 0;
  if constexpr (HIDDEN) {   // the pool of unseen cards and the opponents' hand sizes, the domain checked once -- called here, not
    uint64_t unseen;        // through root_hands<true>: so built, the hidden rows ran 0.3 .. 0.6 % slower (profiles/r18_notes.md 3)
    if (!unseen_pool(root, lane, n_next, n_prev, unseen, pool)) {   // outside the domain: nothing runs, wins stay as they are
      if (lane == 0 && chunk == 0) atomicOr(a.status, DDZ_ST_DOMAIN);
      return;
    }
    if (a.worlds) {   // ddz_playout_worlds: row 0 = the next player's counts and size, row 1 = the previous player's
      for (uint32_t k = chunk; k < a.K; k += a.chunks) {
        redeal_wave(gid, k, a.k0, a.k1, lane, pool, n_next, stage, wn, wp);
        const uint64_t h = lane < 16 ? wn : wp;
        const int b = lane & 15;
        const uint32_t v = b < 15 ? (uint32_t)((h >> (4 * b)) & 15) : (uint32_t)(lane < 16 ? n_next : n_prev);
        if (lane < 32) a.worlds[(((int64_t)t * a.K + k) << 5) + lane] = (uint8_t)v;
      }
      return;
    }
  }
  int32_t* const wins = a.wins + t * a.stride;
  uint64_t total = 0;          // n * K, known behind the probe
  uint64_t w = chunk;          // the next playout of this item
  bool probe = true;
  int cur_j = -1, win_j = 0;   // wins of the move this item is at: one atomicAdd when it moves on
  unsigned long long s_moves = 0;
  uint32_t s_playouts = 0, s_unfinished = 0;
  for (;;) {
    uint32_t j = 0, k = 0;
    if (!probe) {
      if (w >= total) break;
      j = (uint32_t)w / a.K;   // (n * K < 512 * 2^23: 32 bits hold w below total)
      k = (uint32_t)w - j * a.K;
      w += a.chunks;
      if ((int)j != cur_j) {
        if (win_j > 0 && lane == 0) atomicAdd(wins + cur_j, win_j);
        cur_j = (int)j;
        win_j = 0;
      }
    }
    // a private copy of the root
    uint64_t hc = root.hc0, hn = hn0, hp = hp0;
    if constexpr (HIDDEN) {
      if (!probe) {   // (the probe sizes the root's list: the actor's hand alone)
        if (k != world_k) {   // (an item whose chunks divide by K stays with one world)
          redeal_wave(gid, k, a.k0, a.k1, lane, pool, n_next, stage, wn, wp);
          world_k = k;
        }
        hn = wn; hp = wp;
      }
    }
    uint32_t trick = root.trick0, ply = root.ply0;
    int passes = root.passes0, role = role0;
    uint32_t draws = 0, dnext = 64;  // lane l holds the draw of the ply l behind the last refill; 64 = refill
    int winner = -1;
    // the ply loop's place in the 64-byte instruction lines is fixed here, so that code in front of it (the root decode) cannot
    // move it: the same loop measured 2.5 % faster to 1.5 % slower than the parent's by its start's offset alone (44: the
    // fastest open form; 32: the hidden form within the parent's spread; 20 and 4: slower; profiles/r15_notes.md 3)
    asm volatile(".p2align 6\n\t.rept %0\n\ts_nop 0\n\t.endr" ::"n"(HIDDEN ? 7 : 10));
    for (int s = 0; s < DDZ_PLAYOUT_MAX_PLIES; ++s) {
      uint32_t draw = 0;
      if (s > 0) {  // (the first move is the pick at index j: no draw)
        uint32_t dn = rfl(dnext);
        if (dn >= 64u) {   // domain 4, keyed by (gid, k, j, ply)
          dn = 0;
          dnext = 0;
          uint32_t qk0 = a.k0, qk1 = a.k1;
          asm volatile("" : "+s"(qk0), "+s"(qk1));   // the key stays in SGPRs (profiles/r15_notes.md: 21 more spills without)
          draws = ply_draw(gid, (k << 9) | j, RNG_PLAYOUT, ply, lane, qk0, qk1);
        }
        draw = rl(draws, (int)dn);
      }
      const uint32_t info = ply_info(trick, passes);
      uint64_t okm;
      int n0;
      int n = ply_list(hc, info, hot, lane, stage, svl, okm, n0);
      if (n > STAGE_CAP || n > a.stride) {  // cannot happen for a <= 20-card hand: the table (or this playout) runs nothing
        if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
        n = 0;
      }
      if (probe) {
        total = (uint64_t)n * a.K;
        break;
      }
      if (n <= 0) break;  // stopped unfinished
      const int idx = s == 0 ? (int)j : (int)rfl(__umulhi(draw, (uint32_t)n));  // random.choice(actions), envi.py:83
      uint64_t snib;
      uint32_t scat, svlv;
      ply_entry(okm, n0, idx, info, stage, svl, snib, scat, svlv);
      s_moves += 1;
      dnext += 1;
      if (ply_apply(snib, scat, svlv, hc, hn, hp, trick, passes, role, ply)) {
        winner = role;
        break;
      }
    }
    if (probe) {
      probe = false;
      continue;
    }
    s_playouts += 1;
    if (winner < 0) s_unfinished += 1;
    else if (same_side(winner, role0)) win_j += 1;
  }
  if (lane == 0) {
    if (win_j > 0) atomicAdd(wins + cur_j, win_j);
    if (a.totals && s_playouts) {
      atomicAdd(a.totals + 0, s_moves);
      atomicAdd(a.totals + 1, (unsigned long long)s_playouts);
      if (s_unfinished) atomicAdd(a.totals + 2, (unsigned long long)s_unfinished);
    }
  }
}

// ddz_playout_choose: the canonical id of the first maximum of wins[t][0 .. counts[t]) (torch.argmax's tie rule, dqn.py:60), -1
// for an empty list.  One wavefront per table over the live entries only.
__global__ __launch_bounds__(BLOCK) void k_playout_choose(const int32_t* __restrict__ counts, const int32_t* __restrict__ ids,
                                                          int64_t stride, const int32_t* __restrict__ wins,
                                                          int32_t* __restrict__ choice, int64_t T) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (t >= T) return;   // (whole waves: the reductions below run with every lane active)
  int64_t c = counts[t];
  if (c > stride) c = stride;
  if (c <= 0) {
    if (lane == 0) choice[t] = -1;
    return;
  }
  const int32_t* wt = wins + t * stride;
  int best = (int)0x80000000;
  uint32_t at = 0xFFFFFFFFu;
  for (int64_t j = lane; j < c; j += 64) {   // ascending j per lane: `>` keeps the lane's first maximum
    const int v = wt[j];
    if (at == 0xFFFFFFFFu || v > best) { best = v; at = (uint32_t)j; }
  }
  const int m = wave_max_i32(at == 0xFFFFFFFFu ? (int)0x80000000 : best);
  const uint32_t first = wave_min_u32((at != 0xFFFFFFFFu && best == m) ? at : 0xFFFFFFFFu);
  if (lane == 0) choice[t] = ids[t * stride + first];
}
