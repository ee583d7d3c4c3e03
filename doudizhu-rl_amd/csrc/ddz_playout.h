// ddz_playout.h -- k_playout / k_playout_choose: win counts of uniformly random playouts for every legal move of every
// running table ("playout spec v1"; the reference's Monte-Carlo player: server/mcts/interface.py:15-45 with
// default_policy.py:4-10 and the reward of tree.py:71-81, as flat Monte Carlo over perfect information).
// Included by ddz_engine.hip behind k_rollout, inside its anonymous namespace: built from the same device functions (the
// rank-mask tests, round_pre / round_src / round_entry, plan_scan_t<EM_STAGE> into the wave's LDS list, the packed apply).
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
// between two playouts, its first 64 words hold the keys -- and two ballots give the hands.  The ply loop is the open one.  The
// open instance is what it was: everything of the hidden form stands under `if constexpr (HIDDEN)`.
struct PlayoutArgs {
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
  // hidden form only
  uint32_t roles;           // bit r: tables whose actor is role r take part (the others are idle)
  uint8_t* worlds;          // null, or [T][K][2][16]: the worlds alone (ddz_playout_worlds), no playout runs
};

constexpr uint64_t DECK_NIB = 0x0114444444444444ull;  // four of the ranks 3 .. 2, one of each joker

constexpr int PLAYOUT_WAVES = 12;  // 74 KB of LDS per block: two blocks per CU = 6 waves per SIMD (as k_rollout's dense variants)

// world k of a table (playout spec v2): the hands of the next and of the previous player as nibble words.  `pool`: this lane's
// card (Deal v2's numbering) is unseen; keys: 64 x 8 bytes of the calling wave; 1 <= n_next.
__device__ inline void redeal_wave(uint64_t gid, uint32_t k, uint32_t k0, uint32_t k1, int lane, bool pool, int n_next,
                                   uint64_t* keys, uint64_t& o_next, uint64_t& o_prev) {
  const uint4 d = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), k, (5u << 16) | (uint32_t)(lane >> 2)), k0, k1);
  const int w = lane & 3;
  const uint32_t key = w == 0 ? d.x : w == 1 ? d.y : w == 2 ? d.z : d.w;
  const uint64_t kk = pool ? ((uint64_t)key << 6) | (uint32_t)lane : ~0ull;  // a card outside the pool ranks behind every pool card
  keys[lane] = kk;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  int pos = 0;
#pragma unroll 9
  for (int j = 0; j < 54; j += 2) {
    const ulonglong2 v = *(const ulonglong2*)&keys[j];
    pos += (v.x < kk ? 1 : 0) + (v.y < kk ? 1 : 0);
  }
  o_next = nib_from_cards(__ballot(pool && pos < n_next));
  o_prev = nib_from_cards(__ballot(pool && pos >= n_next));
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();   // the keys are read: the staging list is the ply loop's again
}

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
  uint4 R = make_uint4(0, 0, 0, 0);
  if (t < a.T && lane < DDZ_NFIELDS) R = ((const uint4*)(a.state + t * STATE_ROW_BYTES))[lane];
  hot_fill<PLAYOUT_WAVES * 64>(hot);
  __syncthreads();   // the block's only barrier: a wave may leave behind it
  if (t >= a.T) return;
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  // the root, decoded once (as k_rollout decodes a table): row f < 10 as 15 nibbles in lane f, the meta row's words as scalars
  const uint64_t P = pack_row(R);
  const uint32_t aux = R.w >> 24;
  const uint32_t mx = rl(R.x, DDZ_F_META), my = rl(R.y, DDZ_F_META);
  int role0 = mx & 0xFF;
  if (role0 > 2) role0 = 0;
  if (!(((my >> 16) & 0xFF) && !((mx >> 8) & 0xFF))) return;  // not dealt, or done: nothing runs, wins stay as they are
  const uint32_t ply0 = my & 0xFFFF;
  const uint64_t hc0 = rl64(P, DDZ_F_HAND0 + role0);
  uint64_t hn0 = 0, hp0 = 0;
  if constexpr (!HIDDEN) {
    hn0 = rl64(P, DDZ_F_HAND0 + (role0 == 2 ? 0 : role0 + 1));
    hp0 = rl64(P, DDZ_F_HAND0 + (role0 == 0 ? 2 : role0 - 1));
  }
  uint32_t trick0 = mk_info(EMPTY, 0, 1);  // the combo to beat (envi.py:103-109) as (trick, passes since it was played)
  int passes0 = 0;
  {
    const int rm1 = role0 == 0 ? 2 : role0 - 1, rp1 = role0 == 2 ? 0 : role0 + 1;
    const uint64_t n1 = rl64(P, DDZ_F_RECENT0 + rm1), n2 = rl64(P, DDZ_F_RECENT0 + rp1);
    if (n1) trick0 = info_of_row(n1, (int)rl(aux, DDZ_F_RECENT0 + rm1));
    else if (n2) { trick0 = info_of_row(n2, (int)rl(aux, DDZ_F_RECENT0 + rp1)); passes0 = 1; }
  }
  const uint64_t gid = a.gid_base + (uint64_t)t;
  // hidden form: the pool of unseen cards and the opponents' hand sizes, the domain checked once
  bool pool = false;
  int n_next = 0;
  uint32_t world_k = 0xFFFFFFFFu;   // the playout number the world below was dealt for (K < 2^23: none yet)
  uint64_t wn = 0, wp = 0;
  if constexpr (HIDDEN) {
    if (!((a.roles >> role0) & 1u)) return;   // not this call's seat: idle
    const uint64_t taken = rl64(P, DDZ_F_TAKEN);
    n_next = (int)rl(aux, DDZ_F_HAND0 + (role0 == 2 ? 0 : role0 + 1));
    const int n_prev = (int)rl(aux, DDZ_F_HAND0 + (role0 == 0 ? 2 : role0 - 1));
    const int sh = 4 * (lane & 15);
    const int deck = lane < 13 ? 4 : lane < 15 ? 1 : 0;
    const bool over = (int)((hc0 >> sh) & 15) + (int)((taken >> sh) & 15) > deck;   // unseen_r < 0
    const bool bad = __ballot(lane < 15 && over) != 0ull;
    const uint64_t unseen = DECK_NIB - hc0 - taken;   // (no borrow between nibbles where !bad; not used otherwise)
    if (bad || n_next < 1 || n_prev < 1 || nib_sum(unseen) != n_next + n_prev) {
      if (lane == 0 && chunk == 0) atomicOr(a.status, 64);
      return;   // outside the domain: nothing runs, wins stay as they are
    }
    const int rank = lane < 52 ? lane >> 2 : lane - 39;   // card -> rank: 52 = BJ (13), 53 = CJ (14)
    const int cnt = (int)((unseen >> (4 * (rank & 15))) & 15);
    pool = lane < 52 ? (lane & 3) < cnt : (lane < 54 && cnt == 1);
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
    uint64_t hc = hc0, hn = hn0, hp = hp0;
    if constexpr (HIDDEN) {
      if (!probe) {   // (the probe sizes the root's list: the actor's hand alone)
        if (k != world_k) {   // (an item whose chunks divide by K stays with one world)
          redeal_wave(gid, k, a.k0, a.k1, lane, pool, n_next, stage, wn, wp);
          world_k = k;
        }
        hn = wn; hp = wp;
      }
    }
    uint32_t trick = trick0, ply = ply0;
    int passes = passes0, role = role0;
    uint32_t draws = 0, dnext = 64;  // lane l holds the draw of the ply l behind the last refill; 64 = refill
    int winner = -1;
    for (int s = 0; s < DDZ_PLAYOUT_MAX_PLIES; ++s) {
      uint32_t draw = 0;
      if (s > 0) {  // (the first move is the pick at index j: no draw)
        uint32_t dn = rfl(dnext);
        if (dn >= 64u) {
          dn = 0;
          dnext = 0;
          uint32_t qk0 = a.k0, qk1 = a.k1;
          asm volatile("" : "+s"(qk0), "+s"(qk1));
          draws = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), (k << 9) | j,
                                           (4u << 16) | ((ply + (uint32_t)lane) & 0xFFFFu)), qk0, qk1).x;
        }
        draw = rl(draws, (int)dn);
      }
      const uint64_t hand = hc;
      const uint32_t info = rfl((passes >= 2) ? mk_info(EMPTY, 0, 1) : trick);
      const int lc0 = (int)(info & 0xFF);
      const bool lead = lc0 == EMPTY;
      const int cntr = lane < 15 ? (int)((hand >> (4 * (lane & 15))) & 15) : 0;
      const uint32_t b1 = (uint32_t)__ballot(cntr >= 1), b4 = (uint32_t)__ballot(cntr >= 4);
      // the legal lanes of the closed-form round (55 lanes of the lead layout, 30 of the follow layout) and whether the list
      // has a tail beyond it: k_rollout's tests on the rank masks, nothing emitted
      uint64_t okm = 0;
      bool tail = false;
      if ((b1 & M15) == 0) {
        // an empty hand on a running table (an imported state outside the domain): the empty list, the playout stops
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
          okm = (uint64_t)m1 | (uint64_t)m2 << 15 | (uint64_t)m3 << 28 | (uint64_t)m4 << 41 |
                (jokers && !tail ? 1ull << 54 : 0ull);   // (with a tail the rocket is the planner's: id order)
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
      if (tail) {  // the planner without its first range stages the rest of the list from index 0 of the wave's LDS list
        const Out o{nullptr, nullptr, 0, 0, stage, svl, nullptr};
        Pick pk{-1, 0, 0, 0, 0};
        const Follow f = follow_of(info);
        const int n1 = lead ? plan_scan_t<EM_STAGE, false, true, HotTabT<false>, false>(hand, f, hot, lane, o, pk)
                            : plan_scan_t<EM_STAGE, false, false, HotTabT<false>, false>(hand, f, hot, lane, o, pk);
        __builtin_amdgcn_wave_barrier();
        n = (int)rfl((uint32_t)(n0 + n1));
      }
      if (n > STAGE_CAP || n > a.stride) {  // cannot happen for a <= 20-card hand: the table (or this playout) runs nothing
        if (lane == 0) atomicOr(a.status, 2);
        n = 0;
      }
      if (probe) {
        total = (uint64_t)n * a.K;
        break;
      }
      if (n <= 0) break;  // stopped unfinished
      const int idx = s == 0 ? (int)j : (int)rfl(__umulhi(draw, (uint32_t)n));  // random.choice(actions), envi.py:83
      uint64_t snib = 0;
      uint32_t scat = 0, svlv = 0, ncards = 0;
      if (idx < n0) {  // from the round, by lane number
        if (lead) round_entry<true>(round_src<true>(okm, round_pre(okm), idx), 0u, snib, scat, svlv, ncards);
        else round_entry<false>(round_src<false>((uint32_t)okm, round_pre((uint32_t)okm), idx), (uint32_t)lc0, snib, scat, svlv, ncards);
      } else {         // from the staged tail (idx - n0 < n - n0 <= STAGE_CAP): LDS broadcast reads
        const uint64_t e = stage[idx - n0];
        const uint64_t anib = e & 0x0FFFFFFFFFFFFFFFull;
        snib = (uint64_t)rfl((uint32_t)anib) | ((uint64_t)rfl((uint32_t)(anib >> 32)) << 32);
        scat = rfl((uint32_t)(e >> 60));
        svlv = rfl((uint32_t)svl[idx - n0]);
      }
      (void)ncards;
      // the packed apply (envi.py:39-43 on what a playout carries: hands, the combo to beat, role, ply)
      const uint64_t hnew = hand - snib;
      if (snib) { trick = scat | (svlv << 8); passes = 0; } else { passes += 1; }
      s_moves += 1;
      ply += 1;
      dnext += 1;
      __builtin_amdgcn_wave_barrier();  // the staging list is reused by the next ply
      if (rfl((uint32_t)hnew | (uint32_t)(hnew >> 32)) == 0u) {
        winner = role;
        break;
      }
      role = role == 2 ? 0 : role + 1;  // lord -> down -> up, game.py:173-181
      hc = hn; hn = hp; hp = hnew;
    }
    if (probe) {
      probe = false;
      continue;
    }
    s_playouts += 1;
    if (winner < 0) s_unfinished += 1;
    else if ((winner == 1) == (role0 == 1)) win_j += 1;   // tree.py:71-81: the lord alone, or either farmer
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
