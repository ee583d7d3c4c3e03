// ddz_ply.h -- what k_playout (ddz_playout.h), k_search (ddz_search.h), k_ismcts (ddz_ismcts.h), k_cfr (ddz_cfr.h) and k_solve
// (ddz_solve.h) share, each piece stated once:
//   PlyArgs           the six fields every evaluator's arguments hold BY NAME (state, T, k0, k1, gid_base, status): a base of
//                     SearchArgs, CfrArgs and SolveArgs; PlayoutArgs spells them out in its own order (ddz_playout.h)
//   table_enter       a wave enters its table: the 176-byte row load, the hot table's fill, the block's one barrier, the leave
//   play_root_decode  the 176-byte root as wave-uniform values: running, role, ply, the actor's hand, the combo to beat with
//                     the passes since it was played
//   unseen_pool       the hidden-hand domain (playout spec v2): what the actor has not seen, the opponents' hand
//                     sizes, this lane's bit of the 54-lane pool mask
//   root_hands        the decode, the `roles` gate, the opponents' hands (open: the hand rows; hidden: unseen_pool), the hand
//                     sizes, and idle / outside the domain / inside.  No status bit, no output: those are the callers'
//   redeal_wave       world k of a table: the pool dealt to the two opponents
//   ply_list          the legal list of (hand, combo to beat): the closed-form round's legal lanes as a mask (never emitted),
//                     the planner's tail staged into the wave's LDS list.  THE RANK-MASK CHAIN BELOW IS THE STATEMENT OF THE
//                     RULES for every kernel but k_rollout
//   ply_entry         entry idx of that list: from the round by lane number, or from the staged tail
//   ply_apply         the packed apply: the mover's hand, the combo to beat, passes, ply (ply_play), the turn (ply_turn)
//   ply_draw          the Philox call of the playout loops' 64-draw refill (each loop keeps its refill bookkeeping)
//   same_side         two roles play on one side (the lord alone, or either farmer)
//   rfl64 / sld / sst / search_fence   a 64-bit value made wave-uniform; relaxed wavefront-scope atomic accesses and the fence
//                     that orders them (ddz_search.h, MEMORY ORDERING), for the workspaces one wavefront writes and reads
// Included by ddz_engine.hip behind k_rollout and ahead of the four headers, inside its anonymous namespace: built from
// k_rollout's device functions (round_pre / round_src / round_entry, plan_scan_t<EM_STAGE>, deal ranking through LDS), none of
// which it changes.  The two playout loops (k_playout's with the probe pass, k_search's with the child's n) stay where they are
// and call these.
constexpr uint64_t DECK_NIB = 0x0114444444444444ull;  // four of the ranks 3 .. 2, one of each joker

__device__ __forceinline__ uint64_t sld64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ uint32_t sld32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void sst64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void sst32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void search_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t rfl64(uint64_t v) { return (uint64_t)rfl((uint32_t)v) | ((uint64_t)rfl((uint32_t)(v >> 32)) << 32); }

__device__ __forceinline__ int role_next(int role) { return role == 2 ? 0 : role + 1; }
__device__ __forceinline__ int role_prev(int role) { return role == 0 ? 2 : role - 1; }
__device__ __forceinline__ bool same_side(int a, int b) { return (a == 1) == (b == 1); }   // tree.py:71-81: the lord alone, or either farmer

struct PlyArgs {
  const uint8_t* state;
  int64_t T;
  uint32_t k0, k1;          // Philox key: (seed_lo ^ salt, seed_hi)
  uint64_t gid_base;
  int32_t* status;
};

// a wave of a block of WAVES enters table t: lanes < DDZ_NFIELDS load the table's rows into R, the block fills the hot table
// and meets at its only barrier.  false: there is no table t, the wave leaves (behind the barrier).
template <int WAVES, typename Args>
__device__ __forceinline__ bool table_enter(const Args& a, int64_t t, int lane, HotTabT<false>& hot, uint4& R) {
  R = make_uint4(0, 0, 0, 0);
  if (t < a.T && lane < DDZ_NFIELDS) R = ((const uint4*)(a.state + t * STATE_ROW_BYTES))[lane];
  hot_fill<WAVES * 64>(hot);
  __syncthreads();
  return t < a.T;
}

// the root of a table, decoded once (as k_rollout decodes a table): row f < 10 as 15 nibbles in lane f of P, byte 15 of row f
// in lane f of aux, the meta row's words as scalars.  Every field is wave-uniform.
struct PlayRoot {
  uint64_t P;
  uint32_t aux;
  bool running;      // dealt and not done
  int role0;
  uint32_t ply0;
  uint64_t hc0;      // the actor's hand
  uint32_t trick0;   // the combo to beat (envi.py:103-109) ...
  int passes0;       // ... and the passes since it was played: 0 = the previous player's, 1 = the one before's
  bool lead0;        // both recent rows are empty: the actor leads
};
__device__ __forceinline__ PlayRoot play_root_decode(const uint4& R) {
  PlayRoot r = {};
  r.P = pack_row(R);
  r.aux = R.w >> 24;
  const uint32_t mx = rl(R.x, DDZ_F_META), my = rl(R.y, DDZ_F_META);
  r.role0 = meta_role(mx);
  r.running = meta_dealt(my) && !meta_done(mx);
  if (!r.running) return r;   // (the caller leaves: nothing else is read)
  r.ply0 = my & 0xFFFF;
  r.hc0 = rl64(r.P, DDZ_F_HAND0 + r.role0);
  const int rm1 = role_prev(r.role0), rp1 = role_next(r.role0);
  const uint64_t n1 = rl64(r.P, DDZ_F_RECENT0 + rm1), n2 = rl64(r.P, DDZ_F_RECENT0 + rp1);
  r.trick0 = mk_info(EMPTY, 0, 1);
  r.lead0 = !n1 && !n2;
  if (n1) r.trick0 = info_of_row(n1, (int)rl(r.aux, DDZ_F_RECENT0 + rm1));
  else if (n2) { r.trick0 = info_of_row(n2, (int)rl(r.aux, DDZ_F_RECENT0 + rp1)); r.passes0 = 1; }
  return r;
}

// the hidden-hand domain, checked once per root: per rank hand + taken <= the deck's copies, both opponents hold a card, and
// what the actor has not seen (`unseen` = deck - own hand - taken) is as many cards as the opponents' sizes say.  false:
// outside the domain (the caller raises status bit 6 and runs nothing).  `pool`: this lane's card (Deal v2's numbering) is
// unseen.  The opponents' count bytes are never read.
__device__ __forceinline__ bool unseen_pool(const PlayRoot& r, int lane, int& n_next, int& n_prev, uint64_t& unseen, bool& pool) {
  const uint64_t taken = rl64(r.P, DDZ_F_TAKEN);
  n_next = (int)rl(r.aux, DDZ_F_HAND0 + role_next(r.role0));
  n_prev = (int)rl(r.aux, DDZ_F_HAND0 + role_prev(r.role0));
  const int sh = 4 * (lane & 15);
  const int deck = lane < 13 ? 4 : lane < 15 ? 1 : 0;
  const bool over = (int)((r.hc0 >> sh) & 15) + (int)((taken >> sh) & 15) > deck;   // unseen_r < 0
  const bool bad = __ballot(lane < 15 && over) != 0ull;
  unseen = DECK_NIB - r.hc0 - taken;   // (no borrow between nibbles where !bad; not used otherwise)
  pool = false;
  if (bad || n_next < 1 || n_prev < 1 || nib_sum(unseen) != n_next + n_prev) return false;
  const int rank = lane < 52 ? lane >> 2 : lane - 39;   // card -> rank: 52 = BJ (13), 53 = CJ (14)
  const int cnt = (int)((unseen >> (4 * (rank & 15))) & 15);
  pool = lane < 52 ? (lane & 3) < cnt : (lane < 54 && cnt == 1);
  return true;
}

// the root with its hands.  IDLE: not dealt, done, or the actor is not in `roles` (nothing else is set).  Open form: hn0 / hp0
// are the next and the previous player's hand rows and the table is INSIDE.  Hidden form: unseen_pool decides, n_next / n_prev
// are set either way, hn0 / hp0 wait for redeal_wave.  n_me < 1 is left to the callers that care.
enum RootKind { ROOT_IDLE, ROOT_OUTSIDE, ROOT_INSIDE };
struct RootHands {
  PlayRoot root;
  RootKind kind;
  uint64_t hn0, hp0;
  int n_me, n_next, n_prev;
  uint64_t unseen;   // hidden form: deck - own hand - taken
  bool pool;         // hidden form: this lane's card is unseen
};
template <bool HIDDEN>
__device__ __forceinline__ RootHands root_hands(const uint4& R, uint32_t roles, int lane) {
  RootHands h = {};
  h.root = play_root_decode(R);
  h.kind = ROOT_IDLE;
  if (!h.root.running || !((roles >> h.root.role0) & 1u)) return h;
  h.n_me = nib_sum(h.root.hc0);
  if constexpr (HIDDEN) {
    h.kind = unseen_pool(h.root, lane, h.n_next, h.n_prev, h.unseen, h.pool) ? ROOT_INSIDE : ROOT_OUTSIDE;
  } else {
    h.hn0 = rl64(h.root.P, DDZ_F_HAND0 + role_next(h.root.role0));
    h.hp0 = rl64(h.root.P, DDZ_F_HAND0 + role_prev(h.root.role0));
    h.n_next = nib_sum(h.hn0);
    h.n_prev = nib_sum(h.hp0);
    h.kind = ROOT_INSIDE;
  }
  return h;
}

// world k of a table (playout spec v2): the hands of the next and of the previous player as nibble words.  Lane c draws the key
// of card c (RNG domain 5, keyed by (gid, k) alone), the pool is ranked by (key, c) through LDS as deal_wave_lds ranks a deal,
// and two ballots give the hands.  `pool`: unseen_pool's; keys: 64 x 8 bytes of the calling wave; 1 <= n_next.
__device__ inline void redeal_wave(uint64_t gid, uint32_t k, uint32_t k0, uint32_t k1, int lane, bool pool, int n_next,
                                   uint64_t* keys, uint64_t& o_next, uint64_t& o_prev) {
  const uint4 d = philox4x32_10(make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), k, (RNG_WORLD << 16) | (uint32_t)(lane >> 2)), k0, k1);
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

// the combo a mover has to beat: two passes hand the lead back (wave-uniform)
__device__ __forceinline__ uint32_t ply_info(uint32_t trick, int passes) { return rfl((passes >= 2) ? mk_info(EMPTY, 0, 1) : trick); }

// the legal list of the state (hand, info): the legal lanes of the closed-form round (55 lanes of the lead layout, 30 of the
// follow layout) as the mask okm -- k_rollout's tests on the rank masks, nothing emitted: a ply needs the list's SIZE and its
// idx-th ENTRY only -- and, where the rank masks allow a tail beyond the round, the planner without its first range staging the
// rest of the list from index 0 of the wave's LDS list.  Returns the list's size (n0 = the round's share).
template <typename HT>
__device__ __forceinline__ int ply_list(uint64_t hand, uint32_t info, const HT& hot, int lane, uint64_t* stage, uint16_t* svl,
                                        uint64_t& okm_out, int& n0_out) {
  const int lc0 = (int)(info & 0xFF);
  const bool lead = lc0 == EMPTY;
  const int cntr = lane < 15 ? (int)((hand >> (4 * (lane & 15))) & 15) : 0;
  const uint32_t b1 = (uint32_t)__ballot(cntr >= 1), b4 = (uint32_t)__ballot(cntr >= 4);
  uint64_t okm = 0;
  bool tail = false;
  if ((b1 & M15) == 0) {
    // an empty hand on a running state (an imported state outside the domain): the empty list
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

// entry idx < n of the list ply_list left: the nibble word, the category and the value/len byte pair (wave-uniform)
__device__ __forceinline__ void ply_entry(uint64_t okm, int n0, int idx, uint32_t info, const uint64_t* stage, const uint16_t* svl,
                                          uint64_t& snib, uint32_t& scat, uint32_t& svlv) {
  const int lc0 = (int)(info & 0xFF);
  const bool lead = lc0 == EMPTY;
  uint32_t ncards = 0;
  snib = 0; scat = 0; svlv = 0;
  if (idx < n0) {  // from the round, by lane number
    if (lead) round_entry<true>(round_src<true>(okm, round_pre(okm), idx), 0u, snib, scat, svlv, ncards);
    else round_entry<false>(round_src<false>((uint32_t)okm, round_pre((uint32_t)okm), idx), (uint32_t)lc0, snib, scat, svlv, ncards);
  } else {         // from the staged tail (idx - n0 < n - n0 <= STAGE_CAP): LDS broadcast reads
    const uint64_t e = stage[idx - n0];
    snib = rfl64(e & 0x0FFFFFFFFFFFFFFFull);
    scat = rfl((uint32_t)(e >> 60));
    svlv = rfl((uint32_t)svl[idx - n0]);
  }
  (void)ncards;
}

// the packed apply of the entry (snib, scat, svlv) (envi.py:39-43 on what a playout carries: the hands in turn order, the combo
// to beat with the passes since, role, ply), in its two halves -- ply_play: the move is made, -> the mover's hand after it;
// ply_turn: the turn passes on, lord -> down -> up (game.py:173-181) -- and whole.  ply_apply -> true: the mover's hand is
// empty, the game is over, `role` is the winner and the turn has not passed on.
__device__ __forceinline__ uint64_t ply_play(uint64_t snib, uint32_t scat, uint32_t svlv, uint64_t hc, uint32_t& trick, int& passes,
                                             uint32_t& ply) {
  if (snib) { trick = scat | (svlv << 8); passes = 0; } else { passes += 1; }
  ply += 1;
  return hc - snib;
}
__device__ __forceinline__ void ply_turn(uint64_t hnew, uint64_t& hc, uint64_t& hn, uint64_t& hp, int& role) {
  role = role_next(role);
  hc = hn; hn = hp; hp = hnew;
}
__device__ __forceinline__ bool ply_apply(uint64_t snib, uint32_t scat, uint32_t svlv, uint64_t& hc, uint64_t& hn, uint64_t& hp,
                                          uint32_t& trick, int& passes, int& role, uint32_t& ply) {
  const uint64_t hnew = ply_play(snib, scat, svlv, hc, trick, passes, ply);
  __builtin_amdgcn_wave_barrier();  // the staging list is reused by the next ply
  if (rfl((uint32_t)hnew | (uint32_t)(hnew >> 32)) == 0u) return true;
  ply_turn(hnew, hc, hn, hp, role);
  return false;
}

// the Philox call of a playout loop's 64-draw refill: lane l gets the draw of the ply l behind this one, on the counter
// (gid, c2, c3 | ply + lane) -- c2 and c3 say whose playout and which RNG domain.  The refill's bookkeeping (the draws, the
// plies since: dnext, 64 = refill) stays in each loop: k_playout pins the key inside its refill branch.
__device__ __forceinline__ uint32_t ply_draw(uint64_t gid, uint32_t c2, RngDomain domain, uint32_t ply, int lane, uint32_t k0, uint32_t k1) {
  return rng_draw(gid, c2, domain, (ply + (uint32_t)lane) & 0xFFFFu, k0, k1).x;
}
