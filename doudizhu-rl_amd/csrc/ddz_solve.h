// ddz_solve.h -- k_solve / k_solve_choose: the exact endgame solver ("Solve spec v1"): open-hand minimax of the
// two-sided win / lose game (the lord against the two farmers) for every root move of every table that is an endgame.
// Included by ddz_engine.hip behind ddz_ply.h, inside its anonymous namespace.  The entry into a table (table_enter,
// root_hands: the root, its hands, the hidden-hand domain), the deal (redeal_wave), the legal lists (ply_list / ply_entry: the
// device keeps one statement of the rules), the packed apply (ply_play / ply_turn), same_side and the wavefront-scope accesses
// (rfl64 / sld / sst / search_fence) are ddz_ply.h's, shared with the other three; this header holds the search and its table.
//
// One wavefront per WORK ITEM (table t, world k, chunk c), item = (t * worlds + k) * chunks + c.  Chunk c solves the root moves
// j = c, c + chunks, ... of its table in ascending order, each with a node budget of its own and no cut among them.
//
// POSITION.  Wave-uniform values: the three hands in turn order (hc the mover's, hn, hp), the combination to beat as its
// category / value / length word (`trick`, what ply_list reads) AND as its cards (`tnib`, what the table's key holds), the
// passes since it was played, the mover's role.  Two passes hand the lead back: a position whose passes reached 2 is the
// lead position (nothing to beat, no passes) in its key.
//
// SEARCH of one root move.  The move is applied; if it empties the actor's hand the actor's side has won.  Otherwise the
// position behind it is ENTERED.  Entering a position: if the move's nodes have reached `budget` the move is UNKNOWN and its
// search ends; else the node is counted, the table is probed (a hit returns the stored value), the position's list is built
// and its children are tried in list order: a child whose move empties the mover's hand wins at once (it is not entered and
// is no node), any other child is entered; the first child that wins for the mover's side ends the position as WON (the
// cut), a position whose children all lose -- or whose list is empty -- is LOST.  A finished position is stored in the table.
// What a child's value means to its parent: the same where both movers are on one side (the two farmers), the opposite
// otherwise.
//
// FRAMES.  The search is iterative; a frame per applied move below the root move holds what resumes and undoes it: the move's
// nibble word with the passes before it, the cards of the combination that was to beat, its info word, the child index and the
// list size.  The list itself is derived again on return (ply_list) where another child is left to try.  Depth: every move
// that is no pass removes a card, at most two passes follow one and at most two precede the first, and the last move of a
// game is no pass: at most 3 * cards moves from the root, so DDZ_SOLVE_MAX_DEPTH = 3 * DDZ_SOLVE_MAX_CARDS frames hold every
// search of the domain.  The guard that refuses a deeper push raises status bit 8 and leaves the move unknown.
// Frames live in the wave's LDS beside the staging list: written by lane 0, read as broadcasts behind search_fence().
//
// TRANSPOSITION TABLE.  `tt_entries` (a power of two) entries of 32 bytes per work item in the caller's workspace, direct
// mapped, always replaced, cleared by the wave itself (the first word of every entry) before its first root move and shared by
// the root moves it solves.  An entry is the WHOLE key and one bit of value:
//   word 0  hc | mover << 60 | 1 << 63 (an entry in use)        word 1  hn | (the mover's side wins) << 60
//   word 2  hp                                                    word 3  the cards of the combination to beat | passes << 60
// and a hit compares all of it.  slot = solve_slot(the key's four words) & (tt_entries - 1).  Only finished positions are
// stored, so what an exhausted budget leaves behind are still proven values.
//
// LOOPS.  Root moves by the list size, the search by a step count no search of `budget` nodes reaches (each node takes at most
// 2 * n + 3 steps of the state machine below), the clearing by tt_entries.  A wave waits for no other wave.
//
// MEMORY ORDERING.  As ddz_search.h: a table is written and read by ONE wavefront through relaxed wavefront-scope atomic loads
// / stores (vector instructions) with search_fence() behind every store.  n leaves through a plain store of the table's
// first wave, wins / unknown through 32-bit atomic adds (the worlds of a table add up), the totals through 64-bit ones.
struct SolveArgs : PlyArgs {   // (the key: of the worlds)
  uint32_t budget, max_cards, worlds, chunks, roles, tt_entries;
  int64_t stride;           // wins / unknown are [T][stride]
  int32_t* n;
  int32_t* wins;
  int32_t* unknown;
  unsigned long long* totals;  // {nodes, table hits, root moves solved, root moves unknown} or null
  uint8_t* work;            // items x tt_entries x 32 bytes
};

constexpr int SOLVE_WAVES = 8;    // 66 KB of LDS per block: two blocks per CU = 4 waves per SIMD
constexpr int SOLVE_FRAMES = DDZ_SOLVE_MAX_DEPTH + 4;
constexpr uint64_t SOLVE_USED = 1ull << 63, SOLVE_WON = 1ull << 60, SOLVE_HAND = 0x0FFFFFFFFFFFFFFFull;
constexpr uint32_t SOLVE_ENTRY_BYTES = 32;
static_assert(DDZ_SOLVE_MAX_DEPTH == 3 * DDZ_SOLVE_MAX_CARDS, "at most two passes around every card played");

// the slot of a key (before the mask): four odd multipliers, one xor-shift-multiply round, the high half folded in
__device__ __forceinline__ uint32_t solve_slot(uint64_t x, uint64_t y, uint64_t z, uint64_t w) {
  uint64_t h = (x * 0x9E3779B97F4A7C15ull) ^ (y * 0xC2B2AE3D27D4EB4Full) ^ (z * 0x165667B19E3779F9ull) ^ (w * 0x85EBCA77C2B2AE63ull);
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return (uint32_t)h;
}

template <bool HIDDEN>
__global__ __launch_bounds__(SOLVE_WAVES * 64, 4) void k_solve(SolveArgs a) {
  __shared__ HotTabT<false> hot;
  __shared__ uint64_t s_stage[SOLVE_WAVES][STAGE_CAP];
  __shared__ uint16_t s_svl[SOLVE_WAVES][STAGE_CAP];
  __shared__ uint64_t s_frame[SOLVE_WAVES][3 * SOLVE_FRAMES];
  const int lane = threadIdx.x & 63;
  const int wv = (int)rfl(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * SOLVE_WAVES + wv;
  const int64_t per = (int64_t)a.worlds * a.chunks;
  const int64_t t = item / per;
  const uint32_t world = (uint32_t)((item - t * per) / a.chunks);
  const uint32_t chunk = (uint32_t)(item - t * per - (int64_t)world * a.chunks);
  uint4 R;
  if (!table_enter<SOLVE_WAVES>(a, t, lane, hot, R)) return;
  uint64_t* stage = s_stage[wv];
  uint16_t* svl = s_svl[wv];
  uint64_t* frame = s_frame[wv];
  const bool first = world == 0 && chunk == 0 && lane == 0;   // the lane that writes n[t] and the table's status bits
  // ---- decode and domain
  const RootHands rh = root_hands<HIDDEN>(R, a.roles, lane);
  if (rh.kind == ROOT_IDLE) {
    if (first) a.n[t] = 0;
    return;
  }
  const PlayRoot& root = rh.root;
  const int role0 = root.role0;
  const uint64_t hc0 = root.hc0;
  uint64_t hn0 = rh.hn0, hp0 = rh.hp0;
  if (rh.n_me + rh.n_next + rh.n_prev > (int)a.max_cards) {   // not an endgame: what a dispatcher tests
    if (first) a.n[t] = -1;
    return;
  }
  if (HIDDEN && (rh.kind == ROOT_OUTSIDE || rh.n_me < 1)) {
    if (first) { a.n[t] = -1; atomicOr(a.status, DDZ_ST_DOMAIN); }
    return;
  }
  if constexpr (HIDDEN) redeal_wave(a.gid_base + (uint64_t)t, world, a.k0, a.k1, lane, rh.pool, rh.n_next, stage, hn0, hp0);
  // the cards of the combination to beat, as play_root_decode picks its info word
  const uint64_t r1 = rl64(root.P, DDZ_F_RECENT0 + role_prev(role0)), r2 = rl64(root.P, DDZ_F_RECENT0 + role_next(role0));
  const uint64_t tnib0 = rfl64(r1 ? r1 : r2);
  const uint32_t trick0 = rfl(root.trick0);
  const uint32_t info0 = ply_info(trick0, root.passes0);
  int n_root;
  {
    uint64_t okm; int n0;
    n_root = ply_list(hc0, info0, hot, lane, stage, svl, okm, n0);
    __builtin_amdgcn_wave_barrier();
  }
  if (n_root > STAGE_CAP || n_root > a.stride) {   // cannot happen for a <= 20-card hand: the table runs nothing
    if (first) { a.n[t] = 0; atomicOr(a.status, DDZ_ST_CAPACITY); }
    return;
  }
  if (first) a.n[t] = n_root;
  if ((int)chunk >= n_root) return;   // no root move for this chunk: the workspace is not touched
  uint64_t* const tt = (uint64_t*)(a.work + (uint64_t)item * a.tt_entries * SOLVE_ENTRY_BYTES);
  const uint32_t tmask = a.tt_entries - 1u;
  for (uint32_t i = (uint32_t)lane; i < a.tt_entries; i += 64) sst64(tt + 4ull * i, 0ull);
  search_fence();
  const uint64_t step_cap = ((uint64_t)a.budget + 1ull) * (2ull * STAGE_CAP + 4ull);
  unsigned long long s_nodes = 0, s_hits = 0;
  uint32_t s_solved = 0, s_unknown = 0;
  for (int j = (int)chunk; j < n_root; j += (int)a.chunks) {
    uint64_t hc = hc0, hn = hn0, hp = hp0, tnib = tnib0;
    uint32_t trick = trick0, ply = 0;
    int passes = root.passes0, role = role0;
    uint64_t okm; int n0;
    int n = ply_list(hc, info0, hot, lane, stage, svl, okm, n0);   // (the search of the move before reused the staging list)
    uint32_t info = info0;
    uint64_t snib; uint32_t scat, svlv;
    ply_entry(okm, n0, j, info, stage, svl, snib, scat, svlv);
    bool unk = false, won = false;    // won: the ROOT actor's side wins behind move j
    {
      const uint64_t hnew = ply_play(snib, scat, svlv, hc, trick, passes, ply);
      if (snib) tnib = snib;
      __builtin_amdgcn_wave_barrier();
      if (hnew == 0) won = true;
      else {
        ply_turn(hnew, hc, hn, hp, role);
        // ---- the depth-first search of the position behind move j; ret: the mover's side wins the position just finished
        enum { ENTER, CHILD, RETURN };
        int phase = ENTER, depth = 0, idx = 0;
        bool ret = false, over = false;
        uint32_t nodes = 0;
        uint64_t kx = 0, kw = 0;   // the key of the position whose children are tried (words 0 and 3; 1 and 2 are hn, hp)
        for (uint64_t step = 0; ; ++step) {
          if (step >= step_cap) { unk = true; over = true; break; }   // (cannot happen)
          bool finished = false;   // the current position got its value `ret`: store it, then return it
          if (phase == ENTER) {
            if (nodes >= a.budget) { unk = true; break; }
            nodes += 1;
            const bool lead = passes >= 2 || (trick & 0xFFu) == (uint32_t)EMPTY;
            kx = hc | ((uint64_t)role << 60);
            kw = lead ? 0ull : (tnib | ((uint64_t)passes << 60));
            const uint64_t* e = tt + 4ull * (solve_slot(kx, hn, hp, kw) & tmask);
            const uint64_t e0 = rfl64(sld64(e)), e1 = rfl64(sld64(e + 1));
            const uint64_t e2 = rfl64(sld64(e + 2)), e3 = rfl64(sld64(e + 3));
            if (e0 == (kx | SOLVE_USED) && (e1 & ~SOLVE_WON) == hn && e2 == hp && e3 == kw) {
              s_hits += 1;
              ret = (e1 & SOLVE_WON) != 0;
              phase = RETURN;
              continue;
            }
            info = ply_info(trick, passes);
            n = ply_list(hc, info, hot, lane, stage, svl, okm, n0);
            __builtin_amdgcn_wave_barrier();
            if (n > STAGE_CAP) {   // cannot happen for a <= 20-card hand
              if (lane == 0) atomicOr(a.status, DDZ_ST_CAPACITY);
              n = 0;
            }
            idx = 0;
            phase = CHILD;
          }
          if (phase == CHILD) {
            if (idx >= n) { ret = false; finished = true; }
            else {
              ply_entry(okm, n0, idx, info, stage, svl, snib, scat, svlv);
              if (hc == snib) { ret = true; finished = true; }   // the move empties the mover's hand
              else if (depth >= DDZ_SOLVE_MAX_DEPTH) { unk = true; over = true; break; }   // (impossible inside the domain)
              else {
                if (lane == 0) {
                  frame[3 * depth + 0] = snib | ((uint64_t)passes << 60);
                  frame[3 * depth + 1] = tnib;
                  frame[3 * depth + 2] = (uint64_t)trick | ((uint64_t)idx << 24) | ((uint64_t)n << 40);
                }
                const uint64_t hnew = ply_play(snib, scat, svlv, hc, trick, passes, ply);
                if (snib) tnib = snib;
                ply_turn(hnew, hc, hn, hp, role);
                depth += 1;
                search_fence();   // the frame is written; the staging list is the next position's
                phase = ENTER;
                continue;
              }
            }
          }
          if (finished) {
            if (lane == 0) {
              uint64_t* e = tt + 4ull * (solve_slot(kx, hn, hp, kw) & tmask);
              sst64(e, kx | SOLVE_USED);
              sst64(e + 1, hn | (ret ? SOLVE_WON : 0ull));
              sst64(e + 2, hp);
              sst64(e + 3, kw);
            }
            search_fence();
            phase = RETURN;
          }
          // ---- RETURN: `ret` goes to the parent, whose frame undoes the move
          if (depth == 0) break;
          depth -= 1;
          const uint64_t f0 = rfl64(frame[3 * depth + 0]), f1 = rfl64(frame[3 * depth + 1]);
          const uint64_t f2 = rfl64(frame[3 * depth + 2]);
          const int child_role = role;
          role = role_prev(role);
          {
            const uint64_t hnew = hp;
            hp = hn; hn = hc; hc = hnew + (f0 & SOLVE_HAND);
          }
          passes = (int)(f0 >> 60);
          tnib = f1;
          trick = (uint32_t)f2 & 0xFFFFFFu;
          idx = (int)((f2 >> 24) & 0xFFFFu) + 1;
          n = (int)((f2 >> 40) & 0xFFFFu);
          {
            const bool lead = passes >= 2 || (trick & 0xFFu) == (uint32_t)EMPTY;
            kx = hc | ((uint64_t)role << 60);
            kw = lead ? 0ull : (tnib | ((uint64_t)passes << 60));
          }
          const bool mine = same_side(child_role, role) ? ret : !ret;
          if (mine || idx >= n) {   // the cut, or the last child lost: the parent is finished; it returns on the next trip
            ret = mine;
            if (lane == 0) {
              uint64_t* e = tt + 4ull * (solve_slot(kx, hn, hp, kw) & tmask);
              sst64(e, kx | SOLVE_USED);
              sst64(e + 1, hn | (ret ? SOLVE_WON : 0ull));
              sst64(e + 2, hp);
              sst64(e + 3, kw);
            }
            search_fence();
            phase = RETURN;
            continue;
          }
          info = ply_info(trick, passes);
          n = ply_list(hc, info, hot, lane, stage, svl, okm, n0);   // the list again: its next entry is tried
          __builtin_amdgcn_wave_barrier();
          phase = CHILD;
        }
        if (over && lane == 0) atomicOr(a.status, DDZ_ST_SOLVE_DEPTH);
        if (!unk) won = same_side(role, role0) ? ret : !ret;   // (depth 0: `role` moves behind move j)
        s_nodes += nodes;
      }
    }
    if (unk) {
      s_unknown += 1;
      if (lane == 0) atomicAdd(a.unknown + t * a.stride + j, 1);
    } else {
      s_solved += 1;
      if (won && lane == 0) atomicAdd(a.wins + t * a.stride + j, 1);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0 && a.totals) {
    atomicAdd(a.totals + 0, s_nodes);
    if (s_hits) atomicAdd(a.totals + 1, s_hits);
    if (s_solved) atomicAdd(a.totals + 2, (unsigned long long)s_solved);
    if (s_unknown) atomicAdd(a.totals + 3, (unsigned long long)s_unknown);
  }
}

// ddz_solve_choose: one lane per table.  The first move with the most wins, among equals the first with the fewest unknown;
// value 1 where that move won in every world, 0 where every move is proven lost in every world, else -1.
__global__ __launch_bounds__(BLOCK) void k_solve_choose(const int32_t* __restrict__ counts, const int32_t* __restrict__ ids,
                                                        int64_t stride, int32_t worlds, const int32_t* __restrict__ wins,
                                                        const int32_t* __restrict__ unknown, int32_t* __restrict__ choice,
                                                        int32_t* __restrict__ value, int64_t T) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= T) return;
  int64_t c = counts[t];
  if (c > stride) c = stride;
  if (c <= 0) { choice[t] = -1; value[t] = -1; return; }
  int64_t at = 0;
  int32_t bw = wins[t * stride], bu = unknown[t * stride];
  bool all_lost = bw == 0 && bu == 0;
  for (int64_t j = 1; j < c; ++j) {
    const int32_t w = wins[t * stride + j], u = unknown[t * stride + j];
    if (w > bw || (w == bw && u < bu)) { bw = w; bu = u; at = j; }
    all_lost = all_lost && w == 0 && u == 0;
  }
  choice[t] = ids[t * stride + at];
  value[t] = bw >= worlds ? 1 : all_lost ? 0 : -1;
}
