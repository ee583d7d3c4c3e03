"""Stateless observation / legal moves from the reference's serving payload, and the payloads of live tables
(state_to_payloads <-> payloads_to_state).

The reference's HTTP predictor receives, per request, a dict
    {role_id, cur_cards, history{0,1,2}, left{0,1,2}, last_taken{0,1,2}}      (server/client.py:6-25)
with card lists as rank values 3..17, and derives from it the EnvCooperationSimplify `face`
(server/core.py:44-54, prob planes via get_state_prob_manual :26-33) and the legal moves
against last_taken[(role-1)%3] or, if empty, last_taken[(role-2)%3] (server/core.py:56-67).
Here a batch of payloads is packed into the engine's state rows on the host (a few hundred
bytes per request) and handed to the same kernels the batched env uses (ddz_observe,
ddz_get_moves), so a served observation is bit-identical to the one of a live table.
"""
import numpy as np
import torch

from .engine import (BatchedEnv, F_HAND0, F_HIST0, F_META, F_RECENT0, F_TAKEN, META_DEALT, META_NO_WINNER, META_ROLE, META_WINNER,
                     NFIELDS, ROW, STATUS_CFR_CAPACITY, STATUS_DOMAIN, action_table, auto_choose, get_moves)


def _counts(cards):
    out = np.zeros(15, np.uint8)
    for c in cards:
        out[int(c) - 3] += 1                      # envi.py:132-137 cards2arr
    return out


def _get(d, k):
    return d[k] if k in d else d[str(k)]          # JSON turns the integer role keys into strings


def payloads_to_state(payloads):
    """uint8 [n, 11, 16] state rows of n payloads (other players' hands are unknown: only
    their sizes are set, which is all `face` reads of them)."""
    st = np.zeros((len(payloads), NFIELDS, ROW), np.uint8)
    for i, p in enumerate(payloads):
        role = int(p["role_id"])
        st[i, F_HAND0 + role, :15] = _counts(p["cur_cards"])
        for r in range(3):
            st[i, F_HAND0 + r, 15] = int(_get(p["left"], r))
            st[i, F_HIST0 + r, :15] = _counts(_get(p["history"], r))
            st[i, F_RECENT0 + r, :15] = _counts(_get(p["last_taken"], r))
        st[i, F_TAKEN, :15] = st[i, F_HIST0:F_HIST0 + 3, :15].sum(0)   # server/core.py:41 taken = h0 + h1 + h2
        st[i, F_META, META_ROLE] = role
        st[i, F_META, META_WINNER] = META_NO_WINNER
        st[i, F_META, META_DEALT] = 1
    return st


def state_to_payloads(state):
    """The inverse of payloads_to_state: state rows (uint8 [n,11,16] -- a numpy array, a tensor, or a BatchedEnv, whose
    state is copied to the host) -> the list of n serving payloads {role_id, cur_cards, history, left, last_taken} the
    reference's HTTP predictor takes (server/client.py:6-25: card lists as rank values 3..17, dicts keyed by role 0 up /
    1 lord / 2 down), one per table, as seen by the table's ACTOR (only its own hand is in a payload).  What a caller
    that plays on the batched engine POSTs to a reference-style server."""
    if isinstance(state, BatchedEnv):
        state = state.state
    if torch.is_tensor(state):
        state = state.detach().cpu().numpy()
    st = np.asarray(state, np.uint8).reshape(-1, NFIELDS, ROW)
    ranks = np.arange(3, 18)

    def cards(row):
        return [int(x) for x in np.repeat(ranks, row[:15].astype(int))]   # envi.py:118-130 arr2cards

    out = []
    for s in st:
        role = int(s[F_META, META_ROLE])
        out.append({"role_id": role, "cur_cards": cards(s[F_HAND0 + role]),
                    "history": {r: cards(s[F_HIST0 + r]) for r in range(3)},
                    "left": {r: int(s[F_HAND0 + r, 15]) for r in range(3)},
                    "last_taken": {r: cards(s[F_RECENT0 + r]) for r in range(3)}})
    return out


def combo_category(counts):
    """The category (card.py:13-28: 0 pass, 1 single ... 12 rocket, 13 / 14 four with two) of a count vector that is a
    combination of the action space -- the byte a state's recent_handout row carries behind its counts, which a payload
    does not hold.  A vector that is no combination gives 0 (read as "nothing to beat")."""
    c = [int(x) for x in counts[:15]]
    n = [sum(1 for x in c if x == k) for k in range(5)]           # ranks held exactly k times

    def chain(k):                                                  # the ranks held k times are consecutive, within 3..A
        r = [i for i, x in enumerate(c) if x == k]
        return r[-1] - r[0] + 1 == len(r) and r[-1] < 12

    if not any(c) or max(c) > 4 or c[13] > 1 or c[14] > 1:
        return 0
    if n[2] == n[3] == n[4] == 0:
        if n[1] == 1:
            return 1
        if n[1] == 2 and c[13] and c[14]:
            return 12
        return 7 if n[1] >= 5 and chain(1) else 0
    if n[1] == n[3] == n[4] == 0:
        return 2 if n[2] == 1 else 8 if 3 <= n[2] <= 10 and chain(2) else 0
    if n[1] == n[2] == n[4] == 0:
        return 3 if n[3] == 1 else 9 if 2 <= n[3] <= 6 and chain(3) else 0
    if n[1] == n[2] == n[3] == 0:
        return 4 if n[4] == 1 else 0
    if n[3] and not n[4]:
        if not n[2] and n[1] == n[3]:
            return 5 if n[3] == 1 else 10 if n[3] <= 5 and chain(3) else 0
        if not n[1] and n[2] == n[3]:
            return 6 if n[3] == 1 else 11 if n[3] <= 4 and chain(3) else 0
        return 0
    if n[4] == 1 and not n[3]:
        if not n[2] and n[1] == 2:
            return 13
        if not n[1] and n[2] == 2:
            return 14
    return 0


def full_payloads_to_state(payloads):
    """uint8 [n, 11, 16] state rows of n payloads of the reference's Monte-Carlo player (server/mcts/interface.py:15-35): the
    serving payload plus hand_card {0, 1, 2}, the cards of ALL three players as rank values 3..17.  Every hand row is filled
    (its byte 15 = the number of cards listed) and every recent_handout row carries its category byte, so the rows are what a
    live table holds -- apart from ply and episode, which a payload does not say (0) -- and every kernel that reads a table
    reads them: legal lists, steps, playouts."""
    st = payloads_to_state(payloads)
    for i, p in enumerate(payloads):
        for r in range(3):
            hand = _counts(_get(p["hand_card"], r))
            st[i, F_HAND0 + r, :15] = hand
            st[i, F_HAND0 + r, 15] = hand.sum()
            st[i, F_RECENT0 + r, 15] = combo_category(st[i, F_RECENT0 + r])
    return st


def payloads_to_playout_state(payloads):
    """payloads_to_state plus the category byte of every recent_handout row (combo_category): the rows that hidden-hand
    playouts read (BatchedEnv.playout(hidden=True): own hand, taken, recent rows WITH category, the others' hand sizes) from
    the plain serving payload -- no hand_card."""
    st = payloads_to_state(payloads)
    for i in range(len(st)):
        for r in range(3):
            st[i, F_RECENT0 + r, 15] = combo_category(st[i, F_RECENT0 + r])
    return st


def state_to_full_payloads(state):
    """state_to_payloads plus hand_card {0, 1, 2}: the payload of the reference's Monte-Carlo player for every table."""
    if isinstance(state, BatchedEnv):
        state = state.state
    if torch.is_tensor(state):
        state = state.detach().cpu().numpy()
    st = np.asarray(state, np.uint8).reshape(-1, NFIELDS, ROW)
    ranks = np.arange(3, 18)
    out = state_to_payloads(st)
    for s, p in zip(st, out):
        p["hand_card"] = {r: [int(x) for x in np.repeat(ranks, s[F_HAND0 + r, :15].astype(int))] for r in range(3)}
    return out


def _payload_env(payloads, hidden, device, seed):
    """-> (env, dev): the requests as the tables of a fresh env with full slab lists -- the plain serving payloads packed by
    payloads_to_playout_state (hidden) or the full ones, with hand_card, by full_payloads_to_state"""
    n, dev = len(payloads), torch.device(device)
    env = BatchedEnv(n, seed=seed, device=dev, row_capacity=512 * n)
    st = payloads_to_playout_state(payloads) if hidden else full_payloads_to_state(payloads)
    env.state_import(torch.from_numpy(st).view(-1))
    return env, dev


def _check_domain(env, what):
    """ValueError where a table raised status bit 6 (what: the domain's name; None: nothing is asked); -> the status word"""
    status = env.status() if what else 0
    if status & STATUS_DOMAIN:
        raise ValueError(f"a payload is outside the {what} domain: cur_cards, history and left do not add up to a deck")
    return status


def _id_cards(ids, device):
    """canonical action ids -> rank lists 3..17 ([] = pass), None for -1 (no move)"""
    table = action_table(device).cpu().numpy()
    ranks = np.arange(3, 18)
    return [None if a < 0 else [int(x) for x in np.repeat(ranks, table[a, :15].astype(int))] for a in ids]


def _act(payloads, hidden, device, seed, domain, choose):
    """The frame of every *_act: the requests as a fresh env (_payload_env) -> choose(env), the ids or a tuple of tensors with the
    ids first, read back -> _check_domain -> (the ids as rank lists, the status word, choose's result as numpy); none: ([], 0, ())."""
    if not payloads:
        return [], 0, ()
    env, dev = _payload_env(payloads, hidden, device, seed)
    got = choose(env)
    host = tuple(x.cpu().numpy() for x in (got if isinstance(got, tuple) else (got,)))
    status = _check_domain(env, domain)
    return _id_cards(host[0], dev), status, host


def playout_act(payloads, n_playouts, device="cuda:0", salt=0, seed=0, hidden=False):
    """The reference's mcts(payload) (server/mcts/interface.py:15-45) as flat Monte Carlo, for a batch of requests: every
    legal move of every request is followed by n_playouts uniformly random playouts over the three known hands
    (BatchedEnv.playout_choose) and the move with the most wins for the requester's side is returned -- per request a list
    of rank values 3..17 ([] = pass), or None where the request has no move (a finished game).
    hidden=True: the payloads are the PLAIN serving payloads (no hand_card; one that is there is not read) and the playouts
    run on hands dealt from the cards the requester has not seen (playout spec v2)."""
    return _act(payloads, hidden, device, seed, "hidden-hand" if hidden else None,
                lambda env: env.playout_choose(n_playouts, salt=salt, hidden=hidden))[0]


def search_act(payloads, budget, device="cuda:0", salt=0, seed=0, hidden=False, trees=None, mode="reference", c=0.7):
    """The reference's mcts(payload) (server/mcts/interface.py:15-45) itself, for a batch of requests: a UCT tree search of
    `budget` iterations per tree from every request's state (BatchedEnv.search_choose; the reference runs 1000) and the root
    move with the best win ratio for the requester's side is returned -- per request a list of rank values 3..17 ([] =
    pass), or None where the request has no move (a finished game).
    hidden=True: the payloads are the PLAIN serving payloads (no hand_card; one that is there is not read) and tree c
    searches world c of the hands dealt from the cards the requester has not seen (`trees` determinizations)."""
    return _act(payloads, hidden, device, seed, "hidden-hand" if hidden else None,
                lambda env: env.search_choose(budget, trees=trees, mode=mode, c=c, salt=salt, hidden=hidden))[0]


def ismcts_act(payloads, budget, device="cuda:0", salt=0, seed=0, trees=None, mode="reference", c=0.7):
    """Information-set MCTS for a batch of PLAIN serving payloads (no hand_card; one that is there is not read): every
    request is packed by payloads_to_playout_state and searched by BatchedEnv.ismcts_choose (search spec v2: `trees` trees of
    `budget` iterations, each iteration on a fresh deal of the cards the requester has not seen), and the root move with the
    best win ratio for the requester's side is returned -- per request a list of rank values 3..17 ([] = pass), or None where
    the request has no move (a finished game).  ValueError where cur_cards, history and left do not add up to a deck."""
    return _act(payloads, True, device, seed, "hidden-hand",
                lambda env: env.ismcts_choose(budget, trees=trees, mode=mode, c=c, salt=salt))[0]


def guided_act(payloads, evaluator, budget, device="cuda:0", salt=0, seed=0, trees=None, mode="reference", c=0.7):
    """Guided UCT for a batch of PLAIN serving payloads (no hand_card; one that is there is not read): every request is packed
    by payloads_to_playout_state and searched by BatchedEnv.guided_choose in the hidden form (search spec v3: tree c on world
    c of the cards the requester has not seen, `budget` iterations of one launch each, every new leaf judged by `evaluator`
    -- engine.PlayoutLeaf, dqn_glue.QLeaf or any callable that fills search.values), and the root move with the best value
    for the requester's side is returned -- per request a list of rank values 3..17 ([] = pass), or None where the request
    has no move (a finished game).  ValueError where cur_cards, history and left do not add up to a deck."""
    return _act(payloads, True, device, seed, "hidden-hand",
                lambda env: env.guided_choose(evaluator, budget, trees=trees, mode=mode, c=c, salt=salt, hidden=True))[0]


def guided_puct_act(payloads, evaluator, budget, device="cuda:0", salt=0, seed=0, trees=None, c=1.25, pool=None):
    """Guided PUCT for a batch of PLAIN serving payloads (no hand_card; one that is there is not read): every request is packed
    by payloads_to_playout_state and searched by BatchedEnv.guided_puct_choose in the hidden form (search spec v5: tree c on
    world c of the cards the requester has not seen, `budget` iterations of one launch each, every new node judged by
    `evaluator` -- engine.PlayoutLeaf, dqn_glue.QLeaf or any callable that fills search.values and search.priors), and the
    root move with the most visits is returned -- per request a list of rank values 3..17 ([] = pass), or None where the
    request has no move (a finished game).  ValueError where cur_cards, history and left do not add up to a deck."""
    return _act(payloads, True, device, seed, "hidden-hand",
                lambda env: env.guided_puct_choose(evaluator, budget, trees=trees, c=c, salt=salt, hidden=True, pool=pool))[0]


def guided_ismcts_act(payloads, evaluator, budget, device="cuda:0", salt=0, seed=0, trees=None, mode="reference", c=0.7):
    """Guided ISMCTS for a batch of PLAIN serving payloads (no hand_card; one that is there is not read): every request is
    packed by payloads_to_playout_state and searched by BatchedEnv.guided_ismcts_choose (search spec v4: `trees` trees of
    `budget` iterations of one launch each, every iteration on a fresh deal of the cards the requester has not seen, every
    new leaf judged by `evaluator` as in guided_act), and the root move with the best value for the requester's side is
    returned -- per request a list of rank values 3..17 ([] = pass), or None where the request has no move (a finished
    game).  ValueError where cur_cards, history and left do not add up to a deck."""
    return _act(payloads, True, device, seed, "hidden-hand",
                lambda env: env.guided_ismcts_choose(evaluator, budget, trees=trees, mode=mode, c=c, salt=salt))[0]


def cfr_act(payloads, iterations=8, device="cuda:0", salt=0, seed=0, greedy=False):
    """The reference's final_card(payload) (server/CFR.py:520-538) for a batch of PLAIN serving payloads (no hand_card): every
    request is packed by payloads_to_playout_state, solved by BatchedEnv.cfr (CFR spec v1: `iterations` iterations of
    vanilla CFR over every deal of the cards the requester has not seen; the reference runs 8) and answered with a move
    sampled from the strategy at the requester's hand (BatchedEnv.cfr_choose: the engine's draw, keyed by the request's
    position in the batch, `seed` and `salt`; greedy: the first maximum instead).  -> per request a list of rank values
    3..17, [] for a pass.  ValueError where a request is no endgame (more than 6 cards in the three hands, or a finished
    game), where cur_cards, history and left do not add up to a deck (status bit 6), or where the solver's capacities do not
    hold it (status bit 7)."""
    if not payloads:
        return []
    moves, status, (ids,) = _act(payloads, True, device, seed, "endgame", lambda env: env.cfr_choose(
        salt=salt, greedy=greedy, solved=env.cfr(iterations, slots=len(payloads))))
    if status & STATUS_CFR_CAPACITY:
        raise ValueError("an endgame exceeds the solver's capacities")
    if (ids < 0).any():
        raise ValueError("a payload is no endgame: more than 6 cards are left, or the game is over")
    return moves


def solve_act(payloads, budget=65536, max_cards=12, worlds=1, device="cuda:0", salt=0, seed=0, hidden=False, chunks=1,
              tt_entries=4096, want_value=False):
    """The exact endgame move for a batch of requests (BatchedEnv.solve / solve_choose, solve spec v1): every legal move of
    every request is searched to the end of the game and a move that is proven to win for the requester's side is returned
    where there is one -- per request a list of rank values 3..17, [] for a pass.  want_value: -> (moves, values), values[i]
    = 1 the move is proven winning, 0 every move is proven losing, -1 neither (a search ran out of `budget`, or the worlds
    disagree).
    hidden=False: FULL payloads (with hand_card, as full_payloads_to_state reads them), solved over the three known hands.
    hidden=True: the PLAIN serving payloads (no hand_card; one that is there is not read): `worlds` deals of the cards the
    requester has not seen are solved and the move that wins in the most of them is returned (perfect-information Monte
    Carlo).  ValueError where a request is no endgame (more than max_cards cards in the three hands, or a finished game)
    or, hidden form, where cur_cards, history and left do not add up to a deck (status bit 6)."""
    if not payloads:
        return ([], []) if want_value else []
    def choose(env):
        solved = env.solve(budget, max_cards, worlds if hidden else 1, hidden, salt=salt, chunks=chunks, tt_entries=tt_entries)
        return env.solve_choose(worlds=worlds if hidden else 1, solved=solved) + (solved[0],)

    moves, _, (_, value, size) = _act(payloads, hidden, device, seed, "hidden-hand" if hidden else None, choose)
    if (size <= 0).any():
        raise ValueError(f"a payload is no endgame: more than {int(max_cards)} cards are left, or the game is over")
    return (moves, [int(v) for v in value]) if want_value else moves


class Predictor:
    """The reference's serving predictor (server/core.py:74-118 Predictor.act) for a batch of payloads, with its three-way
    switch and thresholds: the rule agent while the requester holds 12 or more cards, CFR when the three hands together hold
    6 cards or fewer, the Q-network otherwise.  Every reply is {"model": "Rule" | "CFR" | "RL1", "data": cards} (rank values
    3..17, [] = pass); the reference's `msg` string is not reproduced, and a payload without cards gets {"model": None,
    "data": []} (core.py:75-76).
      Rule  the project's batched rule agent (ddz_auto_choose, rule_based/utils/rule_based_model.py).  The reference's serving
            process imports a tuned variant of it (server/rule_utils); that variant is NOT built here.
      CFR   cfr_act (final_card).
      RL1   BatchedPredictorInputs (face + legal moves) and the greedy move of the role's QNet over them (dqn.py:61-71).
    nets: {role: QNet} for the roles 0 up / 1 lord / 2 down that may reach the RL branch (core.py:18-24 id2ai)."""

    RULE_MIN_CARDS = 12      # core.py:80
    CFR_MAX_TOTAL = 6        # core.py:88

    def __init__(self, nets, device="cuda:0", variant=3, iterations=8, seed=0):
        self.nets, self.device = nets, torch.device(device)
        self.inputs = BatchedPredictorInputs(self.device, variant)
        self.iterations, self.seed = iterations, seed

    @classmethod
    def route(cls, payload):
        """"Rule" / "CFR" / "RL1" as core.py:78-104 picks it, None for a payload without cards"""
        if not payload["cur_cards"]:
            return None
        if len(payload["cur_cards"]) >= cls.RULE_MIN_CARDS:
            return "Rule"
        if sum(int(_get(payload["left"], r)) for r in range(3)) <= cls.CFR_MAX_TOTAL:
            return "CFR"
        return "RL1"

    def act(self, payloads, salt=0, greedy=False):
        from .dqn_glue import ragged_q
        routes = [self.route(p) for p in payloads]
        out = [{"model": r, "data": []} for r in routes]
        pick = lambda name: [i for i, r in enumerate(routes) if r == name]
        rule, cfr, rl = pick("Rule"), pick("CFR"), pick("RL1")
        if rule:
            sub = [payloads[i] for i in rule]
            hands = np.zeros((len(sub), ROW), np.int8)
            lasts = np.zeros((len(sub), ROW), np.int8)
            for k, p in enumerate(sub):
                role = int(p["role_id"])
                hands[k, :15] = _counts(p["cur_cards"])
                lasts[k, :15] = _counts(_get(p["last_taken"], (role + 2) % 3) or _get(p["last_taken"], (role + 1) % 3))
            left = [[int(_get(p["left"], r)) for r in range(3)] for p in sub]
            ids = auto_choose(torch.from_numpy(hands).to(self.device), torch.from_numpy(lasts).to(self.device), left,
                              [int(p["role_id"]) for p in sub]).cpu().numpy()
            if (ids < 0).any():
                raise ValueError("the rule agent has no move for a payload (no legal combination)")
            for i, cards in zip(rule, _id_cards(ids, self.device)):
                out[i]["data"] = cards
        if cfr:
            moves = cfr_act([payloads[i] for i in cfr], self.iterations, self.device, salt=salt, seed=self.seed, greedy=greedy)
            for i, cards in zip(cfr, moves):
                out[i]["data"] = cards
        for role in sorted({int(payloads[i]["role_id"]) for i in rl}):
            idx = [i for i in rl if int(payloads[i]["role_id"]) == role]
            sub = [payloads[i] for i in idx]
            net = self.nets[role]
            with torch.no_grad():
                face = self.inputs.face(sub)
                _, offsets, rows = self.inputs.valid_actions(sub)
                q = ragged_q(net, face, rows, offsets)
            off = offsets.cpu().numpy()
            rows_h, q_h = rows.cpu().numpy(), q.cpu().numpy()
            ranks = np.arange(3, 18)
            for k, i in enumerate(idx):
                j = off[k] + int(np.argmax(q_h[off[k]:off[k + 1]]))       # torch.argmax: the first maximum (dqn.py:70)
                out[i]["data"] = [int(x) for x in np.repeat(ranks, rows_h[j, :15].astype(int))]
        return out


class BatchedPredictorInputs:
    """face / valid_actions of server/core.py's Predictor for a batch of payloads."""

    def __init__(self, device="cuda:0", variant=3):
        self.device = torch.device(device)
        self.variant = variant
        self._env = None

    def face(self, payloads):
        """f32 [n, P, 15, 4] on the device (server/core.py:44-54 for variant 3)."""
        n = len(payloads)
        if self._env is None or self._env.T != n:
            self._env = BatchedEnv(n, seed=0, device=self.device, row_capacity=max(512 * n, 512), want_ids=False)
        self._env.state_import(torch.from_numpy(payloads_to_state(payloads)).view(-1))
        return self._env.observe(self.variant)

    def valid_actions(self, payloads):
        """(last, offsets, rows): the combo each request has to beat as a rank list
        (server/core.py:57-60) and the CSR list of its legal moves (int8 rows, counts + category)."""
        hands = np.zeros((len(payloads), ROW), np.int8)
        lasts = np.zeros((len(payloads), ROW), np.int8)
        back = []
        for i, p in enumerate(payloads):
            role = int(p["role_id"])
            last = _get(p["last_taken"], (role + 2) % 3) or _get(p["last_taken"], (role + 1) % 3)
            back.append(list(last))
            hands[i, :15] = _counts(p["cur_cards"])
            lasts[i, :15] = _counts(last)
        offsets, rows, _ = get_moves(torch.from_numpy(hands).to(self.device), torch.from_numpy(lasts).to(self.device),
                                     want_ids=False)
        return back, offsets, rows
