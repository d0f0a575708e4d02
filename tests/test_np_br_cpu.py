"""CPU: the multi-round best response of the C oracle (oracle/best_response.c orc_best_response_rounds, pair loop and rank-order leaves)
against an independent reading (oracle/np_br.py: one dense deal matrix per run-out, its own hand evaluator, its own final strategy) and,
on one tiny game, against a deal-by-deal enumeration (a scalar walk per deal; it borrows the oracle's evaluator, run-out list and tree records and np_br's
final strategy, but none of their walks, weights or sums).  BR_MAX is the mode exploitability() uses; it is
discontinuous where two actions of an info set are nearly tied, so every case below also asserts that its smallest non-zero argmax margin
is far above f64 rounding -- the seeds were chosen on the CPU until np_br alone said so; nothing is skipped or filtered at run time."""
import numpy as np
import pytest

from oracle import np_br as nbr
from oracle import np_restate as npr
from oracle import orc

FLOP = [4 * 2 + 1, 4 * 3 + 1, 4 * 12 + 3]            # 4d 5d As
TURN = FLOP + [4 * 1 + 0]                            # 3c
RIVER = TURN + [4 * 11 + 3]                          # Ks, options.rs:55
RTOL, ATOL = 1e-11, 1e-12                            # two summation orders of the same f64 sums: as test_best_response_cpu.py
MARGIN = 1e-8                                        # smallest non-zero (best - runner-up) / (largest |sum| of the node): rounding is ~1e-13 of it
ODT = {"i32": orc.T_I32, "f32": orc.T_F32, "f16": orc.T_F16}
NPDT = {"i32": np.int32, "f32": np.float32, "f16": np.float16}


def combos_of(board0):
    free = [c for c in range(52) if c not in board0]
    return np.array([(a, b) for i, a in enumerate(free) for b in free[i + 1:]], dtype=np.uint8)


def pick_ranges(rng, board0, n0, n1):
    combos = combos_of(board0)
    return [combos[np.sort(rng.choice(len(combos), n, replace=False))] for n in (n0, n1)]


def disjoint_ranges(rng, board0, n0, n1):
    """hands that share no card with the board or with each other: a run-out blocks at most one of them"""
    combos = combos_of(board0)
    free = [c for c in range(52) if c not in board0]
    pairs = np.sort(rng.permutation(free)[: 2 * (n0 + n1)].reshape(-1, 2), axis=1)
    at = [int(np.flatnonzero((combos == pair).all(axis=1))[0]) for pair in pairs]
    return [combos[np.sort(at[:n0])], combos[np.sort(at[n0:])]]


def prefixes_of(board0):
    K, D = 5 - len(board0), 52 - len(board0)
    return [1, D, D * (D - 1)][: K + 1]


def random_cids(rng, board0, h, n_clusters):
    """imperfect recall on purpose: every (round, prefix, hand) draws its info set afresh; n_clusters[r] = (of player 0, of player 1)"""
    return [[rng.integers(0, n_clusters[r][p], size=(pf, len(h[p]))).astype(np.uint32) for p in (0, 1)] for r, pf in enumerate(prefixes_of(board0))]


def lane_cids(board0, h):
    """one info set per (prefix, hand): perfect information about one's own lane"""
    return [[(np.arange(pf, dtype=np.uint32)[:, None] * len(h[p]) + np.arange(len(h[p]), dtype=np.uint32)[None, :]) for p in (0, 1)] for pf in prefixes_of(board0)]


def tied_cids(rng, board0, h, first, tied):
    """the layout of test_gpu_br.multi_round_device_game(tied=...): last-round info sets that stay within `tied` run-outs (the two orders of turn and river card, and
    neighbours), turn info sets of one hand under one turn card, `first` random info sets in the first round"""
    K, D = 5 - len(board0), 52 - len(board0)
    ro = nbr.runouts(board0)
    pair = {}
    pid = np.array([pair.setdefault(tuple(sorted(int(c) for c in row[len(board0):])), len(pair)) for row in ro], dtype=np.uint32) // (tied // 2)
    cids = random_cids(rng, board0, h, [(first, first)] * (K + 1))
    cids[K] = [(pid[:, None] * len(h[p]) + np.arange(len(h[p]), dtype=np.uint32)[None, :]).astype(np.uint32) for p in (0, 1)]
    if K == 2:
        cids[1] = [(np.arange(D, dtype=np.uint32)[:, None] * len(h[p]) + np.arange(len(h[p]), dtype=np.uint32)[None, :]).astype(np.uint32) for p in (0, 1)]
    return cids


def sizes_of(cids):
    return [(int(c[0].max()) + 1, int(c[1].max()) + 1) for c in cids]


def random_sums(rng, shape, dtype, sparse):
    if dtype == "i32":
        S = rng.integers(0, 1000, shape)
    else:
        S = np.round(rng.random(shape) * 1000.0, 2)
    S[rng.random(shape) < sparse] = 0
    return S.astype(NPDT[dtype])


def fill(tb, ot, rng, dtype="i32", sparse=0.15):
    """random strategy sums on the oracle's table; returns {node index: the sums as stored}"""
    sums = {}
    for d in ot.as_dicts():
        if d["kind"] != orc.ACTION:
            continue
        S = random_sums(rng, tb.node_shape(d["index"]), dtype, sparse)
        tb.set_node(d["index"], np.zeros(S.shape), S)
        sums[d["index"]] = S
    return sums


def build(board0, bets, raises, cids, dtype="i32"):
    ot = orc.OracleTree(orc.make_options(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises))
    nodes, n_act = npr.build_tree(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises)
    assert len(nodes) == ot.n_nodes and n_act == ot.n_action_nodes
    tb = orc.OracleDealTable(ot, sizes_of(cids), dtype=ODT[dtype])
    return ot, nodes, tb


def check_margins(margins):
    """every info set's choice is either clear of rounding or cannot be seen (the tied actions are worth the same on every lane)"""
    assert margins and not any(m["visible_tie"] for m in margins)
    rel = [m["margin"] / m["scale"] for m in margins if m["margin"] > 0 and m["scale"] > 0]
    assert rel and min(rel) > MARGIN, min(rel)
    return min(rel)


def compare(board0, h, cids, bets, raises, seed, dtype="i32", sorted_too=True):
    ot, nodes, tb = build(board0, bets, raises, cids, dtype)
    sums = fill(tb, ot, np.random.Generator(np.random.PCG64(seed)), dtype)
    sig = {i: nbr.final_strategy(S) for i, S in sums.items()}
    game = nbr.Game(board0, h)
    margins = []
    want = {0: nbr.best_response(nodes, sig.__getitem__, board0, h, cids, "max", margins, game),
            1: nbr.best_response(nodes, sig.__getitem__, board0, h, cids, "avg", None, game)}
    smallest = check_margins(margins)
    for mode in (0, 1):
        got = tb.best_response_rounds(board0, h[0], h[1], cids, mode)
        assert np.allclose(got, want[mode], rtol=RTOL, atol=ATOL), (mode, got, want[mode])
        if sorted_too:
            srt = tb.best_response_rounds(board0, h[0], h[1], cids, mode | orc.BR_SORTED)
            assert np.allclose(srt, want[mode], rtol=RTOL, atol=ATOL), (mode, srt, want[mode])
    assert abs(want[1].sum()) < 1e-9 and (want[0] >= want[1] - 1e-12).all()
    return smallest


def test_scores_order_hands_as_the_oracles_evaluator_does():
    """np_br's seven-card scores are its own; only their ORDER matters (cfr.rs:326-333).  Random hands, and boards that make straights, flushes and full houses likely"""
    rng = np.random.Generator(np.random.PCG64(1))
    hands = [rng.choice(52, 7, replace=False) for _ in range(3000)]
    hands += [np.concatenate([rng.choice(4 * rng.integers(0, 9) + np.arange(20), 5, replace=False), rng.choice(np.arange(52), 2, replace=False)]) for _ in range(1500)]   # five adjacent ranks
    hands += [np.concatenate([4 * rng.choice(13, 5, replace=False) + rng.integers(0, 4), rng.choice(52, 2, replace=False)]) for _ in range(1500)]                          # one suit
    hands = np.array([x for x in hands if len(set(x.tolist())) == 7])
    mine = nbr.scores7(hands)
    theirs = np.array([orc.evaluate7(x) for x in hands], dtype=np.int64)
    a, b = rng.integers(0, len(hands), 40000), rng.integers(0, len(hands), 40000)
    assert (np.sign(mine[a] - mine[b]) == np.sign(theirs[a] - theirs[b])).all()
    assert len(set((mine >> 26).tolist())) == 9      # every category occurred


def test_final_strategy_is_infoset_rs_on_every_cell_type():
    S = np.array([[3, 0, -5, 2**31 - 1, 0], [1, 0, -1, 2**31 - 1, 7], [0, 0, -2, 1, -7]], dtype=np.int32)
    assert nbr.final_strategy(S).view(np.uint32).tolist() == npr.get_strategy(S).view(np.uint32).tolist()
    F = np.array([[3e38, np.inf, np.nan, -0.0, 1e-45], [3e38, 1.0, 2.0, 0.0, 2e-45], [1.0, np.inf, 6.0, -1.0, 0.0]], dtype=np.float32)
    sig = nbr.final_strategy(F)
    assert sig[:, 0].tolist() == [0.0, 0.0, 0.0]                                   # the sum overflowed to +inf: finite / inf
    assert np.isnan(sig[0, 1]) and sig[1, 1] == 0.0 and np.isnan(sig[2, 1])       # inf / inf, finite / inf
    assert sig[:, 2].tolist() == [0.0, 0.25, 0.75]                                 # NaN > 0 is false: the cell is not played and not summed
    assert sig[:, 3].tolist() == [np.float32(1) / np.float32(3)] * 3               # -0.0, 0.0, -1.0: no positive cell, uniform
    assert sig[:, 4].tolist() == [np.float32(1e-45) / np.float32(3e-45), np.float32(2e-45) / np.float32(3e-45), 0.0]
    H = np.array([[65504.0, np.inf], [65504.0, 1.0]], dtype=np.float16)
    assert nbr.final_strategy(H)[:, 0].tolist() == [0.5, 0.5] and np.isnan(nbr.final_strategy(H)[0, 1])   # binary16 cells add up in f32: 131008 is finite there


CASES = {
    # name: (board0, n0, n1, bet sizes, raise sizes, clusters, cell type, seed)
    "river_coarse": (RIVER, 55, 30, ((0.5, 1.0),), ((3.0,),), [(6, 9)], "i32", 11),
    "river_lanes": (RIVER, 40, 47, ((0.5, 1.0),), ((3.0,),), "lanes", "i32", 12),
    "river_big_overlap": (RIVER, 300, 280, ((0.5,),), ((),), [(40, 25)], "i32", 13),
    "turn_reference_sizes": (TURN, 60, 45, ((0.5, 1.0), (0.5, 1.0)), ((3.0,), (3.0,)), [(7, 5), (9, 12)], "i32", 14),
    "turn_lanes": (TURN, 33, 41, ((0.5,), (1.0,)), ((), ()), "lanes", "i32", 15),
    "turn_f32": (TURN, 50, 38, ((0.5,), (1.0,)), ((), ()), [(6, 4), (3, 8)], "f32", 16),
    "turn_f16": (TURN, 38, 50, ((0.5,), (1.0,)), ((), ()), [(5, 5), (7, 2)], "f16", 17),
    "turn_one_hand_p0": (TURN, 1, 40, ((0.5,), (1.0,)), ((), ()), [(1, 5), (2, 6)], "i32", 18),
    "turn_one_hand_p1": (TURN, 40, 1, ((0.5,), (1.0,)), ((), ()), [(5, 1), (6, 2)], "i32", 19),
    "flop_coarse": (FLOP, 24, 20, ((0.5,), (0.5,), (1.0,)), ((), (), ()), [(4, 3), (6, 5), (8, 7)], "i32", 20),
    "flop_tied_2": (FLOP, 14, 12, ((0.5,), (0.5,), (1.0,)), ((), (), ()), "tied2", "i32", 21),
    "flop_tied_4": (FLOP, 12, 15, ((0.5,), (0.5,), (1.0,)), ((), (), ()), "tied4", "i32", 33),
}


def make_case(name):
    board0, n0, n1, bets, raises, clusters, dtype, seed = CASES[name]
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    h = pick_ranges(rng, board0, n0, n1)
    if clusters == "lanes":
        cids = lane_cids(board0, h)
    elif isinstance(clusters, str):
        cids = tied_cids(rng, board0, h, 4, int(clusters[4:]))
    else:
        cids = random_cids(rng, board0, h, clusters)
    return board0, h, cids, bets, raises, seed, dtype


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_np_br(name):
    board0, h, cids, bets, raises, seed, dtype = make_case(name)
    if name == "river_big_overlap":
        assert len(set(map(tuple, h[0])) & set(map(tuple, h[1]))) > 20 and len(h[0]) != len(h[1])   # different ranges that overlap
    compare(board0, h, cids, bets, raises, seed, dtype)


def test_hands_without_a_compatible_opponent():
    """player 1 holds only combos with the ace of hearts; player 0's combos with that card meet no opponent at all (N1(b, h0) = 0: generate_hand would never draw
    them, cfr.rs:126-137), and the turn card blocks some of the others"""
    rng = np.random.Generator(np.random.PCG64(5))
    ah = 4 * 12 + 1
    combos = combos_of(TURN)
    with_ah = combos[(combos == ah).any(axis=1)]
    rest = combos[~(combos == ah).any(axis=1)]
    h = [np.concatenate([with_ah[:3], rest[np.sort(rng.choice(len(rest), 25, replace=False))]]), with_ah[5:9]]
    cids = random_cids(rng, TURN, h, [(4, 2), (5, 3)])
    g = nbr.Game(TURN, h)
    assert (g.W[:, :3, :] == 0).all() and 0.5 < g.W.sum() < 1.0 - 1e-3      # their share of the draws is lost, as in the C oracle (weight 0), not spread over the others
    compare(TURN, h, cids, ((0.5,), (1.0,)), ((), ()), 23)


def test_deal_weights_are_a_distribution():
    for board0, n0, n1 in ((RIVER, 30, 50), (TURN, 20, 31), (FLOP, 9, 12)):
        g = nbr.Game(board0, pick_ranges(np.random.Generator(np.random.PCG64(3)), board0, n0, n1))
        assert abs(g.W.sum() - 1.0) < 1e-12 and len(g.ro) == {5: 1, 4: 48, 3: 2352}[len(board0)]
        assert (g.ro == orc.br_runouts(board0)).all()


# ---- the third reading: deal by deal --------------------------------------------------------------------------------------------------------------

def enumerate_best_response(ot, sig, board0, h, cids, p, mode, tie="first"):
    """value of player p per deal, one scalar tree walk per deal (cfr.rs:299-349 with the opponent's final strategy in place of a sample).  BR_MAX: own nodes deepest
    first; for each the explicit sum, over every deal of an info set, of deal probability * opponent reach * value below (the deeper choices already made), then the first
    maximum (cfr.rs:684-690).  A fixed pure response is then an explicit sum over the deals."""
    nodes = ot.as_dicts()
    K, D = 5 - len(board0), 52 - len(board0)
    per_prefix = [int(np.prod([D - i for i in range(r, K)])) for r in range(K + 1)]
    ro = orc.br_runouts(board0)
    deals = []
    for b, cards in enumerate(ro):
        new = set(int(c) for c in cards[len(board0):])
        ok0 = [i for i, x in enumerate(h[0]) if not (set(map(int, x)) & new)]
        for i0 in ok0:
            used = new | set(map(int, h[0][i0]))
            ok1 = [j for j, y in enumerate(h[1]) if not (set(map(int, y)) & used)]
            s0 = orc.evaluate7(list(h[0][i0]) + list(cards))
            for i1 in ok1:
                s1 = orc.evaluate7(list(h[1][i1]) + list(cards))
                deals.append((b, (i0, i1), 1.0 / (len(ro) * len(ok0) * len(ok1)), (s0 > s1) - (s0 < s1)))
    choice = {}

    def infoset(d, b, hi):
        return int(cids[d["round_idx"]][d["player"]][b // per_prefix[d["round_idx"]], hi[d["player"]]])

    def value(i, b, hi, cmp01):
        d = nodes[i]
        if d["kind"] == orc.TERMINAL:
            pot = float(np.float32(d["value"]))
            if d["ttype"] == orc.UNCONTESTED:
                return -pot if d["last_to_act"] == p else pot
            return pot * (cmp01 if p == 0 else -cmp01)
        if d["kind"] != orc.ACTION:
            return value(d["children"][0], b, hi, cmp01)
        k = infoset(d, b, hi)
        if d["player"] == p and mode == 0:
            return value(d["children"][choice[d["index"], k]], b, hi, cmp01)
        s = sig[d["index"]][:, k]
        return sum(float(s[a]) * value(c, b, hi, cmp01) for a, c in enumerate(d["children"]) if s[a] != 0)

    def reach_to(i, b, hi):
        """the opponent's probability of playing to node i in this deal"""
        q = 1.0
        while nodes[i]["parent"] >= 0:
            par = nodes[nodes[i]["parent"]]
            if par["kind"] == orc.ACTION and par["player"] != p:
                q *= float(sig[par["index"]][par["children"].index(i), infoset(par, b, hi)])
            i = par["id"]
        return q

    if mode == 0:
        for d in reversed(nodes):                    # a node's descendants have larger ids
            if d["kind"] != orc.ACTION or d["player"] != p:
                continue
            sums = {}
            for b, hi, w, cmp01 in deals:
                q = reach_to(d["id"], b, hi)
                acc = sums.setdefault(infoset(d, b, hi), [0.0] * len(d["children"]))
                for a, c in enumerate(d["children"]):
                    acc[a] += w * q * value(c, b, hi, cmp01)
            for k, acc in sums.items():
                best = 0
                for a in range(1, len(acc)):
                    if acc[best] < acc[a] or (tie == "last" and acc[best] == acc[a]):
                        best = a
                choice[d["index"], k] = best
    return sum(w * value(0, b, hi, cmp01) for b, hi, w, cmp01 in deals)


def test_three_readings_agree_on_a_tiny_game():
    """turn start (48 run-outs), two betting rounds, 9 against 7 hands, imperfect-recall clusters of different counts for the two players: the C oracle, np_br and the
    deal-by-deal enumeration, BR_MAX and BR_AVERAGE, both players"""
    rng = np.random.Generator(np.random.PCG64(32))
    h = pick_ranges(rng, TURN, 9, 7)
    cids = random_cids(rng, TURN, h, [(5, 3), (4, 6)])
    bets, raises = ((0.5,), (1.0,)), ((), ())
    ot, nodes, tb = build(TURN, bets, raises, cids)
    assert ot.n_action_nodes > 8
    sums = fill(tb, ot, rng)
    sig = {i: nbr.final_strategy(S) for i, S in sums.items()}
    margins = []
    for mode, name in ((0, "max"), (1, "avg")):
        mine = nbr.best_response(nodes, sig.__getitem__, TURN, h, cids, name, margins if mode == 0 else None)
        theirs = tb.best_response_rounds(TURN, h[0], h[1], cids, mode)
        explicit = np.array([enumerate_best_response(ot, sig, TURN, h, cids, p, mode) for p in (0, 1)])
        assert np.allclose(mine, explicit, rtol=1e-9, atol=1e-12), (mode, mine, explicit)
        assert np.allclose(theirs, explicit, rtol=1e-9, atol=1e-12), (mode, theirs, explicit)
    check_margins(margins)


# ---- first maximum against last maximum ------------------------------------------------------------------------------------------------------------

def exact_tie_game():
    """A turn-start game whose BR_MAX value hangs on cfr.rs:686's strict <.  Player 0 holds AsAh and 7h8c, player 1 KhKc alone, one bet size per street.  Player 1's sums
    are powers of two: it checks behind always, folds to a turn bet always, calls a river bet always.  On the river player 0's two hands share ONE info set per run-out; where
    the aces win and 7h8c loses (most run-outs) check is worth (+35, -35) w and bet (+69, -69) w: both sum to 0 EXACTLY (x + -x) with different lanes.  On the turn the two
    hands are in DIFFERENT info sets, so the aces' own choice there sees +35 w per run-out after check under the first maximum and +69 w under the last one, against 35 w for
    betting (player 1 folds).  Every leaf is one product (one opponent hand), every weight the same expression in all readings: the tie is exact in each of them."""
    c = lambda t: 4 * "23456789TJQKA".index(t[0]) + "shdc".index(t[1])
    h = [np.array([[c("As"), c("Ah")], [c("7h"), c("8c")]], dtype=np.uint8), np.array([[c("Kh"), c("Kc")]], dtype=np.uint8)]
    assert len(set(np.concatenate(h).ravel().tolist()) | set(TURN)) == 10      # six hole cards and four board cards, all different
    b = np.arange(48, dtype=np.uint32)[:, None]
    cids = [[np.array([[0, 1]], dtype=np.uint32), np.array([[0]], dtype=np.uint32)], [np.repeat(b, 2, axis=1), np.zeros((48, 1), dtype=np.uint32)]]
    bets, raises = ((0.5,), (0.5,)), ((), ())
    nodes, _ = npr.build_tree(n_board_cards=4, bet_sizes=bets, raise_sizes=raises)
    sums = {}
    for nd in nodes:
        if nd["kind"] != "action":
            continue
        first = nd["actions"][0][0]
        if nd["player"] == 0:
            S = [1, 1]
        elif first == "check":
            S = [1, 0]
        else:
            S = [0, 1] if nd["round_idx"] == 0 else [1, 0]      # call / fold
        assert len(nd["actions"]) == 2
        n = [(2, 1), (48, 1)][nd["round_idx"]][nd["player"]]
        sums[nd["index"]] = np.repeat(np.array(S, dtype=np.int32)[:, None], n, axis=1)
    return TURN, h, cids, bets, raises, nodes, sums


def test_first_maximum_not_last_on_an_exact_tie():
    """the four CPU values: np_br and the enumeration under the rule give the same as the C oracle (pair loop and rank order); under the wrong rule (<= for <) both give
    a value far away -- so a reading that took the last maximum could not pass here"""
    board0, h, cids, bets, raises, nodes, sums = exact_tie_game()
    ot, nodes2, tb = build(board0, bets, raises, cids)
    for i, S in sums.items():
        tb.set_node(i, np.zeros(S.shape), S)
    sig = {i: nbr.final_strategy(S) for i, S in sums.items()}
    margins = []
    first = nbr.best_response(nodes, sig.__getitem__, board0, h, cids, "max", margins)
    last = nbr.best_response(nodes, sig.__getitem__, board0, h, cids, "max", None, None, "last")
    assert any(m["visible_tie"] and m["player"] == 0 for m in margins)
    assert last[0] > first[0] + 10.0, (first, last)                       # 69 against 35 on the aces' half of the deals
    for p in (0, 1):
        assert abs(enumerate_best_response(ot, sig, board0, h, cids, p, 0) - first[p]) < 1e-12
        assert abs(enumerate_best_response(ot, sig, board0, h, cids, p, 0, "last") - last[p]) < 1e-12
    for mode in (0, orc.BR_SORTED):
        got = tb.best_response_rounds(board0, h[0], h[1], cids, mode)
        assert np.allclose(got, first, rtol=RTOL, atol=ATOL), (mode, got, first, last)
