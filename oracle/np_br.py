"""Best response and average-profile value of the abstracted game, second reading (numpy, one dense matrix per run-out).

TEST INFRASTRUCTURE ONLY -- PARITY UNPINNED (see oracle/rs_oracle.h).  Written from the game's definition and the Rust
source, NOT from oracle/best_response.c: it never loads librs_oracle.so, builds no lane vectors with a traverser weight
on one side and an initial reach on the other, and has no rank-order leaf.  Tests compare the C oracle with this file
(tests/test_np_br_cpu.py) and the device trainer with both (tests/test_gpu_br_pinned.py).

The game (what MCCFRTrainer plays, read as a matrix game):

  * generate_hand, cfr.rs:100-143 -- the board mask's cards in ascending order (:108-112), then 5 - n new cards drawn
    one after the other without replacement (:115-122: ORDERED, the first one is the turn of a flop start), then player
    0's combo uniformly among the combos of its range that avoid the full board, then player 1's among those of its
    range that avoid the board and player 0 (:126-137, rejection sampling).  Hence for run-out b and hands (h0, h1)
        W[b][h0][h1] = P(b) * [b, h0, h1 disjoint] / (N0(b) * N1(b, h0)),      P(b) = 1 / (D (D-1) ..), D = 52 - n.
  * leaves, cfr.rs:314-348 -- UNCONTESTED: -pot for tn.last_to_act, +pot for the other; SHOWDOWN and ALLIN alike: the
    seven-card hands on the FULL board compared, +-pot, 0 on equal scores.  S[b][h0][h1] = sign(score0 - score1).
  * chance nodes pass through (cfr.rs:306-313): a deal has one run-out, so nothing is enumerated below the root.
  * an action node of round r looks the acting player's info set up under (hole cards, board0 + the first r new cards)
    (cfr.rs:357-365): cids[r][p][prefix_r(b), hand], prefix_r(b) = b // (completions left after r new cards) with the
    run-outs enumerated first-new-card-most-significant, cards ascending among those still in the deck.  Imperfect
    recall is allowed: the ids of different rounds need not nest.
  * the opponent plays Infoset::get_final_strategy (infoset.rs:104-123) of its info set: f32, sequential sums.

For traverser p the walk carries the opponent's reach q[b][h_o] down and values v[b][h_p] up; a leaf is
v[b] = M[b] @ q[b] with M = W (fold) or W * S (showdown), transposed and negated for p = 1.  BR_MAX: at an own node
every info set plays the action whose value summed over ALL its lanes (every run-out, every hand) is largest -- first
maximum, strict < as cfr.rs:684-690.  BR_AVERAGE: the traverser plays its own final strategy.  Returned: the two
players' values per deal; (v0 + v1) / 2 under BR_MAX is the exploitability.  f64; sums in numpy's order.
"""
import numpy as np

F32 = np.float32


# ---- seven-card scores (only compared, cfr.rs:325-333): category << 26 | tie-break, standard high-card poker order --------
def _tables():
    hi = np.full(1 << 13, -1, dtype=np.int64)                  # index of the highest set bit
    top = {k: np.zeros(1 << 13, dtype=np.int64) for k in (2, 3, 5)}   # the mask with only its k highest bits kept
    straight = np.full(1 << 13, -1, dtype=np.int64)            # rank index of a straight's top card, -1: none
    for m in range(1, 1 << 13):
        bits = [i for i in range(12, -1, -1) if m >> i & 1]
        hi[m] = bits[0]
        for k in top:
            top[k][m] = sum(1 << i for i in bits[:k])
        for t in range(12, 3, -1):
            if (m >> (t - 4)) & 0x1F == 0x1F:
                straight[m] = t
                break
        else:
            if m & 0x100F == 0x100F:                           # A 2 3 4 5: the five is the top card
                straight[m] = 3
    return hi, top, straight


_HI, _TOP, _STRAIGHT = _tables()


def scores7(cards):
    """cards: integer array [N][7], card = 4 * rank + suit (cfr.rs:592) -> int64 [N], larger = stronger, equal = split"""
    c = np.asarray(cards, dtype=np.int64)
    rank, suit = c >> 2, c & 3
    n = len(c)
    cnt = np.zeros((n, 13), dtype=np.int64)
    for k in range(7):
        np.add.at(cnt, (np.arange(n), rank[:, k]), 1)
    w = (1 << np.arange(13, dtype=np.int64))[None, :]
    m1, m2, m3, m4 = [((cnt >= k) * w).sum(axis=1) for k in (1, 2, 3, 4)]
    bit = lambda r: np.where(r >= 0, 1 << np.maximum(r, 0), 0)
    fm = np.zeros(n, dtype=np.int64)                            # the ranks of a suit held five times or more (at most one)
    for s in range(4):
        ms = np.zeros(n, dtype=np.int64)
        for k in range(7):
            ms |= np.where(suit[:, k] == s, 1 << rank[:, k], 0)
        fm = np.where((suit == s).sum(axis=1) >= 5, ms, fm)
    quad, trip, p1 = _HI[m4], _HI[m3], _HI[m2]
    fh_pair = _HI[m2 & ~bit(trip)]
    p2 = _HI[m2 & ~bit(p1)]
    cat = np.zeros(n, dtype=np.int64)
    tie = _TOP[5][m1]
    pick = p1 >= 0                                              # one pair
    cat, tie = np.where(pick, 1, cat), np.where(pick, p1 << 13 | _TOP[3][m1 & ~bit(p1)], tie)
    pick = p2 >= 0                                              # two pair (a third pair's rank may be the kicker)
    cat, tie = np.where(pick, 2, cat), np.where(pick, (p1 * 13 + p2) * 13 + _HI[m1 & ~bit(p1) & ~bit(p2)], tie)
    pick = trip >= 0
    cat, tie = np.where(pick, 3, cat), np.where(pick, trip << 13 | _TOP[2][m1 & ~bit(trip)], tie)
    pick = _STRAIGHT[m1] >= 0
    cat, tie = np.where(pick, 4, cat), np.where(pick, _STRAIGHT[m1], tie)
    pick = fm > 0
    cat, tie = np.where(pick, 5, cat), np.where(pick, _TOP[5][fm], tie)
    pick = (trip >= 0) & (fh_pair >= 0)
    cat, tie = np.where(pick, 6, cat), np.where(pick, trip * 13 + fh_pair, tie)
    pick = quad >= 0
    cat, tie = np.where(pick, 7, cat), np.where(pick, quad * 13 + _HI[m1 & ~bit(quad)], tie)
    pick = (fm > 0) & (_STRAIGHT[fm] >= 0)
    cat, tie = np.where(pick, 8, cat), np.where(pick, _STRAIGHT[fm], tie)
    return cat << 26 | tie


# ---- the final strategy, infoset.rs:104-123 ------------------------------------------------------------------------------
def final_strategy(S):
    """S: [A][n] strategy sums, int32 (the reference), float32 or float16 cells -> f32 [A][n].  norm_sum is an f32 that takes
    `strategy_sum[i] as f32` in index order where strategy_sum[i] > 0 (:108-112); then strategy_sum[i] as f32 / norm_sum where
    norm_sum > 0 and the cell is positive, 0 for its other cells, 1 / n_actions where it is not (:113-121).  Float cells follow the
    same text: NaN > 0 is false, +inf > 0 is true, so inf / inf = NaN and finite / inf = 0 come out as IEEE gives them."""
    S = np.asarray(S)
    A, n = S.shape
    Sf = S.astype(np.float32)
    pos = S > 0
    norm = np.zeros(n, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(A):
            norm = np.where(pos[i], (norm + Sf[i]).astype(np.float32), norm)
        has = norm > 0
        sig = np.empty((A, n), dtype=np.float32)
        for i in range(A):
            sig[i] = np.where(has, np.where(pos[i], Sf[i] / np.where(has, norm, F32(1.0)), F32(0.0)), F32(1.0) / F32(A))
    return sig


# ---- the deal matrices ----------------------------------------------------------------------------------------------------
def runouts(board0):
    """int [NB][5]: the initial cards in the order given, then every ordered completion, first new card most significant"""
    board0 = [int(c) for c in board0]
    deck = [c for c in range(52) if c not in board0]
    K = 5 - len(board0)
    if K == 0:
        return np.array([board0], dtype=np.int64)
    if K == 1:
        return np.array([board0 + [c] for c in deck], dtype=np.int64)
    assert K == 2, "a board of 3, 4 or 5 cards"
    return np.array([board0 + [c, d] for c in deck for d in deck if d != c], dtype=np.int64)


class Game:
    """W[b][h0][h1] and S[b][h0][h1] of two ranges from an initial board, and prefix_r(b) per round"""

    def __init__(self, board0, hands):
        self.hands = [np.asarray(h, dtype=np.int64).reshape(-1, 2) for h in hands]
        self.n = [len(h) for h in self.hands]
        self.ro = runouts(board0)
        NB, n0 = len(self.ro), len(board0)
        K, D = 5 - n0, 52 - n0
        self.per_prefix = [int(np.prod([D - i for i in range(r, K)], dtype=np.int64)) for r in range(K + 1)]
        new = self.ro[:, n0:]                                                       # [NB][K]
        hit = [(h[None, :, :, None] == new[:, None, None, :]).any(axis=(2, 3)) for h in self.hands]   # [NB][n_p]: the hand holds a new card
        share = (self.hands[0][:, None, :, None] == self.hands[1][None, :, None, :]).any(axis=(2, 3))  # [n0][n1]
        ok = ~hit[0][:, :, None] & ~hit[1][:, None, :] & ~share[None, :, :]         # [NB][n0][n1]: a deal
        cnt0 = (~hit[0]).sum(axis=1).astype(np.float64)                             # N0(b)
        cnt1 = ok.sum(axis=2).astype(np.float64)                                    # N1(b, h0)
        pb = 1.0 / float(np.prod([D - i for i in range(K)], dtype=np.int64)) if K else 1.0
        self.W = np.where(ok, pb / np.maximum(cnt0[:, None, None] * cnt1[:, :, None], 1.0), 0.0)
        sc = []
        for p in (0, 1):
            c7 = np.concatenate([np.broadcast_to(self.hands[p][None, :, :], (NB, self.n[p], 2)),
                                 np.broadcast_to(self.ro[:, None, :], (NB, self.n[p], 5))], axis=2).reshape(-1, 7)
            live = ~hit[p].reshape(-1)
            s = np.zeros(len(c7), dtype=np.int64)
            s[live] = scores7(c7[live])
            sc.append(s.reshape(NB, self.n[p]))
        self.S = np.sign(sc[0][:, :, None] - sc[1][:, None, :]).astype(np.float64)
        self.blocked = hit

    def infoset_of(self, cids, r, p):
        """[NB][n_p]: the info set of every lane in round r"""
        prefix = np.arange(len(self.ro)) // self.per_prefix[r]
        return np.asarray(cids[r][p]).reshape(-1, self.n[p])[prefix].astype(np.int64)


def _leaf(M, live, q):
    """v[b][h_p] = sum over the deals (b, h_p, h_o) of M * q.  A NaN reach counts in every deal it is part of, also a tied one
    (NaN * 0 = NaN, as the Rust multiplication gives), and in no other: pairs that are no deal are not part of the sum at all."""
    bad = np.isnan(q)
    if not bad.any():
        return np.einsum("bpo,bo->bp", M, q)
    v = np.einsum("bpo,bo->bp", M, np.where(bad, 0.0, q))
    v[np.einsum("bpo,bo->bp", live, bad.astype(np.float64)) > 0] = np.nan
    return v


def best_response(nodes, sigma_bar, board0, hands, cids, mode="max", margins=None, game=None, tie="first"):
    """nodes: np_restate.build_tree's; sigma_bar(index) -> f32 [A][n_clusters of the acting player] (final_strategy of the node's
    strategy sums); hands[p]: [n_p][2]; cids[r][p]: [prefixes of round r][n_p]; mode "max" | "avg".
    margins: a list that receives, for every own info set with a lane under "max", a dict(node, player, infoset, margin, scale, visible_tie):
    margin = the chosen action's sum minus the runner-up's, scale = the largest |sum| of the node, visible_tie = the margin is 0 although
    the tied actions' lanes differ (the choice then hangs on the summation order).
    tie: "first" is the rule (cfr.rs:684-690); "last" is the WRONG rule (<= for <), there so that a test can show that a case tells the two apart."""
    g = game or Game(board0, hands)
    out = np.zeros(2)
    for p in (0, 1):
        o = 1 - p
        live = (g.W > 0).astype(np.float64)
        if p == 0:
            M_fold, M_show = g.W, g.W * g.S
        else:
            M_fold, M_show, live = g.W.transpose(0, 2, 1), -(g.W * g.S).transpose(0, 2, 1), live.transpose(0, 2, 1)
        dealt = ~g.blocked[p]

        def walk(i, q):
            nd = nodes[i]
            if nd["kind"] == "terminal":
                pot = float(np.float32(nd["value"]))                       # tn.value as f32, cfr.rs:318
                if nd["ttype"] == "UNCONTESTED":
                    return _leaf(M_fold, live, q) * (-pot if p == nd["last_to_act"] else pot)
                return _leaf(M_show, live, q) * pot
            if nd["kind"] != "action":
                return walk(nd["children"][0], q)
            sig = np.asarray(sigma_bar(nd["index"]), dtype=np.float32).astype(np.float64)
            r = nd["round_idx"]
            if nd["player"] != p:
                so = sig[:, g.infoset_of(cids, r, o)]                         # [A][NB][n_o]
                so = np.where(g.blocked[o][None, :, :], 0.0, so)              # no deal there: carries nothing
                total = 0.0
                for a, ch in enumerate(nd["children"]):
                    total = total + walk(ch, q * so[a])
                return total
            vch = np.stack([walk(ch, q) for ch in nd["children"]])            # [A][NB][n_p]
            k = g.infoset_of(cids, r, p)
            if mode != "max":
                return np.where(dealt, (sig[:, k] * vch).sum(axis=0), 0.0)
            C = sig.shape[1]
            flat = np.where(dealt, k, C).reshape(-1)                           # lanes that are no deal belong to no info set
            sums = np.stack([np.bincount(flat, weights=np.where(dealt, vch[a], 0.0).reshape(-1), minlength=C + 1)[:C] for a in range(len(vch))])
            best, best_val = np.zeros(C, dtype=np.int64), sums[0].copy()
            for a in range(1, len(vch)):                                       # cfr.rs:684-690: strict <, the first maximum stays
                m = best_val < sums[a] if tie == "first" else best_val <= sums[a]
                best[m], best_val[m] = a, sums[a][m]
            if margins is not None:
                used = np.bincount(flat, minlength=C + 1)[:C] > 0
                scale = float(np.nanmax(np.abs(sums[:, used]))) if used.any() else 0.0
                for c in np.nonzero(used)[0]:
                    others = [sums[a, c] for a in range(len(vch)) if a != best[c]]
                    margin = float(best_val[c] - max(others)) if others else float("inf")
                    seen = False
                    if margin == 0.0:
                        lanes = (k == c) & dealt
                        seen = any(sums[a, c] == best_val[c] and not np.array_equal(vch[a][lanes], vch[best[c]][lanes]) for a in range(len(vch)) if a != best[c])
                    margins.append(dict(node=nd["index"], player=p, infoset=int(c), margin=margin, scale=scale, visible_tie=seen))
            chosen = best[np.where(dealt, k, 0)]
            return np.where(dealt, np.take_along_axis(vch, chosen[None, :, :], axis=0)[0], 0.0)

        out[p] = walk(0, np.ones((len(g.ro), g.n[o]))).sum()
    return out
