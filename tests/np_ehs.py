"""Exact expected hand strength and EHS histograms restated in numpy: what rs_ehs / rs_ehs_bin / rs_ehs_round_histograms are pinned to, bit for bit.

Semantics (include/rustsolver_amd.h states the same):
  * cards are 4 * rank + suit; a hand is two hole cards followed by 3, 4 or 5 board cards;
  * an opponent hand is any two of the remaining cards, each counted once; a completion is any SET of further board cards, from what is left, that brings the board to 5;
  * river (7 cards): over the N = 990 opponent hands W have a lower score and T an equal one; ehs = f32(f64(2 W + T) / f64(2 N));
  * flop / turn (5 / 6 cards): the same formula with W, T, N summed over the 1081 / 46 completions;
  * bin: get_bin of gen_abstraction/main.rs:58-70, literally (f32 thresholds accumulated downwards, strict >);
  * histogram of a flop / turn hand: one count per completion in the bin of the river ehs; out[k] = f32(count[k]) / f32(n_completions).
Scores come from oracle.np_br.scores7 (an evaluator written independently of the device's).  Two forms of the river counts: the dense 1081 x 1081 comparison under a
shares-a-card mask (the definition), and the rank-order form with card removal (fast; what whole boards are computed with)."""
import functools
import itertools
import math

import numpy as np

from oracle.np_br import scores7

F32 = np.float32
N_OPP = 990          # C(45, 2)
N_PAIRS = 1081       # C(47, 2)


def free_cards(used):
    return [c for c in range(52) if c not in set(int(x) for x in used)]


def hole_pairs(board):
    """every two cards that are not on the board, (a, b) with a < b, ascending: int64 [n][2]"""
    return np.array(list(itertools.combinations(free_cards(board), 2)), dtype=np.int64)


def _scores(board5):
    pairs = hole_pairs(board5)
    assert len(board5) == 5 and len(pairs) == N_PAIRS
    hands = np.concatenate([pairs, np.tile(np.asarray(board5, dtype=np.int64), (N_PAIRS, 1))], axis=1)
    return pairs, scores7(hands)


def river_counts(board5):
    """the definition: -> (pairs [1081][2], W [1081], T [1081]) over the hands that share no card with the pair"""
    pairs, sc = _scores(board5)
    share = np.zeros((N_PAIRS, N_PAIRS), dtype=bool)
    for x in (0, 1):
        for y in (0, 1):
            share |= pairs[:, None, x] == pairs[None, :, y]
    W = ((sc[None, :] < sc[:, None]) & ~share).sum(axis=1)
    T = ((sc[None, :] == sc[:, None]) & ~share).sum(axis=1)
    return pairs, W, T


@functools.lru_cache(maxsize=1)
def _card_lists():
    """[47][46]: the pairs (by number) that hold the free card at each position; and [1081][2]: the two positions of every pair"""
    pos = np.array(list(itertools.combinations(range(47), 2)), dtype=np.int64)
    lists = np.array([[p for p in range(N_PAIRS) if c in pos[p]] for c in range(47)], dtype=np.int64)
    return lists, pos


def river_counts_sorted(board5):
    """the same by rank order: counts below / equal among all pairs, minus the counts among the 46 pairs that hold the first card and the 46 that hold the second;
    the pair itself has its own score and stands in both lists (so it is taken off the equal ones twice and put back once)"""
    pairs, sc = _scores(board5)
    lists, pos = _card_lists()
    ordered = np.sort(sc)
    below = np.searchsorted(ordered, sc, side="left")
    equal = np.searchsorted(ordered, sc, side="right") - below
    W, T = below.copy(), equal.copy() + 1
    for side in (0, 1):
        held = sc[lists[pos[:, side]]]              # [1081][46]
        W -= (held < sc[:, None]).sum(axis=1)
        T -= (held == sc[:, None]).sum(axis=1)
    return pairs, W, T


@functools.lru_cache(maxsize=4096)
def _river_k2(board5):
    """board5: a sorted tuple -> (2 W + T of every pair [1081], pair number by cards [52][52] (-1: not a pair of this board))"""
    pairs, W, T = river_counts_sorted(list(board5))
    pid = np.full((52, 52), -1, dtype=np.int64)
    pid[pairs[:, 0], pairs[:, 1]] = pid[pairs[:, 1], pairs[:, 0]] = np.arange(N_PAIRS)
    return 2 * W + T, pid


def ehs_value(k2, n2):
    return F32(np.float64(k2) / np.float64(n2))


def completions(cards):
    """the sets of board cards that bring the hand's board to 5"""
    return list(itertools.combinations(free_cards(cards), 7 - len(cards)))


def river_k2(cards7):
    """2 W + T of one 7-card hand, by evaluating its 990 opponents"""
    cards7 = [int(c) for c in cards7]
    opp = np.array(list(itertools.combinations(free_cards(cards7), 2)), dtype=np.int64)
    assert len(opp) == N_OPP
    so = scores7(np.concatenate([opp, np.tile(np.asarray(cards7[2:], dtype=np.int64), (N_OPP, 1))], axis=1))
    s = scores7(np.asarray([cards7], dtype=np.int64))[0]
    return 2 * int((so < s).sum()) + int((so == s).sum())


def ehs(cards):
    """cards: 5, 6 or 7 -> f32.  7 cards by direct enumeration; 5 and 6 through the rank-order form of every completed board (cached per board)"""
    cards = [int(c) for c in cards]
    assert len(cards) in (5, 6, 7) and len(set(cards)) == len(cards) and all(0 <= c < 52 for c in cards)
    if len(cards) == 7:
        return ehs_value(river_k2(cards), 2 * N_OPP)
    total, comps = 0, completions(cards)
    for extra in comps:
        k2, pid = _river_k2(tuple(sorted(cards[2:] + list(extra))))
        total += int(k2[pid[cards[0], cards[1]]])
    return ehs_value(total, 2 * N_OPP * len(comps))


def get_bin(value, bins):
    """gen_abstraction/main.rs:58-70"""
    value = F32(value)
    interval = F32(1) / F32(bins)
    b = bins - 1
    threshold = F32(1) - interval
    while b > 0:
        if value > threshold:
            return b
        b -= 1
        threshold = F32(threshold - interval)
    return 0


@functools.lru_cache(maxsize=None)
def bin_of_k2(n_bins):
    """get_bin of every value a river hand can take: [1981]"""
    return np.array([get_bin(ehs_value(k, 2 * N_OPP), n_bins) for k in range(2 * N_OPP + 1)], dtype=np.int64)


def histogram(cards, n_bins):
    """one flop or turn hand, every completion's river hand evaluated directly -> f32 [n_bins]"""
    cards = [int(c) for c in cards]
    comps = completions(cards)
    count = np.zeros(n_bins, dtype=np.int64)
    for extra in comps:
        count[get_bin(ehs_value(river_k2(cards + list(extra)), 2 * N_OPP), n_bins)] += 1
    return count.astype(F32) / F32(len(comps))


@functools.lru_cache(maxsize=64)
def _board_counts(board):
    board = list(board)
    pairs = hole_pairs(board)
    runouts = list(itertools.combinations(free_cards(board), 5 - len(board)))
    out = np.full((len(pairs), len(runouts)), -1, dtype=np.int64)
    for r, extra in enumerate(runouts):
        k2, pid = _river_k2(tuple(sorted(board + list(extra))))
        p = pid[pairs[:, 0], pairs[:, 1]]
        out[p >= 0, r] = k2[p[p >= 0]]
    pairs.setflags(write=False)
    out.setflags(write=False)
    return pairs, out


def board_counts(board):
    """every hole pair of a flop or turn board, through the rank-order form: -> (pairs [n][2], 2 W + T per run-out [n][n_runouts], -1 where the run-out takes a card of the pair).
    Kept per board (in the order its cards are given) and handed out read-only: a board shared between tests is paid for once"""
    return _board_counts(tuple(int(c) for c in board))


def board_histograms(board, n_bins):
    """-> (pairs [n][2], f32 [n][n_bins]): the histogram of every hole pair of the board (1176 on a flop, 1128 on a turn board)"""
    pairs, k2 = board_counts(board)
    lut = bin_of_k2(n_bins)
    n_compl = int((k2[0] >= 0).sum())
    assert ((k2 >= 0).sum(axis=1) == n_compl).all() and n_compl == (N_PAIRS if len(board) == 3 else 46)
    count = np.zeros((len(pairs), n_bins), dtype=np.int64)
    for r in range(k2.shape[1]):
        live = k2[:, r] >= 0
        np.add.at(count, (np.nonzero(live)[0], lut[k2[live, r]]), 1)
    return pairs, count.astype(F32) / F32(n_compl)


# ---- whole rounds: the boards by number, and the words a histogram row can hold ------------------------------------------------------------------------------------
def board_by_number(nb, idx):
    """the board with colexicographic number idx among the C(52, nb) sets of nb cards, ascending: idx = C(c0, 1) + C(c1, 2) + ... + C(c[nb-1], nb), c0 < c1 < ...
    (the combinatorial number system: the highest card is the largest c with C(c, nb) <= idx, and so on down)"""
    idx = int(idx)
    assert 0 <= idx < math.comb(52, nb)
    cards = []
    for k in range(nb, 0, -1):
        c = k - 1
        while math.comb(c + 1, k) <= idx:
            c += 1
        idx -= math.comb(c, k)
        cards.append(c)
    return cards[::-1]


def board_number(board):
    """the inverse: the cards in any order"""
    return sum(math.comb(int(c), k + 1) for k, c in enumerate(sorted(int(c) for c in board)))


@functools.lru_cache(maxsize=None)
def round_boards(nb):
    """every board of nb cards in colexicographic order (row idx is board_by_number(nb, idx)): uint8 [C(52, nb)][nb], read-only.  By the order's definition -- compare
    the highest cards first -- not by the digits"""
    b = np.array(list(itertools.combinations(range(52), nb)), dtype=np.uint8)
    b = b[np.lexsort(tuple(b[:, i] for i in range(nb)))]      # lexsort's LAST key is the primary one: the highest card
    b.setflags(write=False)
    return b


def thresholds(n_bins):
    """get_bin's thresholds as its loop accumulates them: f32 [n_bins], thr[b] for b = 1 .. n_bins - 1 is what a value must exceed to land in bin b or above; thr[0] is
    unused (bin 0 takes the rest) and set to -inf"""
    thr = np.full(n_bins, -np.inf, dtype=F32)
    interval = F32(1) / F32(n_bins)
    threshold = F32(1) - interval
    for b in range(n_bins - 1, 0, -1):
        thr[b] = threshold
        threshold = F32(threshold - interval)
    return thr


def on_threshold(n_bins):
    """the k in 0..1980 whose value f32(k / 1980) is bit-equal to one of get_bin's thresholds: [(k, b)], thr[b] the threshold hit"""
    thr = thresholds(n_bins)
    values = np.array([ehs_value(k, 2 * N_OPP) for k in range(2 * N_OPP + 1)], dtype=F32)
    return [(int(k), int(b)) for b in range(1, n_bins) for k in np.nonzero(values == thr[b])[0]]


@functools.lru_cache(maxsize=None)
def count_words(n_compl):
    """the n_compl + 1 words a histogram cell can hold, f32(k) / f32(n_compl) for k = 0 .. n_compl, as uint32: positive floats, so ascending in k as integers too"""
    w = (np.arange(n_compl + 1, dtype=F32) / F32(n_compl)).view(np.uint32)
    assert (np.diff(w.astype(np.int64)) > 0).all()
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _count_lut(n_compl):
    """count_words told apart by their high bits alone: (shift, int16 table over word >> shift; -1: no cell word starts so; the last entry takes every larger word)"""
    words = count_words(n_compl)
    shift = 31
    while len(np.unique(words >> np.uint32(shift))) < len(words):
        shift -= 1
    lut = np.full((int(words[-1]) >> shift) + 2, -1, dtype=np.int16)
    lut[words >> np.uint32(shift)] = np.arange(len(words), dtype=np.int16)
    return shift, lut


def counts_of_words(words, n_compl):
    """uint32 words of histogram rows -> the count k each holds exactly (int16, same shape); -1 where a word is none of count_words(n_compl).  A table lookup on the
    high bits finds the only candidate, the comparison of all 32 bits decides (np.searchsorted over the sorted words says the same, at ten times the cost)"""
    shift, lut = _count_lut(n_compl)
    k = lut[np.minimum(words >> np.uint32(shift), np.uint32(len(lut) - 1))]
    k[count_words(n_compl)[k] != words] = -1            # k = -1 reads the last word, 1.0, whose own high bits give n_compl: never equal here
    return k
