"""Weighted dealing (include/rustsolver_amd.h, rs_deal_weights / rs_deals_sample_weighted), restated in plain Python integers.

TEST INFRASTRUCTURE ONLY.  It imports nothing from the library: the counter hash, rand 0.7's two widening-multiply samplers, the quantisation of a row of weights,
`pick`, and both samplers are written out from the header's text.  Two conventions: every cumulative row is the inclusive prefix sum of its q row, and pick(cum, u) is
the first index i with u < cum[i].

sample_sequential / sample_joint return (the nine cards or None, info) for ONE deal; info counts `fallbacks` (players dealt by the exact branch), `attempts` (whole
attempts of the joint mode) and `words` (counters spent).  generate_hands deals a batch as uint8 [9][n], like oracle/orc.py's generate_hands."""
import math
from bisect import bisect_right

import numpy as np

M64 = (1 << 64) - 1
MAX_DRAWS = 4096      # kSampleMaxDraws: counter 4096 is the prune draw
TRIES = 32            # RS_DEAL_WEIGHTED_TRIES
DEALS = ("sequential", "joint")


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def deal_bits(seed, deal, k):
    """word k of deal `deal` under `seed`: the two-round splitmix finaliser"""
    return mix64((mix64(seed ^ (((deal + 1) * 0xD1B54A32D192ED03) & M64)) + k * 0x632BE59BD9B4E019) & M64)


def uniform52(draw32):
    """Uniform::from(0..52) on a u32 word: the card, or -1 when the word is rejected"""
    zone = 0xFFFFFFFF - (0xFFFFFFFF - 52 + 1) % 52
    wide = draw32 * 52
    return wide >> 32 if (wide & 0xFFFFFFFF) <= zone else -1


def choose_index(draw64, length):
    """gen_range(0, length) on a u64 word: zone = (length << clz(length)) - 1; -1 when rejected"""
    zone = ((length << (64 - length.bit_length())) & M64) - 1
    wide = draw64 * length
    return wide >> 64 if (wide & M64) <= zone else -1


def quanta(weights):
    """q[i] = floor(w[i] / max(w) * 2^32 + 0.5) in IEEE f64, as Python ints; None (length n) = unit weights.  ValueError where the library refuses"""
    w = [float(x) for x in weights]
    if not 1 <= len(w) <= 1326:
        raise ValueError("1..1326 hands per range")
    if any(not (x > 0.0) or math.isinf(x) for x in w):
        raise ValueError("a weight is not finite and > 0")
    m = max(w)
    q = [int(math.floor(x / m * 4294967296.0 + 0.5)) for x in w]
    if 0 in q:
        raise ValueError("a weight quantises to 0")
    return q


def cumulative(q):
    out, s = [], 0
    for x in q:
        s += int(x)
        out.append(s)
    return out


def pick(cum, u):
    return bisect_right(cum, u)


def combo(hand):
    return 1 << int(hand[0]) | 1 << int(hand[1])


def complete_board(seed, deal, board_mask, k):
    """the board cards of board_mask ascending, then the missing ones by rejection from counter k on -> (cards, used mask, k)"""
    cards = [c for c in range(52) if board_mask >> c & 1]
    used = board_mask
    while len(cards) < 5 and k < MAX_DRAWS:
        c = uniform52(deal_bits(seed, deal, k) & 0xFFFFFFFF)
        k += 1
        if c < 0 or used >> c & 1:
            continue
        cards.append(c)
        used |= 1 << c
    return cards, used, k


def sample_sequential(seed, deal, board_mask, hands, cums):
    info = dict(fallbacks=0, attempts=1, words=0)
    cards, used, k = complete_board(seed, deal, board_mask, 0)
    ok = len(cards) == 5
    for p in (0, 1):
        if not ok:
            break
        h, cum = hands[p], cums[p]
        Q = cum[-1]
        idx, tries = None, 0
        while idx is None and tries < TRIES and k < MAX_DRAWS:
            u = choose_index(deal_bits(seed, deal, k), Q)
            k += 1
            tries += 1
            if u < 0:
                continue
            i = pick(cum, u)
            if combo(h[i]) & used:
                continue
            idx = i
        if idx is None:   # the exact draw among the hands that fit
            info["fallbacks"] += 1
            q = [cum[i] - (cum[i - 1] if i else 0) for i in range(len(cum))]
            fits = [i for i in range(len(h)) if not combo(h[i]) & used]
            Z = sum(q[i] for i in fits)
            if Z:
                u = -1
                while u < 0 and k < MAX_DRAWS:
                    u = choose_index(deal_bits(seed, deal, k), Z)
                    k += 1
                run = 0
                for i in fits:
                    run += q[i]
                    if u >= 0 and run > u:
                        idx = i
                        break
        ok = idx is not None
        if ok:
            used |= combo(h[idx])
            cards += [int(h[idx][0]), int(h[idx][1])]
    info["words"] = k
    return (cards if ok else None), info


def sample_joint(seed, deal, board_mask, hands, cums):
    info = dict(fallbacks=0, attempts=0, words=0)
    k, out = 0, None
    while out is None and k < MAX_DRAWS:
        info["attempts"] += 1
        cards, used, k = complete_board(seed, deal, board_mask, k)
        if len(cards) != 5:
            break
        idx = []
        for p in (0, 1):
            u = -1
            while u < 0 and k < MAX_DRAWS:
                u = choose_index(deal_bits(seed, deal, k), cums[p][-1])
                k += 1
            if u < 0:
                break
            idx.append(pick(cums[p], u))
        if len(idx) != 2:
            break
        h0, h1 = hands[0][idx[0]], hands[1][idx[1]]
        if combo(h0) & used or combo(h1) & used or combo(h0) & combo(h1):
            continue
        out = cards + [int(h0[0]), int(h0[1]), int(h1[0]), int(h1[1])]
    info["words"] = k
    return out, info


SAMPLERS = {"sequential": sample_sequential, "joint": sample_joint}


def lowest_free_cards(board_mask):
    """what a deal that gave up writes: the board, then the lowest free cards up to nine"""
    cards = [c for c in range(52) if board_mask >> c & 1]
    return cards + [c for c in range(52) if not board_mask >> c & 1][: 9 - len(cards)]


def generate_hands(seed, first_deal, board_mask, hands0, hands1, q0, q1, deal, n_deals, stats=None, give_up="raise"):
    """deals first_deal .. first_deal + n_deals - 1 -> uint8 [9][n_deals].  q0 / q1: the quanta (None = unit weights).  stats (a dict) collects fallbacks, attempts and
    gave_up over the batch.  give_up: "raise" (RuntimeError) or "fill" (the lowest nine free cards, as the device writes)"""
    hands = [[(int(a), int(b)) for a, b in np.asarray(h).reshape(-1, 2)] for h in (hands0, hands1)]
    cums = [cumulative([1 << 32] * len(hands[p]) if q is None else q) for p, q in enumerate((q0, q1))]
    assert all(len(cums[p]) == len(hands[p]) for p in (0, 1))
    out = np.zeros((n_deals, 9), dtype=np.uint8)
    total = dict(fallbacks=0, attempts=0, gave_up=0)
    for i in range(n_deals):
        cards, info = SAMPLERS[deal](seed, first_deal + i, board_mask, hands, cums)
        total["fallbacks"] += info["fallbacks"]
        total["attempts"] += info["attempts"]
        if cards is None:
            total["gave_up"] += 1
            if give_up == "raise":
                raise RuntimeError("no valid deal for deal number %d" % (first_deal + i))
            cards = lowest_free_cards(board_mask)
        out[i] = cards
    if stats is not None:
        stats.update(total)
    return np.ascontiguousarray(out.T)
