"""CPU: weighted dealing.  The library's host quantisation (rs_deal_weights_create / _quanta, no device needed) against the restatement in plain Python integers
(tests/np_weighted_deals.py), every refusal of the header, and the restatement's two samplers against the law the header states: counts over 65 536 deals within five
standard deviations of N * P built from the quanta, impossible cells empty; the exact fallback reached and never giving up; ranges that block each other give up.
The cases (LAW, FALLBACK) are the ones tests/test_gpu_weighted_deals.py runs on the device byte for byte."""
import numpy as np
import pytest

import np_weighted_deals as nwd
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab

# name: (board mask, hands of player 0, their weights, hands of player 1, their weights, seed, deals)
LAW = (0b11111, [(5, 6), (5, 7), (8, 9), (10, 11), (6, 12), (13, 14)], [1, .5, .25, 2, .125, 1.5], [(5, 8), (6, 7), (9, 10), (15, 16), (13, 17)], [3, 1, .5, .75, 2], 77, 65536)
FALLBACK = (0b1111, [(20, 21), (22, 23), (24, 25)], [1, 2.0**-20, 2.0**-20], [(30, 31), (20, 32), (33, 34)], [1, 2.0**-10, 1], 3, 4096)


def test_library_quanta_equal_the_restatement():
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (1, 2, 7, 300, 1326):
        w = 2.0 ** -rng.uniform(0, 20, n)
        want = nwd.quanta(w)
        got = ab.deal_quanta(w)
        assert got.dtype == np.uint64 and got.tolist() == want and max(want) == 1 << 32 and min(want) > 0
        assert ab.deal_quanta(w * 2.0**-7).tolist() == want and ab.deal_quanta(w * 2.0**40).tolist() == want    # a power of two changes no bit
        assert nwd.quanta(w * 2.0**-7) == want
        assert ab.deal_quanta(np.ones(n)).tolist() == [1 << 32] * n == nwd.quanta([1.0] * n)
        assert ab.deal_quanta(np.full(n, 0.3)).tolist() == [1 << 32] * n
        assert sum(want) < 1 << 43
    # arbitrary doubles, not powers of two; a NULL row is unit weights; both players of one object
    w0, w1 = rng.uniform(0.001, 5.0, 50), rng.uniform(1e-9, 1.0, 33)
    dw = ab.DealWeights(None, (w0, w1), (50, 33), "joint")
    assert dw.quanta(0).tolist() == nwd.quanta(w0) and dw.quanta(1).tolist() == nwd.quanta(w1)
    dw.destroy()
    dw = ab.DealWeights(None, (None, w1), (4, 33))
    assert dw.quanta(0).tolist() == [1 << 32] * 4 and dw.quanta(1).tolist() == nwd.quanta(w1)
    dw.destroy()
    # rounding to nearest, ties up: 2^-33 of the largest is the smallest weight that stays, and it becomes 1
    assert ab.deal_quanta([1.0, 2.0**-33]).tolist() == [1 << 32, 1] == nwd.quanta([1.0, 2.0**-33])
    assert ab.deal_quanta([1.0, 1.5 * 2.0**-32]).tolist() == [1 << 32, 2] == nwd.quanta([1.0, 1.5 * 2.0**-32])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 0.0, -1.0, 2.0**-34, 1e-300])
def test_weights_the_library_refuses(bad):
    w = np.array([1.0, 0.5, bad, 0.25])
    with pytest.raises(L.RsError) as e:
        ab.deal_quanta(w)
    assert e.value.code == L.ERR_INVALID
    text = L.load().rs_last_error()
    assert (b"quantises to 0" in text) if bad in (2.0**-34, 1e-300) else (b"rs_range_weights: weight 2 of player 0" in text)
    with pytest.raises(ValueError):
        nwd.quanta(w)
    with pytest.raises(L.RsError):   # ... in player 1's row as well
        ab.DealWeights(None, (None, w), (3, 4))


def test_shapes_the_library_refuses():
    for n_hands in ((0, 5), (5, 0), (1327, 5), (5, 1327)):
        with pytest.raises(L.RsError) as e:
            ab.DealWeights(None, (None, None), n_hands)
        assert e.value.code == L.ERR_INVALID and b"1..1326" in L.load().rs_last_error()
    for deal in (2, -1, 7):
        with pytest.raises(L.RsError) as e:
            ab.DealWeights(None, (None, None), (5, 5), deal)
        assert e.value.code == L.ERR_INVALID and b"RS_DEAL_SEQUENTIAL or RS_DEAL_JOINT" in L.load().rs_last_error()
    with pytest.raises(ValueError):
        ab.DealWeights(None, (np.ones(4), None), (5, 5))
    ab.DealWeights(None, (None, None), (1326, 1)).destroy()
    for name in ("rs_deal_weights_create", "rs_deal_weights_destroy", "rs_deal_weights_quanta", "rs_deals_sample_weighted", "rs_deal_trainer_set_weights"):
        assert name in L.SYMBOLS and hasattr(L.load(), name)


def law_of(case, deal):
    """P[h0][h1] from the quanta by the header's two formulas (the board is whole: P(b) = 1)"""
    mask, h0, w0, h1, w1, _, _ = case
    q0, q1 = nwd.quanta(w0), nwd.quanta(w1)
    fits0 = [not nwd.combo(a) & mask for a in h0]
    ok = np.array([[fits0[i] and not nwd.combo(b) & (mask | nwd.combo(a)) for b in h1] for i, a in enumerate(h0)])
    raw = np.where(ok, np.array(q0, dtype=np.float64)[:, None] * np.array(q1, dtype=np.float64)[None, :], 0.0)
    if deal == "joint":
        return raw / raw.sum()
    z0 = sum(q for q, f in zip(q0, fits0) if f)
    z1 = raw.sum(axis=1) / np.array(q0, dtype=np.float64)      # Z1(b, h0)
    return np.where(ok, raw / (z0 * np.where(z1 > 0, z1, 1.0))[:, None], 0.0)


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_the_restated_sampler_draws_the_law(deal):
    mask, h0, w0, h1, w1, seed, n = LAW
    P = law_of(LAW, deal)
    assert abs(P.sum() - 1.0) < 1e-12 and (P == 0).sum() == 9 and P.shape == (6, 5)
    stats = {}
    cards = nwd.generate_hands(seed, 0, mask, h0, h1, nwd.quanta(w0), nwd.quanta(w1), deal, n, stats)
    assert stats["gave_up"] == 0 and (cards[:5] == np.arange(5)[:, None]).all()
    at0 = {h: i for i, h in enumerate(h0)}
    at1 = {h: i for i, h in enumerate(h1)}
    counts = np.zeros(P.shape)
    for col in cards.T.tolist():
        counts[at0[(col[5], col[6])], at1[(col[7], col[8])]] += 1
    assert (counts[P == 0] == 0).all()
    z = (counts - n * P)[P > 0] / np.sqrt(n * P * (1 - P))[P > 0]
    print(deal, "max |z| %.2f" % np.abs(z).max(), "attempts per deal %.3f" % (stats["attempts"] / n), "fallbacks", stats["fallbacks"])
    assert (np.abs(z) <= 5.0).all(), z
    if deal == "joint":   # an attempt is accepted with probability Z / (Q0 Q1)
        q0, q1 = np.array(nwd.quanta(w0), dtype=np.float64), np.array(nwd.quanta(w1), dtype=np.float64)
        accept = (np.where(P > 0, q0[:, None] * q1[None, :], 0.0)).sum() / (q0.sum() * q1.sum())
        assert abs(stats["attempts"] / n - 1.0 / accept) < 0.02, (stats["attempts"] / n, 1.0 / accept)
    else:
        assert stats["attempts"] == n
    # the two distributions differ on this case, clearly enough for the counts to tell them apart
    other = law_of(LAW, "joint" if deal == "sequential" else "sequential")
    zo = (counts - n * other)[other > 0] / np.sqrt(n * other * (1 - other))[other > 0]
    assert np.abs(zo).max() > 5.0


def test_the_exact_fallback_is_reached_and_never_gives_up():
    mask, h0, w0, h1, w1, seed, n = FALLBACK
    stats = {}
    cards = nwd.generate_hands(seed, 0, mask, h0, h1, nwd.quanta(w0), nwd.quanta(w1), "sequential", n, stats)
    print("fallbacks", stats["fallbacks"])
    assert stats["fallbacks"] >= 1 and stats["gave_up"] == 0
    assert all(len(set(col)) == 9 for col in cards.T.tolist())
    # ... and it is exact: where the flop's fourth card takes (20, 21) away, the two light hands are even
    hit = np.isin(cards[4], (20, 21))
    light = cards[5][hit]
    assert hit.sum() > 100 and set(light.tolist()) == {22, 24}
    k = int((light == 22).sum())
    assert abs(k - len(light) / 2) <= 5 * np.sqrt(len(light) / 4)
    # without player 1's third hand some deals do not exist (the fourth card takes 30 or 31, player 0 holds 20): those give up, the others are dealt
    stats2 = {}
    nwd.generate_hands(seed, 0, mask, h0, h1[:2], nwd.quanta(w0), nwd.quanta(w1[:2]), "sequential", n, stats2, give_up="fill")
    assert stats2["gave_up"] > 0 and stats2["fallbacks"] > stats2["gave_up"]


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_ranges_that_block_each_other_give_up(deal):
    hands = [[(10, 11)], [(11, 12)]]
    cums = [[1 << 32], [1 << 32]]
    for d in range(3):
        cards, info = nwd.SAMPLERS[deal](3, d, 0b111, hands, cums)
        assert cards is None and info["words"] <= nwd.MAX_DRAWS
    with pytest.raises(RuntimeError):
        nwd.generate_hands(3, 0, 0b111, hands[0], hands[1], None, None, deal, 4)
    filled = nwd.generate_hands(3, 0, 0b111, hands[0], hands[1], None, None, deal, 4, give_up="fill")
    assert (filled == np.arange(9)[:, None]).all()
    # a board card in the only hand of player 0
    cards, _ = nwd.SAMPLERS[deal](3, 0, 0b111, [[(2, 20)], [(30, 31)]], cums)
    assert cards is None


def test_pick_on_unit_rows_is_the_uniform_index():
    """unit weights: Q = n * 2^32, so pick(cum, hi(v * Q)) = hi(v * n), the index the unweighted sampler takes from the word v (the zones differ, so the streams do)"""
    rng = np.random.Generator(np.random.PCG64(9))
    for n in (1, 7, 300, 1326):
        cum = nwd.cumulative([1 << 32] * n)
        for v in rng.integers(0, 1 << 63, 200).tolist():
            u, i = nwd.choose_index(v, cum[-1]), nwd.choose_index(v, n)
            if u >= 0 and i >= 0:
                assert nwd.pick(cum, u) == i
    assert nwd.pick([3, 3, 10], 2) == 0 and nwd.pick([3, 5, 10], 3) == 1 and nwd.pick([3, 5, 10], 9) == 2
