"""CPU: the numpy restatement of exact EHS (tests/np_ehs.py) agrees with itself and with the reference's recorded point, rs_ehs_bin is get_bin, and the kernels of
rs_ehs.hip compile for gfx950 without scratch."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ehs as ne  # noqa: E402

from rustsolver_amd import abstraction as ab  # noqa: E402

F32 = np.float32
BROADWAY = [32, 37, 42, 47, 48]      # T J Q K A, no flush possible
PAIRED = [0, 1, 22, 35, 49]          # 2 2 7 T A
FOUR_FLUSH = [0, 8, 20, 36, 45]      # four cards of suit 0 and one of suit 1
RAINBOW = [0, 10, 20, 25, 29]        # the issue's board
ROYAL = [32, 36, 40, 44, 48]         # T J Q K A of suit 0: the board plays
ROYAL_DRAW = [32, 36, 40, 44]       # the turn board one card short of ROYAL
TURN_PAIRED = [0, 1, 22, 35]
ON_THRESHOLD_BINS = [2, 4, 5, 6, 8, 9, 10, 12, 15, 16, 18, 20, 21, 22, 30, 32, 33, 35, 36, 39, 44, 45, 51, 55, 60, 63, 64]
BOARDS = {"broadway": BROADWAY, "paired": PAIRED, "four_flush": FOUR_FLUSH, "rainbow": RAINBOW}


@pytest.mark.parametrize("name", sorted(BOARDS))
def test_the_two_forms_of_river_counts_agree(name):
    pairs, W, T = ne.river_counts(BOARDS[name])
    pairs2, W2, T2 = ne.river_counts_sorted(BOARDS[name])
    assert (pairs == pairs2).all() and (W == W2).all() and (T == T2).all()
    # the wins of one side are the losses of the other: the board's mean EHS is exactly one half
    assert W.min() >= 0 and T.min() >= 0 and (W + T <= ne.N_OPP).all() and len(W) == ne.N_PAIRS
    assert int((2 * W + T).sum()) == ne.N_PAIRS * ne.N_OPP


def test_every_pair_has_990_opponents():
    pairs, W, T = ne.river_counts(RAINBOW)
    sc = ne._scores(RAINBOW)[1]
    share = np.zeros((ne.N_PAIRS, ne.N_PAIRS), dtype=bool)
    for x in (0, 1):
        for y in (0, 1):
            share |= pairs[:, None, x] == pairs[None, :, y]
    lost = ((sc[None, :] > sc[:, None]) & ~share).sum(axis=1)
    assert ((W + T + lost) == ne.N_OPP).all()
    assert int((2 * W + T).sum()) == 1081 * 990


def test_a_board_that_plays_is_one_half_in_bin_ten_of_twenty():
    pairs, W, T = ne.river_counts(ROYAL)
    assert (W == 0).all() and (T == ne.N_OPP).all()
    v = ne.ehs_value(ne.N_OPP, 2 * ne.N_OPP)
    assert v == F32(0.5) and ne.get_bin(v, 20) == 10 and ab.ehs_bin(v, 20) == 10
    assert ne.ehs([0, 5] + ROYAL) == F32(0.5)
    assert ne.get_bin(F32(0.95), 20) == 18 and ab.ehs_bin(F32(0.95), 20) == 18


@pytest.mark.parametrize("bins", [1, 2, 7, 20, 30, 35, 50])
def test_rs_ehs_bin_is_the_literal_get_bin(bins):
    values = [F32(np.float64(k) / np.float64(1980)) for k in range(1981)] + [F32(j) / F32(bins) for j in range(bins + 1)] + [F32(0), F32(1)]
    interval, threshold = F32(1) / F32(bins), F32(1) - F32(1) / F32(bins)
    for _ in range(bins - 1):                      # the thresholds as the loop accumulates them, and their f32 neighbours
        values += [threshold, np.nextafter(threshold, F32(2)), np.nextafter(threshold, F32(-1))]
        threshold = F32(threshold - interval)
    for v in values:
        assert ab.ehs_bin(v, bins) == ne.get_bin(v, bins), (float(v), bins)
    assert (ne.bin_of_k2(bins) == [ab.ehs_bin(ne.ehs_value(k, 1980), bins) for k in range(1981)]).all()


def test_rs_ehs_bin_refuses_bin_counts_outside_the_range():
    import rustsolver_amd as rs
    for bad in (0, -1, ab.EHS_MAX_BINS + 1):
        with pytest.raises(rs.RsError):
            ab.ehs_bin(0.5, bad)
    assert ab.EHS_MAX_BINS >= 50 and ab.ehs_bin(1.0, ab.EHS_MAX_BINS) == ab.EHS_MAX_BINS - 1


def test_the_reference_point_of_ehs_rs():
    """gen_abstraction/ehs.rs holds 0.84274 from 10 000 samples for this hand; exact enumeration gives 1673 / 1980"""
    cards = [48, 49, 0, 10, 20, 25, 29]
    assert ne.river_k2(cards) == 1673
    assert ne.ehs(cards) == F32(1673 / 1980)
    pairs, W, T = ne.river_counts(cards[2:])
    p = int(np.nonzero((pairs == [48, 49]).all(axis=1))[0][0])
    assert 2 * int(W[p]) + int(T[p]) == 1673
    assert abs(0.84274 - 1673 / 1980) < 3 * np.sqrt(0.845 * 0.155 / 10000)


@pytest.mark.parametrize("bins", [1, 20, 35])
def test_histogram_rows_sum_to_one(bins):
    pairs, h = ne.board_histograms([0, 10, 20, 25], bins)
    assert h.shape == (1128, bins) and h.dtype == F32
    s = h.astype(np.float64).sum(axis=1)
    assert (np.abs(s - 1.0) <= bins * np.finfo(F32).eps).all()
    # the direct form of one hand agrees with the board's row
    p = int(np.nonzero((pairs == [48, 49]).all(axis=1))[0][0])
    assert (ne.histogram([48, 49, 0, 10, 20, 25], bins).view(np.uint32) == h[p].view(np.uint32)).all()


def test_a_suit_permutation_leaves_the_histogram_unchanged():
    perm = [2, 0, 3, 1]
    swap = lambda cards: [4 * (c >> 2) + perm[c & 3] for c in cards]
    hand = [45, 21, 0, 9, 20, 25]      # a flush draw on a two-tone turn board
    assert (ne.histogram(hand, 20).view(np.uint32) == ne.histogram(swap(hand), 20).view(np.uint32)).all()
    assert ne.ehs(hand) == ne.ehs(swap(hand))
    assert ne.ehs(hand + [30]) == ne.ehs(swap(hand + [30]))


# ---- the premises of tests/test_gpu_ehs_rounds.py, on the restatement alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [3, 4])
def test_board_by_number_is_the_combinatorial_number_system(nb):
    total = math.comb(52, nb)
    assert total == (22100 if nb == 3 else 270725)
    rng = np.random.Generator(np.random.PCG64(11))
    every = ne.round_boards(nb)
    assert every.shape == (total, nb) and len(set(map(tuple, every.tolist()))) == total
    for idx in [0, total - 1] + rng.integers(0, total, size=1000).tolist():
        c = ne.board_by_number(nb, idx)
        assert len(c) == nb and 0 <= c[0] and c[-1] < 52 and all(a < b for a, b in zip(c, c[1:])), (idx, c)
        assert sum(math.comb(c[k], k + 1) for k in range(nb)) == idx == ne.board_number(c[::-1])
        assert every[idx].tolist() == c
    assert ne.board_by_number(nb, 0) == list(range(nb)) and ne.board_by_number(nb, total - 1) == list(range(52 - nb, 52))
    assert ne.board_by_number(3, 10116) == [5, 22, 40]
    # the whole list: every number once, in order
    choose = np.array([[math.comb(c, k) for k in range(nb + 1)] for c in range(52)], dtype=np.int64)
    assert (sum(choose[every[:, k], k + 1] for k in range(nb)) == np.arange(total)).all()


def test_the_thresholds_never_fall_and_which_bin_counts_have_a_value_on_one():
    """the device bins by a binary search over the thresholds, get_bin by a downward loop: the same bin only if the thresholds are non-decreasing.  Where an attainable
    value IS a threshold, the strict > decides"""
    hit = []
    for n_bins in range(1, ab.EHS_MAX_BINS + 1):
        thr = ne.thresholds(n_bins)
        assert (np.diff(thr[1:]) >= 0).all() and (n_bins == 1 or thr[1] > 0), n_bins
        for b in range(1, n_bins):                     # the library's own thresholds are these: a value on one stays below, its f32 successor is above
            assert ab.ehs_bin(thr[b], n_bins) == ne.get_bin(thr[b], n_bins) < b
            assert ab.ehs_bin(np.nextafter(thr[b], F32(2)), n_bins) == ne.get_bin(np.nextafter(thr[b], F32(2)), n_bins) >= b
        on = ne.on_threshold(n_bins)
        for k, b in on:
            assert ne.bin_of_k2(n_bins)[k] < b <= ne.bin_of_k2(n_bins)[k + 1]
        if on:
            hit.append(n_bins)
    assert hit == ON_THRESHOLD_BINS
    assert len(ne.on_threshold(45)) == 22


def test_the_turn_boards_of_the_bin_count_sweep_reach_thresholds():
    """which (n_bins, k) pairs with f32(k / 1980) on a threshold the run-outs of the two boards produce.  The royal draw's run-out 48 puts a royal flush on the board:
    every live pair ties every opponent, 2 W + T = 990, v = 0.5, a threshold of every even bin count"""
    pairs, k2 = ne.board_counts(ROYAL_DRAW)
    tied = [r for r in range(k2.shape[1]) if (k2[:, r][k2[:, r] >= 0] == ne.N_OPP).all()]
    assert len(tied) == 1 and ne.free_cards(ROYAL_DRAW)[tied[0]] == 48 and int((k2[:, tied[0]] >= 0).sum()) == ne.N_PAIRS   # the 1081 pairs that do not hold card 48
    assert ne.ehs_value(ne.N_OPP, 2 * ne.N_OPP) == F32(0.5)
    reached = {}
    for name, board, distinct in (("royal_draw", ROYAL_DRAW, 138), ("paired", TURN_PAIRED, 288)):
        values = set(np.unique(ne.board_counts(board)[1]).tolist()) - {-1}
        assert len(values) == distinct
        reached[name] = {n: [(k, b) for k, b in ne.on_threshold(n) if k in values] for n in ON_THRESHOLD_BINS}
        reached[name] = {n: v for n, v in reached[name].items() if v}
        print(name, reached[name])
    assert sorted(reached["royal_draw"]) == [2, 4, 5, 8, 15, 16, 32, 35, 45, 64] and sorted(reached["paired"]) == [6, 15, 36, 45]
    for n in (2, 4, 8, 16, 32, 64):
        assert (ne.N_OPP, n // 2) in reached["royal_draw"][n]
    assert len(reached["royal_draw"][45]) == 4 and len(reached["paired"][45]) == 5


def test_the_words_of_a_histogram_cell():
    for n_compl in (46, 1081):
        words = ne.count_words(n_compl)
        assert len(words) == n_compl + 1 and words[0] == 0 and words[-1] == F32(1).view(np.uint32)
        k = np.arange(n_compl + 1)
        assert (ne.counts_of_words(words, n_compl) == k).all()
        near = np.concatenate([words[1:] - 1, words + 1, np.array([0xCDCDCDCD, 0x80000000, 0xFFFFFFFF, 0x7FC00000], dtype=np.uint32)])
        assert (ne.counts_of_words(near, n_compl) == -1).all()
        rng = np.random.Generator(np.random.PCG64(3))
        x = rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32)
        x[::7] = words[rng.integers(0, n_compl + 1, size=len(x[::7]))]
        by_search = np.minimum(np.searchsorted(words, x), n_compl)
        assert (ne.counts_of_words(x, n_compl) == np.where(words[by_search] == x, by_search, -1)).all()


def test_the_ehs_kernels_use_no_scratch(tmp_path):
    from rustsolver_amd import build as B

    hipcc = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    os.makedirs(os.path.join(B.HERE, "_build"), exist_ok=True)
    cmd = [hipcc] + B.FLAGS + ["-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "rs_ehs.hip"), "-o",
                               str(tmp_path / "rs_ehs.dev.o")]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", done.stdout, re.S)}
    assert sum("k_ehs" in k for k in found) == 4, sorted(found)     # the lookup form for 5, 6 and 7 cards, and the sweep
    assert all(v == 0 for v in found.values()), found


def test_gen_emd_tool_parses_its_arguments_and_fails_loudly_without_a_gpu():
    import rustsolver_amd as rs
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_emd.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(flag in r.stdout for flag in ("--round", "--clusters", "--bins", "--seed", "--out"))
    r = subprocess.run([sys.executable, tool, "--round", "3", "--clusters", "4", "--bins", "20"], capture_output=True, text=True)
    assert r.returncode == 2                                         # preflop and river are out of scope
    if rs.device_count() == 0:
        r = subprocess.run([sys.executable, tool, "--round", "1", "--clusters", "4", "--bins", "20"], capture_output=True, text=True)
        assert r.returncode != 0 and "no HIP device" in r.stderr
