"""CPU: the numpy restatement of the exact OCHS features and the preflop counts (tests/np_ochs.py) agrees with itself and with the EHS restatement at its edges, the
kernels of rs_ochs.hip compile for gfx950 without scratch, and tools/gen_ochs.py parses its arguments."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ehs as ne  # noqa: E402
import np_ochs as no  # noqa: E402

from rustsolver_amd import abstraction as ab  # noqa: E402

F32 = np.float32
BROADWAY = [32, 37, 42, 47, 48]      # T J Q K A, no flush possible: the board plays unless a hand pairs nothing better -- every hand ties
PAIRED = [0, 1, 22, 35, 49]          # 2 2 7 T A
ACES = [48, 49, 0, 22, 35]           # two aces on the board: one AA combo is left
LOW = [4, 9, 14, 23, 31]             # 3 4 5 7 9, no ace
TURN_PAIRED = [0, 1, 22, 35]
FLOP_PAIRED = [0, 1, 20]
FLOP_LAST = [49, 50, 51]
BOARDS = {"broadway": BROADWAY, "paired": PAIRED, "aces": ACES, "low": LOW}
ROWS_WITH_AN_EMPTY_CLUSTER = {"broadway": 3, "paired": 3, "aces": 91, "low": 0}


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def test_the_seeded_partition():
    pc = no.seeded_partition()
    assert pc.shape == (1326,) and pc.dtype == np.uint8
    assert set(pc.tolist()) == set(range(8)) | {no.NO_CLUSTER}
    aces = [no.pair_index(a, b) for a in (48, 49, 50, 51) for b in (48, 49, 50, 51) if a < b]
    assert np.nonzero(pc == 7)[0].tolist() == sorted(aces) and len(aces) == 6
    assert (pc == no.NO_CLUSTER).sum() > 0
    assert ab.OCHS_MAX_CLUSTERS == no.MAX_CLUSTERS == 8 and ab.OCHS_NO_CLUSTER == no.NO_CLUSTER == 255
    cards = no.hole_cards()
    assert (ab.hole_pair_index(cards[:, 1], cards[:, 0]) == np.arange(1326)).all()
    # a partition by preflop class: the library's 169 classes are the restatement's
    rows = ab.HandIndexer([2]).get_index(cards.astype(np.uint8)).astype(np.int64)
    assert len(set(zip(rows.tolist(), no.preflop_classes()[1].tolist()))) == 169


@pytest.mark.parametrize("name", sorted(BOARDS))
def test_the_two_forms_of_the_cluster_counts_agree(name):
    pc = no.seeded_partition()
    pairs, W, T, N = no.river_counts(BOARDS[name], pc, 8)
    pairs2, W2, T2, N2 = no.river_counts_sorted(BOARDS[name], pc, 8)
    assert (pairs == pairs2).all() and (W == W2).all() and (T == T2).all() and (N == N2).all()
    assert W.min() >= 0 and T.min() >= 0 and (W + T <= N).all() and W.shape == (ne.N_PAIRS, 8)
    # the clusters partition part of the 990 opponents; all eight together with the hands in no range are np_ehs's counts
    every = no.river_counts(BOARDS[name], no.single_cluster(), 1)
    _, W1, T1 = ne.river_counts(BOARDS[name])
    assert (every[1][:, 0] == W1).all() and (every[2][:, 0] == T1).all() and (every[3] == ne.N_OPP).all()
    assert (N.sum(axis=1) < ne.N_OPP).all() and (W.sum(axis=1) <= W1).all()
    empty = int((N == 0).any(axis=1).sum())
    print("OCHS-CPU %s: rows with some N_k == 0: %d" % (name, empty))
    assert empty == ROWS_WITH_AN_EMPTY_CLUSTER[name]
    if empty:      # only AA can run out of combos: the rows are the hands that hold the aces that are left
        assert ((N == 0).sum(axis=0)[:7] == 0).all()
    raw = no.features_of(2 * W + T, N, False)
    assert (raw[N == 0] == 0).all() and not np.signbit(raw[N == 0]).any()
    if name == "broadway":
        assert (W == 0).all() and (T == N).all() and (raw[N > 0] == F32(0.5)).all()
    # the board forms (dense and by rank order) give the same rows
    a = no.board_features(BOARDS[name], pc, 8, True, dense=True)[1]
    b = no.board_features(BOARDS[name], pc, 8, True)[1]
    assert (bits(a) == bits(b)).all() and not np.isnan(a).any()


@pytest.mark.parametrize("board", [PAIRED, TURN_PAIRED, FLOP_PAIRED], ids=["river", "turn", "flop"])
def test_one_cluster_of_every_pair_is_the_ehs(board):
    pairs, got = no.board_features(board, no.single_cluster(), 1, False)
    n_compl = {5: 1, 4: 46, 3: 1081}[len(board)]
    _, k2, n = no.board_sums(board, no.single_cluster(), 1)
    assert (n == ne.N_OPP * n_compl).all()
    if len(board) == 5:
        want = np.array([ne.ehs(list(p) + board) for p in pairs], dtype=F32)
    else:
        _, per_runout = ne.board_counts(board)
        total = np.where(per_runout >= 0, per_runout, 0).sum(axis=1)
        want = np.array([ne.ehs_value(int(k), 2 * ne.N_OPP * n_compl) for k in total], dtype=F32)
        for p in range(0, len(pairs), 97):      # np_ehs.ehs itself, on a sample
            assert ne.ehs(list(pairs[p]) + board) == want[p]
    assert (bits(got[:, 0]) == bits(want)).all()


def test_a_row_of_zeros_normalises_to_zeros():
    pairs, W, T, N = no.river_counts_sorted(LOW, no.aces_only(), 1)
    assert (N[:, 0] == np.where((pairs >= 48).any(axis=1), np.where((pairs >= 48).all(axis=1), 1, 3), 6)).all()
    raw = no.features_of(2 * W + T, N, False)
    out = no.features_of(2 * W + T, N, True)
    zero = raw[:, 0] == 0
    print("OCHS-CPU zero rows on LOW against AA: %d of %d" % (zero.sum(), len(raw)))
    assert 0 < zero.sum() < len(raw)
    assert not np.isnan(out).any() and (bits(out[zero]) == 0).all() and (out[~zero] == F32(1)).all()


def test_a_suit_permutation_leaves_the_features_unchanged():
    perm = [2, 0, 3, 1]
    swap = lambda cards: [4 * (int(c) >> 2) + perm[int(c) & 3] for c in cards]
    pc = no.seeded_partition()
    for board in (PAIRED, TURN_PAIRED):
        pairs, f = no.board_features(board, pc, 8, True)
        pairs2, f2 = no.board_features(swap(board), pc, 8, True)
        row2 = {tuple(sorted(p)): r for r, p in enumerate(pairs2.tolist())}
        at = np.array([row2[tuple(sorted(swap(p)))] for p in pairs.tolist()])
        assert (bits(f) == bits(f2[at])).all()


def test_the_preflop_counts_of_two_listed_flops():
    flops = [FLOP_PAIRED, FLOP_LAST]
    counts = no.preflop_counts(flops, 20)
    assert counts.shape == (1326, 20)
    cards = no.hole_cards()
    off = np.stack([~np.isin(cards, f).any(axis=1) for f in flops], axis=1)
    assert (counts.sum(axis=1) == 1081 * off.sum(axis=1)).all()
    assert (off.sum(axis=1) == 0).sum() == 9 and (counts[off.sum(axis=1) == 0] == 0).all()      # a card of each flop
    # a row of one flop alone is the un-normalised histogram of np_ehs
    alone = no.preflop_counts([FLOP_LAST], 20)
    pairs, h = ne.board_histograms(FLOP_LAST, 20)
    assert (ne.counts_of_words(bits(h), 1081) == alone[no.pair_index(pairs[:, 0], pairs[:, 1])]).all()
    assert 21187600 == ab.PREFLOP_ROW_SUM == 10 * 2118760


def test_the_ochs_kernels_use_no_scratch(tmp_path):
    from rustsolver_amd import build as B

    hipcc = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    os.makedirs(os.path.join(B.HERE, "_build"), exist_ok=True)
    cmd = [hipcc] + B.FLAGS + ["-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "rs_ochs.hip"), "-o",
                               str(tmp_path / "rs_ochs.dev.o")]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", done.stdout, re.S)}
    assert len(found) == 2 and sum("k_ochs_round" in k for k in found) == 1 and sum("k_preflop_counts" in k for k in found) == 1, sorted(found)
    assert all(v == 0 for v in found.values()), found
    assert "rs_ochs.hip" in B.SOURCES


def test_gen_ochs_tool_parses_its_arguments_and_fails_loudly_without_a_gpu(tmp_path):
    import rustsolver_amd as rs
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_ochs.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(flag in r.stdout for flag in ("--round", "--clusters", "--opp-clusters", "--seed", "--out", "--no-kmeans"))
    for bad in (["--round", "0", "--clusters", "4"], ["--round", "3", "--clusters", "4", "--opp-clusters", "9"], ["--round", "3"]):
        r = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert r.returncode == 2, bad
    kept = tmp_path / "kept.dat"
    kept.write_bytes(b"mine")
    r = subprocess.run([sys.executable, tool, "--round", "3", "--clusters", "4", "--out", str(kept)], capture_output=True, text=True)
    assert r.returncode != 0 and "not overwritten" in r.stderr and kept.read_bytes() == b"mine"
    if rs.device_count() == 0:
        r = subprocess.run([sys.executable, tool, "--round", "3", "--clusters", "4"], capture_output=True, text=True)
        assert r.returncode != 0 and "no HIP device" in r.stderr
