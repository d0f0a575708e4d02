"""Exact OCHS features and the preflop EHS counts restated in numpy: what rs_ochs_round_features / rs_ehs_preflop_counts are pinned to, bit for bit.

Semantics (include/rustsolver_amd.h states the same):
  * pair_cluster[1326]: one entry per hole pair c0 < c1 at index c1 (c1 - 1) / 2 + c0, a cluster id or NO_CLUSTER = 255;
  * feature k of a hand (hole pair + board of 3, 4 or 5 cards): over every completion of the board to 5 cards from the cards the hand does not hold, and every
    opponent pair of cluster k that shares no card with the hand or the completion, W score lower, T equal, N is their count; e_k = f32(f64(2 W + T) / f64(2 N)),
    +0.0 where N == 0;
  * normalised: s = e_0 + e_1 + ... in f32 in index order, out_k = e_k / s in f32; a row with s == 0 stays all +0.0;
  * preflop counts: for a hole pair and a flop that shares no card with it, one count per completion (1081) in the bin of the river EHS; summed over the flops.
Scores come from oracle.np_br.scores7 through np_ehs.  Two forms of a river board's counts: the dense 1081 x 1081 comparison under the shares-a-card mask and the
cluster mask (the definition), and the rank-order form with per-cluster prefix counts and card removal (what whole flops are computed with)."""
import functools
import itertools

import numpy as np

import np_ehs as ne

F32 = np.float32
NO_CLUSTER = 255
MAX_CLUSTERS = 8
N_HOLE = 1326


def pair_index(c0, c1):
    """c1 (c1 - 1) / 2 + c0 for c0 < c1 (either order given; arrays welcome)"""
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    return hi * (hi - 1) // 2 + lo


@functools.lru_cache(maxsize=1)
def hole_cards():
    """[1326][2]: the cards (c0 < c1) of every hole pair, in pair_index order"""
    out = np.array([(c0, c1) for c1 in range(52) for c0 in range(c1)], dtype=np.int64)
    assert (pair_index(out[:, 0], out[:, 1]) == np.arange(N_HOLE)).all()
    return out


def preflop_class(c0, c1):
    """(high rank, low rank, suited) of a hole pair"""
    r0, r1 = int(c0) >> 2, int(c1) >> 2
    return max(r0, r1), min(r0, r1), int((int(c0) & 3) == (int(c1) & 3) and r0 != r1)


@functools.lru_cache(maxsize=1)
def preflop_classes():
    """the 169 classes in ascending (high, low, suited) order, and the class number of every hole pair [1326]"""
    keys = sorted({preflop_class(a, b) for a, b in hole_cards()})
    assert len(keys) == 169
    number = {k: i for i, k in enumerate(keys)}
    return keys, np.array([number[preflop_class(a, b)] for a, b in hole_cards()], dtype=np.int64)


def partition_of_classes(class_cluster):
    """one cluster per preflop class [169] -> pair_cluster uint8 [1326]"""
    return np.asarray(class_cluster, dtype=np.uint8)[preflop_classes()[1]]


@functools.lru_cache(maxsize=None)
def seeded_partition(seed=5):
    """the tests' partition: every class draws one of 8 clusters from PCG64(seed); cluster 7 is AA alone, the other classes that drew 7 are in no cluster"""
    keys, _ = preflop_classes()
    draw = np.random.Generator(np.random.PCG64(seed)).integers(0, MAX_CLUSTERS, size=169)
    cc = np.where(draw == 7, NO_CLUSTER, draw)
    cc[keys.index((12, 12, 0))] = 7
    out = partition_of_classes(cc)
    out.setflags(write=False)
    return out


def single_cluster():
    """every pair in cluster 0: the feature is the EHS"""
    return np.zeros(N_HOLE, dtype=np.uint8)


def aces_only():
    """AA is cluster 0 and nothing else is in a range"""
    out = np.full(N_HOLE, NO_CLUSTER, dtype=np.uint8)
    for a, b in itertools.combinations((48, 49, 50, 51), 2):
        out[pair_index(a, b)] = 0
    return out


def river_counts(board5, pair_cluster, n_clusters):
    """the definition: -> (pairs [1081][2], W [1081][n_clusters], T, N)"""
    pairs, sc = ne._scores(board5)
    cl = np.asarray(pair_cluster)[pair_index(pairs[:, 0], pairs[:, 1])]
    share = np.zeros((ne.N_PAIRS, ne.N_PAIRS), dtype=bool)
    for x in (0, 1):
        for y in (0, 1):
            share |= pairs[:, None, x] == pairs[None, :, y]
    W, T, N = (np.zeros((ne.N_PAIRS, n_clusters), dtype=np.int64) for _ in range(3))
    for k in range(n_clusters):
        opp = ~share & (cl == k)[None, :]
        W[:, k] = ((sc[None, :] < sc[:, None]) & opp).sum(axis=1)
        T[:, k] = ((sc[None, :] == sc[:, None]) & opp).sum(axis=1)
        N[:, k] = opp.sum(axis=1)
    return pairs, W, T, N


def river_counts_sorted(board5, pair_cluster, n_clusters):
    """the same by rank order: per cluster, the members below / equal among all pairs from a prefix count over the order, minus the members among the 46 pairs that hold
    the first card and the 46 that hold the second; the pair itself stands in both lists and in one cluster (taken off twice there, put back once, so it is in no count)"""
    pairs, sc = ne._scores(board5)
    cl = np.asarray(pair_cluster)[pair_index(pairs[:, 0], pairs[:, 1])]
    lists, pos = ne._card_lists()
    order = np.argsort(sc, kind="stable")
    ordered = sc[order]
    lb, ub = np.searchsorted(ordered, sc, side="left"), np.searchsorted(ordered, sc, side="right")
    member = (cl[:, None] == np.arange(n_clusters)[None, :]).astype(np.int64)                      # [1081][n_clusters], a row of zeros for a hand in no range
    ahead = np.concatenate([np.zeros((1, n_clusters), dtype=np.int64), np.cumsum(member[order], axis=0)])
    W, T, N = ahead[lb], ahead[ub] - ahead[lb] + member, ahead[-1][None, :] + member
    # the 47 x 46 (card, pair that holds it) entries under the key card << 11 | rank of the score among the board's distinct scores (fewer than 2048): a cluster's
    # entries in key order hold each card's list as one ascending run, and a pair's counts in the list of its card are differences of positions in that run
    held = lists.reshape(-1)
    sc = np.unique(sc, return_inverse=True)[1].astype(np.int64)
    key, held_cl = np.repeat(np.arange(47, dtype=np.int64), 46) << 11 | sc[held], cl[held]
    for k in range(n_clusters):
        run = np.sort(key[held_cl == k])
        for side in (0, 1):
            base = pos[:, side] << 11
            first, lo, hi, last = (np.searchsorted(run, q, side=s) for q, s in ((base, "left"), (base | sc, "left"), (base | sc, "right"), (base + (1 << 11), "left")))
            W[:, k] -= lo - first
            T[:, k] -= hi - lo
            N[:, k] -= last - first
    return pairs, W, T, N


def features_of(k2, n, normalize):
    """integers [rows][n_clusters] -> f32 [rows][n_clusters]"""
    k2, n = np.asarray(k2, dtype=np.int64), np.asarray(n, dtype=np.int64)
    e = np.zeros(k2.shape, dtype=F32)
    live = n > 0
    e[live] = (k2[live].astype(np.float64) / (2 * n[live]).astype(np.float64)).astype(F32)
    if not normalize:
        return e
    s = np.zeros(len(e), dtype=F32)
    for k in range(e.shape[1]):
        s = (s + e[:, k]).astype(F32)
    out = np.zeros_like(e)
    nz = s != 0
    out[nz] = (e[nz] / s[nz, None]).astype(F32)
    return out


@functools.lru_cache(maxsize=64)
def _board_sums(board, cluster_bytes, n_clusters, dense):
    board = list(board)
    pair_cluster = np.frombuffer(cluster_bytes, dtype=np.uint8)
    pairs = ne.hole_pairs(board)
    k2 = np.zeros((len(pairs), n_clusters), dtype=np.int64)
    n = np.zeros((len(pairs), n_clusters), dtype=np.int64)
    number = np.full((52, 52), -1, dtype=np.int64)
    number[pairs[:, 0], pairs[:, 1]] = np.arange(len(pairs))
    for extra in itertools.combinations(ne.free_cards(board), 5 - len(board)):
        rp, W, T, N = (river_counts if dense else river_counts_sorted)(board + list(extra), pair_cluster, n_clusters)
        row = number[rp[:, 0], rp[:, 1]]
        assert (row >= 0).all()
        k2[row] += 2 * W + T
        n[row] += N
    for x in (pairs, k2, n):
        x.setflags(write=False)
    return pairs, k2, n


def board_sums(board, pair_cluster, n_clusters, dense=False):
    """every hole pair of a board of 3, 4 or 5 cards (np_ehs.hole_pairs order): -> (pairs [n][2], 2 W + T [n][n_clusters], N [n][n_clusters]) summed over the
    run-outs.  Kept per (board, partition) and handed out read-only"""
    return _board_sums(tuple(int(c) for c in board), np.ascontiguousarray(pair_cluster, dtype=np.uint8).tobytes(), int(n_clusters), bool(dense))


def board_features(board, pair_cluster, n_clusters, normalize, dense=False):
    """-> (pairs [n][2], f32 [n][n_clusters])"""
    pairs, k2, n = board_sums(board, pair_cluster, n_clusters, dense)
    return pairs, features_of(k2, n, normalize)


def preflop_counts(flops, n_bins):
    """-> int64 [1326][n_bins]: for every listed flop and every hole pair off it, the completions' river-EHS bins"""
    lut = ne.bin_of_k2(n_bins)
    out = np.zeros((N_HOLE, n_bins), dtype=np.int64)
    for flop in flops:
        pairs, k2 = ne.board_counts(flop)
        rows = pair_index(pairs[:, 0], pairs[:, 1])
        for r in range(k2.shape[1]):
            live = k2[:, r] >= 0
            np.add.at(out, (rows[live], lut[k2[live, r]]), 1)
    return out
