"""Inputs of the width, count, size, list-length and value edge cases of the k-means training loops (rs_kmeans.hip: init_s, reassign, fit_regular, fit_growbatch).
test_kmeans_cpu.py shows with the oracle alone (oracle/kmeans_fit.c) that every case reaches its edge; test_gpu_kmeans_edges.py runs the device on the same arrays.
Every case is built once per process from a fixed PCG64 seed and handed out read-only.  Nothing here touches the library or the oracle.

Contract of the inputs: finite, non-negative bins with a finite f32 sum (-0.0 counts as zero).  Non-finite bins and rows whose f32 sum overflows are no inputs:
emd_1d casts round(n_bins / factor) to an integer, which is undefined for NaN."""
import functools

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
DIST_EMD, DIST_L2 = 0, 1                       # orc.DIST_* = ab.DIST_* (include/rustsolver_amd.h)
DISTS = (DIST_EMD, DIST_L2)

WIDTHS = (1, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 63, 64)
WIDTH_ROUNDS, WIDTH_BATCH = 4, 1537
COUNT_CASES = {2: (3000, 20, 3, DISTS), 256: (3000, 20, 3, DISTS), 257: (3000, 20, 3, DISTS),      # k -> (n, n_bins, rounds, distances)
               4000: (1000, 3, 3, DISTS), 16384: (20000, 2, 1, (DIST_L2,))}                        # the oracle's init_s is k^2 distances: L2 and one round at 16 384
LIST_SIZES = (0, 1, 2, 3, 31, 32, 33, 36, 37, 38, 39, 41, 64, 65, 127, 700, 900)                   # members of the well-separated groups, one centre each
LIST_ROUNDS, LIST_BRIDGE, NO_GROUP = 3, 60, 0xffffffff
SIZES = (1, 2, 511, 512, 513, 3584, 4095, 4096, 4097)                                              # 1, 7, 8 and 9 tiles of 512
SIZE_KS = (2, 5)
SIZE_ROUNDS = 3
SIZE_BATCHES = (1, 2, 512, 513)                                                                    # of the n = 4097 case; every n also runs batch = n
LONG_N = 16384 * 256 + 5                                                                           # the grid is capped at 16 384 workgroups of 256: a second trip
COUNTER_N = 2 ** 24 + 40
VALUE_CASES = ("subnormal", "zero_rows", "neg_zero", "centre_rows", "zero_centre", "dup_centre", "emptied")
VALUE_ROUNDS = 3
REUSE = ((300, 20), (5, 63), (300, 8))                                                             # (k, n_bins) of three fits back to back on one table


def histograms(rng, n, n_bins, kind):
    """EHS-like histograms: counts out of n_samples per bin (gen_abstraction/main.rs:86-160 produces such f32 rows)"""
    if kind == "counts":
        centres = rng.random(n)[:, None] * n_bins
        width = (0.5 + 6 * rng.random(n))[:, None]
        x = np.exp(-0.5 * ((np.arange(n_bins)[None, :] - centres) / width) ** 2)
        x = np.floor(x / x.sum(axis=1, keepdims=True) * 250) / 250.0
    elif kind == "sparse":
        x = rng.random((n, n_bins)) * (rng.random((n, n_bins)) < 0.25)
    else:
        x = rng.random((n, n_bins)) ** 3
    return x.astype(np.float32)


def frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def reassign_state(rng, n, k):
    """an arbitrary state for reassign: some bounds hold, some force one distance, some a full scan -> (clusters, bounds)"""
    clusters = rng.integers(0, k, size=n).astype(np.uint32)
    bounds = np.stack([rng.random(n) * 0.3, rng.random(n) * 3.0], axis=1).astype(F32)
    bounds[::5, 1] = FLT_MAX
    return clusters, bounds


@functools.lru_cache(maxsize=None)
def width_case(n_bins):
    """n = 2003, k = 23, every 131st row zero; `centres` for the fits, `dup` (centres 7 and 2 equal: s = 0 there) and `zeroed` (centre 11 the zero
    histogram as well: under EMD every s is 0) for init_s and reassign; a reassign state over
    all data, 700 shuffled items for the reassign with an order, a shuffle for growbatch"""
    rng = _rng(1, n_bins)
    n, k = 2003, 23
    data = np.concatenate([histograms(rng, m, n_bins, kind) for m, kind in ((700, "counts"), (600, "sparse"), (703, "dense"))])[rng.permutation(n)]
    data[::131] = 0
    centres = data[rng.choice(np.nonzero((data > 0).sum(axis=1) >= min(2, n_bins))[0], size=k, replace=False)].copy()   # no zero row: under EMD it would be at distance 0 from all
    dup = centres.copy()
    dup[7] = dup[2]
    zeroed = dup.copy()
    zeroed[11] = 0                                               # the zero histogram on the datum side of init_s (emd_1d's shortcut, emd.rs:59-61)
    clusters, bounds = reassign_state(rng, n, k)
    sub = rng.permutation(n)[:700].astype(np.uint32)
    order = rng.permutation(n).astype(np.uint32)
    return frozen(data=data, centres=centres, dup=dup, zeroed=zeroed, clusters=clusters, bounds=bounds, sub=sub, order=order)


@functools.lru_cache(maxsize=None)
def count_case(k):
    """k = 2 (two_longest reads mv[1]), 256 / 257 (one and two workgroups of init_s, one and two clusters per scanning thread), 4000 > n with centres that are no
    data, 16 384 (64 KB of LDS counters)"""
    n, n_bins, rounds, dists = COUNT_CASES[k]
    rng = _rng(2, k)
    data = histograms(rng, n, n_bins, "counts" if n_bins > 3 else "dense")
    centres = data[rng.choice(n, size=k, replace=False)].copy() if k <= 257 else histograms(rng, k, n_bins, "dense")
    order = rng.permutation(n).astype(np.uint32)
    return frozen(data=data, centres=centres, order=order, batch=n - n // 3, rounds=rounds, dists=dists)


@functools.lru_cache(maxsize=None)
def lists_case():
    """member lists of chosen lengths: group g of LIST_SIZES[g] rows keeps nearly all its mass in bin g (the rest, at most 6 / 250, in the bins beside it), centre g
    is such a row too, so the first round -- a full scan of every datum -- gives list g exactly LIST_SIZES[g] members under either distance, plus, for
    the two longest, its share of LIST_BRIDGE rows that lie between their centres (group NO_GROUP).  The rows are
    shuffled, so a list's members are spread over the tiles of the counting sort.  7 bins of width would do; 17 keep one bin per group."""
    rng = _rng(3)
    k = n_bins = len(LIST_SIZES)

    def rows(g, m):
        x = np.zeros((m, n_bins))
        side = rng.integers(0, 4, size=(m, 2))
        x[:, (g - 1) % n_bins] = side[:, 0]
        x[:, (g + 1) % n_bins] = side[:, 1]
        x[:, g] = 250 - side.sum(axis=1)
        return x / 250.0

    bridge = np.zeros((LIST_BRIDGE, n_bins))                      # between the two longest lists: lower bound ~ upper bound, so these scan in every round
    bridge[:, k - 2] = rng.integers(110, 141, size=LIST_BRIDGE)
    bridge[:, k - 1] = 250 - bridge[:, k - 2]
    data = np.concatenate([rows(g, m) for g, m in enumerate(LIST_SIZES)] + [bridge / 250.0]).astype(F32)
    group = np.concatenate([np.repeat(np.arange(k), LIST_SIZES), np.full(LIST_BRIDGE, NO_GROUP)])
    perm = rng.permutation(len(data))
    data, group = data[perm], group[perm].astype(np.uint32)
    centres = np.concatenate([rows(g, 1) for g in range(k)])
    centres[k - 2, k - 2:] = 190 / 250.0, 60 / 250.0            # starts towards the bridge and takes all of it, then moves back: the bridge splits in round 2, so
    centres = centres.astype(F32)                                # both centres still move when round 3 begins
    order = rng.permutation(len(data)).astype(np.uint32)
    return frozen(data=data, centres=centres, order=order, group=group)


@functools.lru_cache(maxsize=None)
def size_case(n, k):
    """12 bins; the centres are drawn apart from the data (n may be below k)"""
    rng = _rng(4, n, k)
    data = histograms(rng, n, 12, "counts")
    centres = histograms(rng, k, 12, "counts")
    order = rng.permutation(n).astype(np.uint32)
    return frozen(data=data, centres=centres, order=order)


@functools.lru_cache(maxsize=None)
def long_case():
    """n = 16 384 x 256 + 5 rows of 2 bins, k = 3: the second trip of every grid-stride loop"""
    rng = _rng(5)
    n, k = LONG_N, 3
    data = rng.random((n, 2), dtype=F32)
    data[::1000003] = 0
    centres = np.array([[0.2, 0.7], [0.8, 0.3], [0.5, 0.5]], dtype=F32)
    clusters, bounds = reassign_state(rng, n, k)
    order = rng.permutation(n).astype(np.uint32)
    s = np.array([0.05, 0.1, 0.02], dtype=F32)
    return frozen(data=data, centres=centres, clusters=clusters, bounds=bounds, order=order, s=s)


@functools.lru_cache(maxsize=None)
def counter_case():
    """n = 2^24 + 40 rows of 1 bin, k = 2, L2: all rows but three lie in [0.75, 1.25) around centre 0 = 1.0, three (the first, one in the middle, the last but
    one) at 5.0 = centre 1.  List 0 has 2^24 + 37 members: its f32 member counter stops at 2^24"""
    rng = _rng(6)
    n = COUNTER_N
    data = (0.75 + 0.5 * rng.random((n, 1), dtype=F32)).astype(F32)
    far = np.array([0, n // 2 + 3, n - 2])
    data[far] = 5.0
    centres = np.array([[1.0], [5.0]], dtype=F32)
    return frozen(data=data, centres=centres, far=far)


@functools.lru_cache(maxsize=None)
def value_case(which):
    """12 bins, n = 3000, k = 9 centres that are data rows, plus:
    subnormal: every 7th row scaled by 1e-42; zero_rows: every 97th row zero; neg_zero: -0.0 in place of a third of the zero bins (data and centres);
    centre_rows: forty more rows that are copies of centres; zero_centre: centre 4 is the zero histogram; dup_centre / emptied: centre 5 = centre 1 (a
    strict `<` never prefers the later copy, so list 5 is empty after round 1 and centre 5 becomes the zero histogram)"""
    rng = _rng(7, VALUE_CASES.index(which))
    n, k, n_bins = 3000, 9, 12
    data = histograms(rng, n, n_bins, "counts")
    pick = rng.choice(n, size=k, replace=False)
    if which == "subnormal":
        data[::7] = (data[::7].astype(np.float64) * 1e-42).astype(F32)
        pick[0] = 7 * (pick[0] // 7)                         # one centre is a subnormal row
    if which in ("zero_rows", "neg_zero"):
        data[::97] = 0
    if which == "neg_zero":
        data[(data == 0) & (rng.random(data.shape) < 1 / 3)] = -0.0
    centres = data[pick].copy()
    if which == "centre_rows":
        data[rng.choice(n, size=40, replace=False)] = centres[rng.integers(0, k, size=40)]
    if which == "zero_centre":
        centres[4] = 0
    if which in ("dup_centre", "emptied"):
        centres[5] = centres[1]
    order = rng.permutation(n).astype(np.uint32)
    return frozen(data=data, centres=centres, order=order, batch=2000)


@functools.lru_cache(maxsize=None)
def reuse_case(i):
    """fit i of three back to back on one table: n = 3000"""
    k, n_bins = REUSE[i]
    rng = _rng(8, i)
    data = histograms(rng, 3000, n_bins, "counts")
    centres = data[rng.choice(3000, size=k, replace=False)].copy()
    order = rng.permutation(3000).astype(np.uint32)
    return frozen(data=data, centres=centres, order=order, batch=1100)


def list_facts(clusters, k, rows):
    """what the member lists of an assignment look like to k_kmeans_center_sums -> (the set of list lengths, the set of residues mod 4 of the first float of a lane's
    row, `start[c] * rows + lane * cnt`, over the lanes < rows of the lists of 36 or more members: peel + a whole 32-member body + a tail)"""
    cnt = np.bincount(clusters, minlength=k).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    residues = set()
    for c in np.nonzero(cnt >= 36)[0]:
        residues |= set(((start[c] * rows + np.arange(rows) * cnt[c]) % 4).tolist())
    return set(cnt.tolist()), residues
