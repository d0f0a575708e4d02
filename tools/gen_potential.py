#!/usr/bin/env python3
"""A potential-aware flop or turn bucket file (Ganzfried and Sandholm, AAAI 2014) end to end on the device: every hand of the round as the histogram of the NEXT
round's buckets over its next cards (rs_next_round_histograms), a k-means under the greedy earth mover's distance whose ground distance is the distance between the
next round's centres (rs_pa_fit over a training selection), predict over the whole round (rs_pa_predict), and the bucket file CardAbstraction reads.

    python tools/gen_ochs.py --round 3 --clusters 5000 --seed 1 --out river.dat --centers-out river.npy
    python tools/gen_potential.py --round 2 --clusters 5000 --next-buckets river.dat --next-centers river.npy --next-dist l2 --seed 1 --out turn_pa.dat

The ground distance comes from the next round's fitted centres (--next-centers with --next-dist: abstraction.ground_distances), or from a file (--ground: float32
[n_next][n_next], for a next round that is itself potential-aware).  Every draw comes from numpy's Generator(PCG64(seed)): `choice(rows, rows // train_fraction,
replace=False)` for the training set (kept in ascending row order), then `permutation(n_train)`, of which the first --clusters rows with pairwise different
contents, densified, are the initial means.  A given seed gives the same file every time.

Prints the times of the steps and the data that changed cluster per iteration; the last line is JSON.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustsolver_amd as rs  # noqa: E402
from rustsolver_amd import abstraction as ab  # noqa: E402

ROUNDS = {1: ([2, 3], [2, 4]), 2: ([2, 4], [2, 5])}   # the round's indexer, the next round's


def rows_at(rows, wanted, slice_rows=1 << 21):
    """the rows `wanted` (ascending) in one pass over the table in slices -> uint32 [len(wanted)][PA_ROW_WORDS]"""
    taken, at = np.empty((len(wanted), ab.PA_ROW_WORDS), dtype=np.uint32), 0
    for first in range(0, rows.rows, slice_rows):
        count = min(slice_rows, rows.rows - first)
        end = int(np.searchsorted(wanted, first + count))
        if end > at:
            taken[at:end] = rows.download(first, count)[wanted[at:end] - first]
        at = end
    return taken


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--round", type=int, choices=(1, 2), required=True, help="1 = flop (over turn buckets), 2 = turn (over river buckets)")
    ap.add_argument("--clusters", type=int, required=True)
    ap.add_argument("--next-buckets", required=True, help="the next round's bucket file")
    ap.add_argument("--next-centers", default=None, help=".npy float32 [n_next][bins]: the next round's fitted centres (gen_emd / gen_ochs --centers-out)")
    ap.add_argument("--next-dist", choices=("l2", "emd"), default=None, help="the distance the next round was clustered under")
    ap.add_argument("--ground", default=None, help=".npy float32 [n_next][n_next]: the ground distance itself, instead of --next-centers")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--train-fraction", type=int, default=5, help="the k-means trains on rows // this many rows")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", required=True, help="bucket file to write (refuses to overwrite)")
    ap.add_argument("--centers-out", default=None, help=".npy to write the fitted means to (refuses to overwrite)")
    args = ap.parse_args()
    if (args.ground is None) == (args.next_centers is None):
        ap.error("give --next-centers (with --next-dist) or --ground")
    if args.next_centers is not None and args.next_dist is None:
        ap.error("--next-centers needs --next-dist")
    if args.clusters < 1 or args.train_fraction < 1 or args.iterations < 1:
        ap.error("--clusters, --train-fraction and --iterations are at least 1")
    for path in (args.out, args.centers_out):
        if path and os.path.exists(path):
            raise SystemExit("gen_potential: %s exists; it is not overwritten" % path)
    if rs.device_count() < 1:
        raise SystemExit("gen_potential: no HIP device visible; the engine has no CPU fallback")
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])      # lends its device and stream
    indexer, next_indexer = ab.HandIndexer(ROUNDS[args.round][0]), ab.HandIndexer(ROUNDS[args.round][1])
    n_rows = indexer.size(1)

    t0 = time.perf_counter()
    if args.ground is not None:
        ground = np.ascontiguousarray(np.load(args.ground), dtype=np.float32)
    else:
        ground = ab.ground_distances(table, np.load(args.next_centers), ab.DIST_L2 if args.next_dist == "l2" else ab.DIST_EMD)
    if ground.ndim != 2 or ground.shape[0] != ground.shape[1] or not 1 <= ground.shape[0] <= ab.PA_MAX_NEXT:
        raise SystemExit("gen_potential: the ground distance is [n_next][n_next], n_next at most %d" % ab.PA_MAX_NEXT)
    n_next = ground.shape[0]
    next_buckets = ab.read_cluster_file(args.next_buckets)
    if len(next_buckets) != next_indexer.size(1) or int(next_buckets.max()) >= n_next:
        raise SystemExit("gen_potential: %s is not a bucket file of the next round with buckets below %d" % (args.next_buckets, n_next))
    t_ground = time.perf_counter() - t0
    print("ground: %d next-round buckets in %.3f s" % (n_next, t_ground))

    t0 = time.perf_counter()
    rows = ab.next_round_histograms(table, indexer, next_indexer, next_buckets, n_next)      # synchronises
    t_hist = time.perf_counter() - t0
    print("histograms: round %d, %d rows x %d draws in %.3f s (with the upload of the next round's buckets)" % (args.round, n_rows, rows.n_draws, t_hist))

    rng = np.random.Generator(np.random.PCG64(args.seed))
    t0 = time.perf_counter()
    train = np.sort(rng.choice(n_rows, size=max(n_rows // args.train_fraction, 1), replace=False))
    perm = rng.permutation(len(train))
    tried = np.sort(perm[:min(len(train), 4 * args.clusters)])
    contents = rows_at(rows, train[tried])
    seen, picks = set(), []
    for p in perm[:len(tried)]:
        key = contents[int(np.searchsorted(tried, p))].tobytes()
        if key not in seen:
            seen.add(key)
            picks.append(int(np.searchsorted(tried, p)))
            if len(picks) == args.clusters:
                break
    if len(picks) < args.clusters:
        raise SystemExit("gen_potential: %d different rows among the %d tried, %d clusters wanted" % (len(picks), len(tried), args.clusters))
    means = rows.dense(contents[picks], n_next)
    km = ab.PotentialKmeans(table, rows, ground)
    t_init = time.perf_counter() - t0

    t0 = time.perf_counter()
    _, means, _, changed = km.fit(means, iterations=args.iterations, sel=train.astype(np.uint32))
    t_fit = time.perf_counter() - t0
    print("fit: %d means over %d training rows, %d iterations in %.3f s, changed per iteration %s" % (args.clusters, len(train), len(changed), t_fit, changed.tolist()))

    t0 = time.perf_counter()
    clusters, dist = km.predict(means)
    t_predict = time.perf_counter() - t0
    inertia = float(dist.astype(np.float64).sum())
    used = int(len(np.unique(clusters)))
    print("predict: %d rows in %.3f s, inertia %.6f (sum of distances), %d clusters in use" % (n_rows, t_predict, inertia, used))
    ab.write_cluster_file(args.out, clusters)
    print("wrote %s: %d u32" % (args.out, len(clusters)))
    if args.centers_out:
        with open(args.centers_out, "xb") as f:
            np.save(f, means)
    print(json.dumps({"round": args.round, "clusters": args.clusters, "n_next": n_next, "seed": args.seed, "rows": n_rows, "train_rows": len(train),
                      "iterations_run": len(changed), "changed": changed.tolist(), "ground_s": t_ground, "histogram_s": t_hist, "init_s": t_init, "fit_s": t_fit,
                      "predict_s": t_predict, "inertia": inertia, "used_clusters": used}))


if __name__ == "__main__":
    main()
