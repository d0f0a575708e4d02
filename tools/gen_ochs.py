#!/usr/bin/env python3
"""gen_ochs (gen_abstraction/main.rs:161-330, shipped commented out) end to end on the device: the opponent ranges from the preflop EHS histograms
(rs_ehs_preflop_counts, kmeans++ / fit_regular / predict with EMD), the OCHS feature vector of every hand of a round by exact enumeration
(rs_ochs_round_features), an L2 k-means over a fifth of the rows (Kmeans::init_random's choice among 50 restarts, fit_regular), predict over the whole
round, and the bucket file CardAbstraction reads.

    python tools/gen_ochs.py --round 3 --clusters 5000 --opp-clusters 8 --seed 1 --out round_3_ochs.dat

The features depend on the cards and the opponent partition alone.  The k-means does not: the reference draws from thread_rng, which nobody can replay.
Here every draw comes from numpy's Generator(PCG64(seed)) -- the opponent ranges' kmeans++ (abstraction.opponent_clusters), then `choice(rows, rows // 5,
replace=False)` for the training set (kept in ascending row order), then `choice(n_train, clusters, replace=False)` per restart -- which is this tool's own
choice, not the reference's; a given seed gives the same file every time.

Prints the times of the three steps, 7-card evaluations per second of the feature sweep, the XOR of all feature words (profiles/ochs.md records it), the
inertia and the clusters in use; the last line is JSON.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustsolver_amd as rs  # noqa: E402
from rustsolver_amd import _lib as L  # noqa: E402
from rustsolver_amd import abstraction as ab  # noqa: E402
from rustsolver_amd.solver import DeviceBuffer  # noqa: E402

RESTARTS, TRAIN_FRACTION, OPP_BINS = 50, 5, 35          # main.rs:306, :300-304, :164
ROUNDS = {1: ([2, 3], 1755, 1176), 2: ([2, 4], 16432, 48), 3: ([2, 5], 134459, 1)}   # indexer, suit-isomorphism classes of the boards, run-outs per board


def checksum_and_rows(feat, wanted, slice_rows=1 << 22):
    """one pass over the table in slices: -> (XOR of all feature words, the rows `wanted` (ascending) as float32 [len(wanted)][n])"""
    xor, taken, at = np.uint32(0), np.empty((len(wanted), feat.n_bins), dtype=np.float32), 0
    for first in range(0, feat.rows, slice_rows):
        x = feat.download(first, min(slice_rows, feat.rows - first))
        xor ^= np.bitwise_xor.reduce(x.view(np.uint32), axis=None)
        end = int(np.searchsorted(wanted, first + len(x)))
        taken[at:end] = x[wanted[at:end] - first]
        at = end
    return int(xor), taken


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--round", type=int, choices=(1, 2, 3), required=True, help="1 = flop, 2 = turn, 3 = river")
    ap.add_argument("--clusters", type=int, required=True)
    ap.add_argument("--opp-clusters", type=int, default=8, help="opponent ranges (1..8; the reference's n_opp_clusters is 8)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="bucket file to write (refuses to overwrite); omitted: nothing is written")
    ap.add_argument("--centers-out", default=None, help=".npy to write the fitted centres to (refuses to overwrite): what tools/gen_potential.py --next-centers reads")
    ap.add_argument("--no-kmeans", action="store_true", help="opponent ranges, features and checksum only")
    args = ap.parse_args()
    if not 1 <= args.opp_clusters <= ab.OCHS_MAX_CLUSTERS:
        ap.error("--opp-clusters must be 1..%d" % ab.OCHS_MAX_CLUSTERS)
    if args.out and os.path.exists(args.out):
        raise SystemExit("gen_ochs: %s exists; it is not overwritten" % args.out)
    if args.centers_out and os.path.exists(args.centers_out):
        raise SystemExit("gen_ochs: %s exists; it is not overwritten" % args.centers_out)
    if rs.device_count() < 1:
        raise SystemExit("gen_ochs: no HIP device visible; the engine has no CPU fallback")
    cpr, n_boards, runouts = ROUNDS[args.round]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])      # lends its device and stream
    indexer = ab.HandIndexer(cpr)
    rows = indexer.size(1)

    t0 = time.perf_counter()
    pair_cluster = ab.opponent_clusters(table, args.opp_clusters, OPP_BINS, args.seed)
    t_opp = time.perf_counter() - t0
    sizes = np.bincount(pair_cluster, minlength=args.opp_clusters).tolist()
    print("opponent ranges: %d from the preflop histograms at %d bins in %.3f s, combos per range %s" % (args.opp_clusters, OPP_BINS, t_opp, sizes))

    t0 = time.perf_counter()
    feat = ab.ochs_features(table, indexer, pair_cluster, args.opp_clusters)      # synchronises
    t_feat = time.perf_counter() - t0
    evals = n_boards * runouts * 1081
    print("features: round %d, %d boards -> %d rows x %d in %.3f s (%.3e 7-card evaluations / s)" % (args.round, n_boards, rows, args.opp_clusters, t_feat, evals / t_feat))
    result = {"round": args.round, "opp_clusters": args.opp_clusters, "seed": args.seed, "rows": rows, "range_sizes": sizes, "opponent_s": t_opp, "features_s": t_feat,
              "evals_per_s": evals / t_feat}

    rng = np.random.Generator(np.random.PCG64(args.seed + 1))
    t0 = time.perf_counter()
    wanted = np.zeros(0, dtype=np.int64) if args.no_kmeans else np.sort(rng.choice(rows, size=rows // TRAIN_FRACTION, replace=False))
    xor, train = checksum_and_rows(feat, wanted)
    t_pass = time.perf_counter() - t0
    print("checksum: xor 0x%08x (%.3f s with the training rows)" % (xor, t_pass))
    result.update({"xor": "0x%08x" % xor, "download_s": t_pass})

    if not args.no_kmeans:
        if args.clusters > len(train):
            raise SystemExit("gen_ochs: %d clusters from %d training rows" % (args.clusters, len(train)))
        t0 = time.perf_counter()
        d_train = DeviceBuffer.from_numpy(table, train)
        km = ab.Kmeans.from_device(table, d_train, len(train), args.opp_clusters)
        candidates = np.stack([train[np.sort(rng.choice(len(train), size=args.clusters, replace=False))] for _ in range(RESTARTS)])
        best, spread = km.pick_restart(candidates, ab.DIST_L2)
        _, centers, _, fit_inertia = km.fit_regular(candidates[best], ab.DIST_L2)
        d_train.free()
        clusters, dist = ab.Kmeans.from_device(table, feat, rows, args.opp_clusters).predict(centers, ab.DIST_L2)
        L.check(L.load().rs_sync(table._h))
        t_km = time.perf_counter() - t0
        inertia = float(dist.astype(np.float64).sum())
        used = int(len(np.unique(clusters)))
        print("k-means: %d clusters (%d used by predict) from %d training rows, restart %d of %d, fit inertia %.6g, predict inertia %.6f (sum of distances) in %.3f s"
              % (args.clusters, used, len(train), best, RESTARTS, fit_inertia, inertia, t_km))
        result.update({"clusters": args.clusters, "train_rows": len(train), "kmeans_s": t_km, "inertia": inertia, "used_clusters": used})
        if args.out:
            ab.write_cluster_file(args.out, clusters)
            print("wrote %s: %d u32" % (args.out, len(clusters)))
        if args.centers_out:
            with open(args.centers_out, "xb") as f:
                np.save(f, centers)
            print("wrote %s: %d centres" % (args.centers_out, len(centers)))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
