#!/usr/bin/env python3
"""gen_emd (gen_abstraction/main.rs:340-381) end to end on the device: the EHS histograms of a whole round by exact enumeration
(rs_ehs_round_histograms), Kmeans::init_random's choice among restarts (rs_kmeans_pick_restart), fit_growbatch as coded, predict, and the
bucket file CardAbstraction reads.

    python tools/gen_emd.py --round 1 --clusters 500 --bins 20 --seed 1 --out means_500_round_1_emd.dat      # the reference's gen_emd(1, 500, 250, 20)
    python tools/gen_emd.py --round 2 --clusters 5000 --bins 30 --seed 1 --out means_5000_round_2_emd.dat    # its commented-out turn call

The histograms depend on the cards alone.  The k-means does not: the reference draws its candidate centers and its shuffle from thread_rng,
which nobody can replay.  Here both come from numpy's Generator(PCG64(seed)) -- `choice(n, clusters, replace=False)` per restart, then
`permutation(n)` -- which is this tool's own choice, not the reference's; a given seed gives the same file every time.

One more choice of the tool's: a cluster that the one growbatch pass leaves without members has an all-zero mean (kmeans.rs:404-415), and emd_1d
puts an empty histogram at distance 0 from everything (emd.rs:59-61), so `predict` would hand the whole round to the first such center.  The
reference's noisy histograms rarely repeat; exact ones do (a repeated candidate never wins a tie), so such a center keeps the candidate it
started from.

Prints the histogram time, 7-card evaluations per second, the k-means time, the inertia, and the whole-table checksum (the sum of all counts before
normalisation, which must be rows x completions, and the XOR of all histogram words) that profiles/ehs.md records; the last line is JSON.
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

RESTARTS, BATCH = 10, 10000          # main.rs:358, :368
ROUNDS = {1: ([2, 3], 22100, 1176, 1081), 2: ([2, 4], 270725, 48, 46)}   # indexer, boards, run-outs per board, completions per hand


def table_checksum(hist, completions, slice_rows=1 << 20):
    """-> (sum of counts, XOR of the histogram words), over slices of rows"""
    total, xor = 0, np.uint32(0)
    for first in range(0, hist.rows, slice_rows):
        x = hist.download(first, min(slice_rows, hist.rows - first))
        total += int(np.rint(x.astype(np.float64) * completions).sum())
        xor ^= np.bitwise_xor.reduce(x.view(np.uint32), axis=None)
    return total, int(xor)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--round", type=int, choices=(1, 2), required=True, help="1 = flop, 2 = turn")
    ap.add_argument("--clusters", type=int, required=True)
    ap.add_argument("--bins", type=int, required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="bucket file to write (refuses to overwrite); omitted: nothing is written")
    ap.add_argument("--centers-out", default=None, help=".npy to write the fitted centres to (refuses to overwrite): what tools/gen_potential.py --next-centers reads")
    ap.add_argument("--no-kmeans", action="store_true", help="histograms and checksum only")
    args = ap.parse_args()
    if args.centers_out and os.path.exists(args.centers_out):
        raise SystemExit("gen_emd: %s exists; it is not overwritten" % args.centers_out)
    if rs.device_count() < 1:
        raise SystemExit("gen_emd: no HIP device visible; the engine has no CPU fallback")
    cpr, n_boards, runouts, completions = ROUNDS[args.round]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])      # lends its device and stream
    indexer = ab.HandIndexer(cpr)
    rows = indexer.size(1)

    t0 = time.perf_counter()
    hist = ab.round_histograms(table, indexer, args.bins)      # synchronises
    t_hist = time.perf_counter() - t0
    evals = n_boards * runouts * 1081
    print("histograms: round %d, %d boards -> %d rows x %d bins in %.3f s (%.3e 7-card evaluations / s)" % (args.round, n_boards, rows, args.bins, t_hist, evals / t_hist))
    total, xor = table_checksum(hist, completions)
    print("checksum: counts %d (rows x completions = %d), xor 0x%08x" % (total, rows * completions, xor))
    if total != rows * completions:
        raise SystemExit("gen_emd: the counts do not add up to rows x completions")
    result = {"round": args.round, "bins": args.bins, "rows": rows, "histogram_s": t_hist, "evals_per_s": evals / t_hist, "count_sum": total, "xor": "0x%08x" % xor}

    if not args.no_kmeans:
        rng = np.random.Generator(np.random.PCG64(args.seed))
        t0 = time.perf_counter()
        km = ab.Kmeans.from_device(table, hist, rows, args.bins)
        picks = [rng.choice(rows, size=args.clusters, replace=False) for _ in range(RESTARTS)]
        candidates = np.stack([hist.gather(p) for p in picks])
        best, spread = km.pick_restart(candidates)
        order = rng.permutation(rows).astype(np.uint32)
        _, centers, _, stats = km.fit_growbatch(order, min(BATCH, rows), candidates[best])
        empty = centers.sum(axis=1) == 0
        centers[empty] = candidates[best][empty]
        clusters, dist = km.predict(centers)
        L.check(L.load().rs_sync(table._h))
        t_km = time.perf_counter() - t0
        inertia = float(dist.astype(np.float64).sum())
        used = int(len(np.unique(clusters)))
        print("k-means: %d clusters (%d left empty by the batch, %d used by predict), restart %d of %d, growbatch inertia %.6g, predict inertia %.6f (sum of distances) in %.3f s"
              % (args.clusters, int(empty.sum()), used, best, RESTARTS, stats[1], inertia, t_km))
        result.update({"clusters": args.clusters, "seed": args.seed, "kmeans_s": t_km, "inertia": inertia, "empty_after_batch": int(empty.sum()), "used_clusters": used})
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
