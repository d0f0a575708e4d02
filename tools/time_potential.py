#!/usr/bin/env python3
"""Times the potential-aware abstraction's two device steps (profiles/potential.md): the next-round histogram sweep of a whole round over a synthetic bucket file,
and one assignment pass (rs_pa_predict) of its rows against means that are each the mean of 32 random rows, under the L2 distances of random next-round centres.

    python tools/time_potential.py --round 1 --next 500 --means 500
    python tools/time_potential.py --round 2 --next 500,1000,2000,5000 --means 500,1000,2000,5000 --budget 120

For every (next, means) setting the pass is timed on about 50 000 evenly spaced rows first; the whole round is assigned only when that projects to at most --budget seconds.
One JSON line per measurement.
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

ROUNDS = {1: ([2, 3], [2, 4]), 2: ([2, 4], [2, 5])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--round", type=int, choices=(1, 2), required=True)
    ap.add_argument("--next", default="500", help="next-round bucket counts, comma separated")
    ap.add_argument("--means", default="500", help="means per setting, comma separated (paired with --next)")
    ap.add_argument("--budget", type=float, default=60.0, help="seconds a whole-round pass may be projected to take")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    settings = list(zip([int(x) for x in args.next.split(",")], [int(x) for x in args.means.split(",")]))
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])
    indexer, next_indexer = ab.HandIndexer(ROUNDS[args.round][0]), ab.HandIndexer(ROUNDS[args.round][1])
    index = np.arange(next_indexer.size(1), dtype=np.uint64)
    mixed = (index * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    for n_next, n_means in settings:
        rng = np.random.Generator(np.random.PCG64(args.seed))
        buckets = (mixed % np.uint64(n_next)).astype(np.uint32)
        ab.next_round_histograms(table, indexer, next_indexer, buckets, n_next).buffer.free()      # the indexers' tables and the kernel are on the device
        t0 = time.perf_counter()
        rows = ab.next_round_histograms(table, indexer, next_indexer, buckets, n_next)
        t_hist = time.perf_counter() - t0
        print(json.dumps({"step": "histograms", "round": args.round, "n_next": n_next, "rows": rows.rows, "seconds_with_the_bucket_upload": t_hist}), flush=True)
        points = rng.random((n_next, 8)).astype(np.float32)
        ground = ab.ground_distances(table, points, ab.DIST_L2)
        picks = np.sort(rng.choice(rows.rows, size=32 * n_means, replace=False))
        taken = np.concatenate([rows.download(int(p), 1) for p in picks])
        means = rows.dense(taken, n_next).reshape(n_means, 32, n_next).astype(np.float64).mean(axis=1).astype(np.float32)
        km = ab.PotentialKmeans(table, rows, ground)
        sel = np.arange(0, rows.rows, max(rows.rows // 50000, 1), dtype=np.uint32)      # enough waves to fill the device
        km.predict(means, sel=sel[:64])
        t0 = time.perf_counter()
        km.predict(means, sel=sel)
        t_part = time.perf_counter() - t0
        projected = t_part * rows.rows / len(sel)
        line = {"step": "assign", "round": args.round, "n_next": n_next, "means": n_means, "mean_nonzeros": float((means > 0).sum(axis=1).mean()), "rows": len(sel),
                "seconds": t_part, "pairs_per_s": len(sel) * n_means / t_part, "projected_whole_round_s": projected}
        print(json.dumps(line), flush=True)
        if projected <= args.budget:
            t0 = time.perf_counter()
            clusters, _ = km.predict(means)
            t_all = time.perf_counter() - t0
            print(json.dumps({"step": "assign", "round": args.round, "n_next": n_next, "means": n_means, "rows": rows.rows, "seconds": t_all,
                              "pairs_per_s": rows.rows * n_means / t_all, "clusters_in_use": int(len(np.unique(clusters)))}), flush=True)
        rows.buffer.free()


if __name__ == "__main__":
    main()
