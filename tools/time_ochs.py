#!/usr/bin/env python3
"""The timings of profiles/ochs.md on one device: the whole-round OCHS feature sweep of every street at 8 and 2 opponent clusters, and the preflop counts beside
rs_ehs_round_histograms on the flop at the same bin count, alternating in one process.  Host clock around calls that synchronise; every shape is warmed up on a listed
board first; three repeats each.  The last line is JSON.

    python tools/time_ochs.py [--bins 35] [--repeats 3]
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

WARM = {3: [[0, 1, 20]], 4: [[0, 1, 22, 35]], 5: [[0, 1, 22, 35, 49]]}


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def table_xor(feat, slice_rows=1 << 22):
    xor = np.uint32(0)
    for first in range(0, feat.rows, slice_rows):
        xor ^= np.bitwise_xor.reduce(feat.download(first, min(slice_rows, feat.rows - first)).view(np.uint32), axis=None)
    return "0x%08x" % int(xor)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bins", type=int, default=35)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if rs.device_count() < 1:
        raise SystemExit("time_ochs: no HIP device visible; the engine has no CPU fallback")
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])
    result = {"bins": args.bins}
    result["opponent_clusters_s"] = [timed(lambda: ab.opponent_clusters(table, 8, args.bins, seed=1))[0] for _ in range(2)]
    pair_cluster = ab.opponent_clusters(table, 8, args.bins, seed=1)
    result["range_sizes"] = np.bincount(pair_cluster, minlength=8).tolist()
    for nb in (3, 4, 5):
        indexer = ab.HandIndexer([2, nb])
        for n_clusters in (8, 2):
            pc = np.where(pair_cluster < n_clusters, pair_cluster, ab.OCHS_NO_CLUSTER).astype(np.uint8)
            feat = ab.ochs_features(table, indexer, pc, n_clusters, True, boards=WARM[nb])
            times = [timed(lambda: ab.ochs_features(table, indexer, pc, n_clusters, True, out=feat))[0] for _ in range(args.repeats)]
            key = "features_%d_board_cards_%d_clusters" % (nb, n_clusters)
            result[key + "_s"] = times
            if feat.nbytes <= 1 << 31:                       # the river at 8 clusters is 3.9 GB: tools/gen_ochs.py prints its checksum
                result[key + "_xor"] = table_xor(feat)
            print(key, times, flush=True)
            feat.buffer.free()
    flop = ab.HandIndexer([2, 3])
    hist = ab.round_histograms(table, flop, args.bins, boards=WARM[3])
    ab.preflop_counts(table, args.bins, boards=WARM[3])
    result["flop_histograms_s"], result["preflop_counts_s"] = [], []
    for _ in range(args.repeats):
        result["flop_histograms_s"].append(timed(lambda: ab.round_histograms(table, flop, args.bins, out=hist))[0])
        seconds, counts = timed(lambda: ab.preflop_counts(table, args.bins))
        result["preflop_counts_s"].append(seconds)
    result["preflop_nonzero_cells"] = int((counts != 0).sum())
    print(json.dumps(result))


if __name__ == "__main__":
    main()
