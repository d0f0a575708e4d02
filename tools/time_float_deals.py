#!/usr/bin/env python3
"""Times the float-table deal path past 16 384 clusters per round.

    python tools/time_float_deals.py members       # rs_member_lists on 4 M and 64 K deals, k = 16 384 (counting sort), 16 385, 55 000 and 2^20 (radix sort); kernel times: run under
                                                   # rocprofv3 --kernel-trace --stats (k_kmeans_* = the counting sort, k_ml_* = the radix sort)
    python tools/time_float_deals.py train         # the three-street game from 7h8hQc with bucket files on flop and turn and the ISOMORPHIC river (40 / 55 combos:
                                                   # > 40 000 river clusters per player), ms per batch on f16 and i32 tables at 64 K and 1 M deals (no pruning on either)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd.solver import DeviceBuffer


def members():
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])
    rng = np.random.Generator(np.random.PCG64(3))
    for n, k in [(n, k) for n in (1 << 22, 1 << 16) for k in (16384, 16385, 55000, 1 << 20)]:
        keys = DeviceBuffer.from_numpy(table, rng.integers(0, k, size=n, dtype=np.uint64).astype(np.uint32))
        start, mem = DeviceBuffer(table, (k + 1) * 4), DeviceBuffer(table, n * 4)
        reps = int(os.environ.get("REPS", "20"))
        t0 = time.perf_counter()
        for _ in range(reps):   # each call allocates and frees its scratch and synchronises: the wall time is an upper bound, the kernel trace gives the build itself
            L.check(L.load().rs_member_lists(table._h, keys.ptr, n, k, start.ptr, mem.ptr))
        print("member lists n=%d k=%d: %.3f ms per call (wall, with the scratch allocation)" % (n, k, (time.perf_counter() - t0) / reps * 1e3), flush=True)
        for b in (keys, start, mem):
            b.free()


def train():
    rng = np.random.Generator(np.random.PCG64(79))
    mask = ab.card_mask("7h8hQc")
    allh = ab.random_range(mask)
    ranges = [allh[rng.permutation(len(allh))[:40]], allh[rng.permutation(len(allh))[:55]]]
    files = [rng.integers(0, 37, size=1286792, dtype=np.uint32), rng.integers(0, 61, size=13960050, dtype=np.uint32), None]
    n_actions, tree = rs.build_game_tree(rs.three_street_options())
    card_abs = [ab.CardAbstraction.init(ranges, mask, r, files[r]) for r in range(3)]
    print("river clusters per player: %s" % [card_abs[2].get_size(p) for p in (0, 1)], flush=True)
    sizes = [int(x) for x in os.environ.get("SIZES", "65536,1048576").split(",")]
    batches = int(os.environ.get("BATCHES", "5"))
    for n in sizes:
        for name, dtype in (("f16", rs.F16), ("i32", rs.I32)):
            tr = rs.DealTrainer(tree, card_abs, ranges, mask, n, seed=7, discount_interval=0, prune_threshold=None, dtype=dtype)
            tr.train(2)
            tr.infosets.sync()
            best = 1e9
            for _ in range(int(os.environ.get("REPS", "3"))):
                t0 = time.perf_counter()
                tr.train(batches)
                tr.infosets.sync()
                best = min(best, (time.perf_counter() - t0) / batches * 1e3)
            print("three-street ISOMORPHIC river, %s table, %d deals: best %.3f ms/batch" % (name, n, best), flush=True)
            del tr


if __name__ == "__main__":
    {"members": members, "train": train}[sys.argv[1]]()
