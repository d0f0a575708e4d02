#!/usr/bin/env python3
"""Times Discounted CFR on the headline shape (river tree, 9 216 boards x 1 000 clusters; i32 clamp and f32), a tick after every iteration:

    (a) rs_train without ticks                  -- the sweeps alone (a paired solver: one pair launch per iteration, 612 B per lane on the 14-node tree)
    (b) rs_train_dcfr, fused = RS_FORM_OFF      -- the same sweeps + rs_discount_dcfr between the iterations (+ 608 B per lane)
    (c) rs_train_dcfr, fused = RS_FORM_ON       -- the two discounted single-traverser launches, the tick applied where the rows are loaded (776 B per lane)

The three legs run interleaved, round after round, on one solver and one table; every leg of a round runs the same number of iterations between two stream
synchronisations; the figure is the median over the rounds, the spread is printed beside it.  One JSON line per dtype at the end.

    python tools/time_dcfr.py [--iters 20] [--rounds 7] [--boards 9216] [--clusters 1000]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)
import rustsolver_amd as rs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boards", type=int, default=9216)
ap.add_argument("--clusters", type=int, default=1000)
args = ap.parse_args()

SUM_A = 38   # actions over the 14 action nodes of the river tree
for dtype in ("i32", "f32"):
    tr = bench.make_trainer(rs, args.boards, args.clusters, "clamp", 0, 0, 1235, 1, dtype=dtype)
    table = tr.infosets
    lanes = args.boards * args.clusters
    legs = {
        "a_sweeps_only": lambda: tr.train(args.iters, discount_interval=10**12, discount_cap=10**12),
        "b_unfused": lambda: tr.train_dcfr(args.iters, fused=False),
        "c_fused": lambda: tr.train_dcfr(args.iters, fused=True),
    }
    for f in legs.values():   # warm-up: the variant's compile, first-touch of the workspace
        f()
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, f in legs.items():
            table.sync()
            t0 = time.perf_counter()
            f()                # both wrappers synchronise the stream before they return
            ms[k].append((time.perf_counter() - t0) / args.iters * 1e3)
    assert tr.dcfr_fused
    # algorithmic bytes per lane and iteration on the 14-node tree with 4-byte cells: two single-traverser sweeps 776, one pair launch 612, a discount sweep 16 per cell
    sweeps = 612 if tr.paired else 776
    per_lane = {"a_sweeps_only": sweeps, "b_unfused": sweeps + 16 * SUM_A, "c_fused": 776}
    out = {"dtype": dtype, "lanes": lanes, "iters": args.iters, "rounds": args.rounds, "paired": bool(tr.paired)}
    for k in legs:
        med = statistics.median(ms[k])
        out[k] = {"ms_per_iteration": round(med, 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4), "bytes_per_lane": per_lane[k],
                  "GBps": round(per_lane[k] * lanes / med / 1e6, 1)}
        print("%s %-14s %.3f ms/iteration (min %.3f max %.3f), %d B/lane -> %.0f GB/s" % (dtype, k, med, min(ms[k]), max(ms[k]), per_lane[k], out[k]["GBps"]), flush=True)
    print(json.dumps(out), flush=True)
    tr.destroy()
    table.destroy()
