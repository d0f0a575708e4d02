#!/usr/bin/env python3
"""Times weighted dealing (rs_deals_sample_weighted, rs_deal_trainer_set_weights) on one GPU: 4 M deals from the flop 7h8hQc with both full ranges (1 176 hands).
profiles/weighted_deals.md and DESIGN.md section 5h quote its output.  One JSON line per figure.

    python tools/time_weighted_deals.py kernels                      # the unweighted kernel, then the weighted one: unit weights, random 2^-10 .. 1, 99.9 % on one hand
    python tools/time_weighted_deals.py trainer [--weights unit]     # the three-street trainer's batch time (tools/time_three_street.py's game, K = 5 000), without / with unit weights
    python tools/time_weighted_deals.py trainer --root DIR           # ... with the package of another checkout (the parent commit: it has no weights, leave --weights out)

Environment: N (deals, default 4194304), REPS (kernel launches per figure, default 20), BATCHES (timed trainer batches, default 10), K (clusters per street, default 5000)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["kernels", "trainer"])
ap.add_argument("--weights", choices=["none", "unit"], default="none")
ap.add_argument("--deal", choices=["sequential", "joint"], default="sequential")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd.solver import DeviceBuffer, deal_pitch

N = int(os.environ.get("N", str(1 << 22)))
mask = ab.card_mask("7h8hQc")
hands = ab.random_range(mask)


def emit(**kw):
    print(json.dumps(dict(kw, tag=args.tag, deals=N)), flush=True)


def kernels():
    reps = int(os.environ.get("REPS", "20"))
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])
    d = DeviceBuffer.from_numpy(table, np.ascontiguousarray(hands, dtype=np.uint8))
    pitch = deal_pitch(N)
    dc, de = DeviceBuffer(table, 9 * pitch), DeviceBuffer(table, 4)
    de.zero()
    lib, n = L.load(), len(hands)

    def timed(name, dw):
        ms = []
        for r in range(reps + 2):
            table.sync()
            t0 = time.perf_counter()
            L.check(lib.rs_deals_sample_weighted(table._h, 7, r * N, mask, d.ptr, n, d.ptr, n, None if dw is None else dw._h, N, dc.ptr, de.ptr))
            table.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[2:])
        emit(figure="kernel", case=name, ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), error_word=int(de.download(np.uint32, 1)[0]))
        de.zero()

    rng = np.random.Generator(np.random.PCG64(3))
    random_w = [2.0 ** -rng.uniform(0, 10, n) for _ in (0, 1)]
    peaked = [np.full(n, 0.001 / (n - 1)) for _ in (0, 1)]
    peaked[0][100], peaked[1][900] = 0.999, 0.999
    assert not set(hands[100].tolist()) & set(hands[900].tolist())
    same = [peaked[0], peaked[0]]          # both players want the same hand: player 1 is dealt by the exact fallback nearly every time
    timed("unweighted (k_deal_sample)", None)
    for deal in ("sequential", "joint"):
        for name, w in (("unit weights", (None, None)), ("random 2^-10..1", random_w), ("99.9 % on one hand each", peaked)):
            dw = ab.DealWeights(table, w, (n, n), deal)
            timed("%s, %s" % (deal, name), dw)
            table.sync()
            dw.destroy()
    dw = ab.DealWeights(table, same, (n, n), "sequential")
    timed("sequential, 99.9 % on the SAME hand (fallback)", dw)
    table.sync()
    dw.destroy()
    timed("unweighted (k_deal_sample), again", None)


def trainer():
    K = int(os.environ.get("K", "5000"))
    rng = np.random.Generator(np.random.PCG64(1))
    files = [rng.integers(0, K, size=1286792, dtype=np.uint32), rng.integers(0, K, size=13960050, dtype=np.uint32), rng.integers(0, K, size=123156254, dtype=np.uint32)]
    n_actions, tree = rs.build_game_tree(rs.three_street_options())
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, files[r]) for r in range(3)]
    kw = {} if args.weights == "none" else dict(weights=(np.ones(len(hands)), np.ones(len(hands))), deal=args.deal)
    tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, N, seed=7, discount_interval=0, **kw)
    tr.train(2)
    tr.status()
    KB = int(os.environ.get("BATCHES", "10"))
    passes = []
    for _ in range(3):
        tr.infosets.sync()
        t0 = time.perf_counter()
        tr.train(KB)
        tr.infosets.sync()
        passes.append((time.perf_counter() - t0) / KB * 1e3)
    tr.status()
    emit(figure="trainer", weights=args.weights, deal=args.deal if args.weights != "none" else None, ms_per_batch=round(sorted(passes)[1], 4), passes=[round(p, 4) for p in passes],
         deal_iterations_per_s=round(N / (sorted(passes)[1] * 1e-3)))


kernels() if args.part == "kernels" else trainer()
