#!/usr/bin/env python3
"""Times the device trainer (rs_deal_trainer) on a flop-start three-street tree with K-bucket files on every street: the reference's
"real" configuration (options.rs:68-77 commented vectors), sampled mccfr.  DESIGN.md section 8 quotes its output.

    python tools/time_three_street.py            # K=5000 N=1048576 by default (environment variables K, N)
    RS_JIT_ROWS=0 RS_JIT_ORDERED=0 / RS_JIT_NO_STAGE=1 python tools/time_three_street.py   # the earlier forms, for comparison (one setting per process)
    N=4194304 python tools/time_three_street.py --rake 0.1 60   # raked against unraked (rs_deal_trainer_set_rake): two trainers in this process, ROUNDS (default 7) rounds of
                                                                # BATCHES batches each, interleaved; medians and spread as one JSON line (profiles/rake_deals.md)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rustsolver_amd as rs
# PRUNE=none: never prune; PRUNE=<t>: train()'s schedule with PRUNE_THRESHOLD = t (cfr.rs:190; default 10 000 000): batches beyond it run the `_prune` kernel forms
PRUNE = None if os.environ.get("PRUNE", "10000000") == "none" else int(os.environ.get("PRUNE", "10000000"))
from rustsolver_amd import abstraction as ab
ap = argparse.ArgumentParser()
ap.add_argument("--rake", nargs=2, type=float, metavar=("RATE", "CAP"), default=None)
args = ap.parse_args()
rng = np.random.Generator(np.random.PCG64(1))
mask = ab.card_mask("7h8hQc")
hands = ab.random_range(mask)
K = int(os.environ.get("K", "5000"))
files = [rng.integers(0, K, size=1286792, dtype=np.uint32), rng.integers(0, K, size=13960050, dtype=np.uint32), rng.integers(0, K, size=123156254, dtype=np.uint32)]
t0 = time.perf_counter()
n_actions, tree = rs.build_game_tree(rs.three_street_options())
card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, files[r]) for r in range(3)]
print("abstractions: %.1f s, sizes" % (time.perf_counter() - t0), [a.get_size(0) for a in card_abs], "action nodes", n_actions)
n = int(os.environ.get("N", str(1 << 20)))



def rake_ab():
    """the same game, seed and forms, unraked and raked, in one process: the rounds alternate, so that whatever else the machine does falls on both"""
    kw = dict(seed=7, discount_interval=0, prune_threshold=PRUNE)
    trainers = {"unraked": rs.DealTrainer(tree, card_abs, [hands, hands], mask, n, **kw), "raked": rs.DealTrainer(tree, card_abs, [hands, hands], mask, n, rake=tuple(args.rake), **kw)}
    KB, rounds = int(os.environ.get("BATCHES", "5")), int(os.environ.get("ROUNDS", "7"))
    for tr in trainers.values():
        tr.train(2)
        tr.status()
    ms = {k: [] for k in trainers}
    for r in range(rounds):
        for k in (("unraked", "raked") if r % 2 == 0 else ("raked", "unraked")):
            tr = trainers[k]
            tr.infosets.sync()
            t0 = time.perf_counter()
            tr.train(KB)
            tr.infosets.sync()
            ms[k].append((time.perf_counter() - t0) / KB * 1e3)
    for tr in trainers.values():
        tr.status()
    out = dict(figure="three-street batch, raked against unraked", clusters=K, deals=n, rake=list(args.rake), batches_per_round=KB, rounds=rounds)
    for k, v in ms.items():
        out[k] = dict(ms_median=round(float(np.median(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), rounds=[round(x, 4) for x in v])
    out["raked_over_unraked_median"] = round(float(np.median(ms["raked"]) / np.median(ms["unraked"])), 5)
    print(json.dumps(out), flush=True)


if args.rake is not None:
    rake_ab()
    sys.exit(0)
t0 = time.perf_counter()
tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, n, seed=7, discount_interval=0, prune_threshold=PRUNE, use_graph=bool(int(os.environ.get("GRAPH", "0"))), prefetch=(None if os.environ.get("PREFETCH") is None else bool(int(os.environ["PREFETCH"]))),
                    forms={"shadow": rs.SHADOW_ALL} if os.environ.get("SHADOW_ALL") else ({"kept_records": rs.FORM_OFF} if os.environ.get("NO_KEPT") else None))
# SHADOW_ALL=1: rs_kernel_forms.shadow = RS_SHADOW_ALL instead of the rule; NO_KEPT=1: rs_kernel_forms.kept_records = RS_FORM_OFF
print("trainer create: %.1f s, table %.1f MB" % (time.perf_counter() - t0, tr.infosets.nbytes / 1e6 if not callable(tr.infosets.nbytes) else tr.infosets.nbytes() / 1e6))
tr.train(2); tr.status()
KB = int(os.environ.get("BATCHES", "5"))
t0 = time.perf_counter(); tr.train(KB); tr.infosets.sync(); dt = (time.perf_counter() - t0) / KB
print("walks of the last batch per round (deal, round subtree): traverser 0", tr.walk_counts(0), "traverser 1", tr.walk_counts(1))
print("three-street, %d clusters, %d deals per batch: %.2f ms per batch = %.3g deal-iterations/s" % (K, n, dt * 1e3, n / dt))
