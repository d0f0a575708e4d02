#!/usr/bin/env python3
"""Times DealTrainer.exploitability() (rs_best_response_rounds with rank-order showdowns) from a flop on the three-street tree with lossless abstractions.
    python tools/time_best_response.py                 # the full 1 176-combo ranges: 2.8 M (run-out, hand) lanes
    HANDS=200 python tools/time_best_response.py       # 200 combos per range
    RS_BR_DEPTH_FIRST=1 ...                            # one launch per tree node instead of one per tree depth and kind
    python tools/time_best_response.py --real [rounds] # the abstract call and the real-game call (RS_BR_REAL) on the same trainer, interleaved: median and spread
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rustsolver_amd as rs
from rustsolver_amd import abstraction as ab

mask = ab.card_mask("7h8hQc")
hands = ab.random_range(mask)
if os.environ.get("HANDS"):
    hands = hands[np.random.Generator(np.random.PCG64(1)).permutation(len(hands))[: int(os.environ["HANDS"])]]
n_actions, tree = rs.build_game_tree(rs.three_street_options())
card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, None) for r in range(3)]
tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, 1 << 16, seed=1)
print("hands", len(hands), "clusters", [a.get_size(0) for a in card_abs], "table GB %.2f" % (tr.infosets.nbytes / 1e9))

def timed(real):
    t0 = time.perf_counter()
    e = tr.exploitability(real=real)
    return e, time.perf_counter() - t0


if "--real" in sys.argv[1:]:
    rest = [a for a in sys.argv[1:] if a != "--real"]
    rounds = int(rest[0]) if rest else 9
    for real in (False, True):   # warm-up: the index, the workspace, the kernels' code
        e, dt = timed(real)
        print("warm-up %-8s exploitability %.6f  %.3f s  launches %d  held %.2f GB" % ("real" if real else "abstract", e, dt, tr.br_launches(), tr.br_bytes() / 1e9), flush=True)
    times = {False: [], True: []}
    for k in range(rounds):
        for real in (False, True):
            times[real].append(timed(real)[1])
    for real in (False, True):
        t = np.sort(times[real])
        print("%-8s median %.4f s  min %.4f  max %.4f  over %d rounds" % ("real" if real else "abstract", np.median(t), t[0], t[-1], rounds))
else:
    for k in range(4):
        e, dt = timed(False)
        print("exploitability %.6f  %.4f s  launches %d  held %.2f GB" % (e, dt, tr.br_launches(), tr.br_bytes() / 1e9))
