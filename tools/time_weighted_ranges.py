#!/usr/bin/env python3
"""Times rs_best_response_rounds, prepare included, and the prepare step alone with and without range weights, from a flop with the full 1 176-combo ranges
(2.8 M (run-out, hand) lanes a side) on a three-street tree with one bet size per street and 200 random info sets per player and round.
    python tools/time_weighted_ranges.py [calls]                # per call: the unweighted best response, then the prepare step (rs_range_cfr_create*) without weights,
                                                                # with sequential and with joint weights, interleaved in one process; medians and spreads
    python tools/time_weighted_ranges.py --unweighted [calls]   # the unweighted best response alone: uses nothing a checkout without weighted ranges lacks, so two
                                                                # checkouts can be timed in turn (A/B between commits: alternate the two processes, compare the medians
                                                                # with the spread between rounds of one of them)
Prints one JSON line at the end."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab

args = [a for a in sys.argv[1:] if not a.startswith("--")]
calls = int(args[0]) if args else 5
only_unweighted = "--unweighted" in sys.argv[1:]

rng = np.random.Generator(np.random.PCG64(1))
mask = ab.card_mask("7h8hQc")
board0 = [c for c in range(52) if mask >> c & 1]
hands = ab.random_range(mask)
n = len(hands)
sizes = [(200, 200)] * 3
cids = [[rng.integers(0, 200, size=(pf, n)).astype(np.uint32) for _ in (0, 1)] for pf in (1, 49, 49 * 48)]
n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=3, bet_sizes=((0.5,), (0.5,), (1.0,)), raise_sizes=((), (), ())))
table = rs.create_infosets(n_actions, tree, sizes, [1, 1, 1], dtype=L.F32)
for nd in tree.action_nodes():
    shape = (nd.n_children, 200)
    table.upload_node(nd.index, rng.standard_normal(shape).astype(np.float32), (rng.random(shape) * 10.0).astype(np.float32))
weights = [rng.integers(1, 9, n) / 4.0 for _ in (0, 1)]
print("hands", n, "lanes", 49 * 48 * n, "action nodes", n_actions, flush=True)


def best_response():
    t0 = time.perf_counter()
    out = table.best_response_rounds(tree, board0, hands, hands, cids, L.BR_MAX | L.BR_SORTED)
    return time.perf_counter() - t0, out


def prepare(**kw):
    t0 = time.perf_counter()
    s = rs.RangeCFR(table, tree, board0, hands, hands, cids, **kw)
    dt = time.perf_counter() - t0
    s.destroy()
    return dt


what = {"best_response": lambda: best_response()[0]}
if not only_unweighted:
    what["prepare"] = prepare
    what["prepare_sequential"] = lambda: prepare(weights=weights)
    what["prepare_joint"] = lambda: prepare(weights=weights, deal="joint")
for name, f in what.items():                     # warm-up: the kernels' code, the allocator
    print("warm-up %-20s %.4f s" % (name, f()), flush=True)
times = {name: [] for name in what}
for k in range(calls):
    for name, f in what.items():
        times[name].append(f())
res = {}
for name, t in times.items():
    t = np.sort(t)
    res[name] = dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]), calls=calls)
    print("%-20s median %.4f s  min %.4f  max %.4f  over %d calls" % (name, np.median(t), t[0], t[-1], calls), flush=True)
print(json.dumps(res))
