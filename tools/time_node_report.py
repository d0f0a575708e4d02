#!/usr/bin/env python3
"""Times DealTrainer.node_report() beside the best-response call whose walk it shares, on the trainer tools/time_best_response.py builds (a flop, the three-street tree,
lossless abstractions), interleaved: medians and their ratio.
    HANDS=200 python tools/time_node_report.py [rounds]            # every action node, both traversers, against one RS_BR_AVERAGE | RS_BR_SORTED call (both traversers)
    NODES=first HANDS=200 python tools/time_node_report.py         # the first betting round's action nodes only (what a range view of the flop asks for)
    RS_BR_DEPTH_FIRST=1 ...                                        # one launch per tree node instead of one per tree depth and kind
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab

mask = ab.card_mask("7h8hQc")
hands = ab.random_range(mask)
if os.environ.get("HANDS"):
    hands = hands[np.random.Generator(np.random.PCG64(1)).permutation(len(hands))[: int(os.environ["HANDS"])]]
n_actions, tree = rs.build_game_tree(rs.three_street_options())
card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, None) for r in range(3)]
tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, 1 << 16, seed=1)
first_round = min(nd.round_idx for nd in tree.nodes if nd.kind == L.NODE_ACTION)
ids = [i for i, nd in enumerate(tree.nodes) if nd.kind == L.NODE_ACTION and (os.environ.get("NODES") != "first" or nd.round_idx == first_round)]
print("hands", len(hands), "action nodes reported", len(ids), "of", n_actions, "table GB %.2f" % (tr.infosets.nbytes / 1e9))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def report():
    doubles = 0
    for p in (0, 1):
        rep = tr.node_report(p, ids)
        doubles += sum(b["cfv"].size + 3 * b["value"].size for b in rep.values())
    return doubles


average = lambda: tr.best_response(L.BR_AVERAGE | L.BR_SORTED)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
for name, f in (("average", average), ("report", report)):   # warm-up: the index, the workspace (the report trades it for a larger one), the kernels' code
    out, dt = timed(f)
    print("warm-up %-8s %.3f s  launches %d  held %.2f GB  %s" % (name, dt, tr.br_launches(), tr.br_bytes() / 1e9, out), flush=True)
times = {"average": [], "report": []}
for k in range(rounds):
    for name, f in (("average", average), ("report", report)):
        times[name].append(timed(f)[1])
med = {}
for name in times:
    t = np.sort(times[name])
    med[name] = float(np.median(t))
    print("%-8s median %.4f s  min %.4f  max %.4f  over %d rounds" % (name, med[name], t[0], t[-1], rounds))
print("report / average %.2f" % (med["report"] / med["average"]))
