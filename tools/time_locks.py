#!/usr/bin/env python3
"""Times one full-width iteration (both traversers) of a turn-start game with 0, 1 and all of player 1's action nodes locked (rs_range_cfr_create_locked).

    python tools/time_locks.py [rounds]               # 7h8hQc2d, HANDS (default 200) combos a side, one info set per (board, hand), one pot-size bet per street
    rocprofv3 --kernel-trace --stats -d out -- python tools/time_locks.py 5      # the per-kernel split profiles/node_locks.md records

The locks are seeded random strategies per (prefix, hand).  The three objects take turns, round by round, in one process.  Prints the medians in milliseconds, the
launches per sweep and the bytes each object holds.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustsolver_amd as rs  # noqa: E402
from rustsolver_amd import _lib as L  # noqa: E402
from rustsolver_amd import abstraction as ab  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    n = int(os.environ.get("HANDS", "200"))
    rng = np.random.Generator(np.random.PCG64(11))
    mask = ab.card_mask("7h8hQc2d")
    board0 = [c for c in range(52) if mask >> c & 1]
    combos = ab.random_range(mask)
    hands = [combos[np.sort(rng.choice(len(combos), n, replace=False))] for _ in (0, 1)]
    clusters = [[(np.arange(pf, dtype=np.uint32)[:, None] * n + np.arange(n, dtype=np.uint32)[None, :]) for _ in (0, 1)] for pf in (1, 48)]
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=((1.0,), (1.0,)), raise_sizes=((), ())))

    def lock(node):
        x = rng.random((node.n_children, (1, 48)[node.round_idx], n)) + 0.05
        return x / x.sum(axis=0)[None]

    own = [i for i, nd in enumerate(tree.nodes) if nd.kind == L.NODE_ACTION and nd.player == 1]
    every = {i: lock(tree.nodes[i]) for i in own}
    last = [i for i in own if tree.nodes[i].round_idx == 1][0]           # a last-round node: its lock's rows are as long as a lane row
    cases = [("no lock", None), ("1 node locked", {last: every[last]}), ("%d nodes locked" % len(own), every)]
    solvers, tables = [], []
    for _, locks in cases:                                                # a table each: the sweeps write it
        tables.append(rs.create_infosets(n_actions, tree, [(n, n), (48 * n, 48 * n)], [1, 1], dtype=L.F32))
        solvers.append(rs.RangeCFR(tables[-1], tree, board0, hands[0], hands[1], clusters, locks=locks))
        solvers[-1].train(2)                                              # the workspace, the first launches
    ms, launches = [[] for _ in cases], [None] * len(cases)
    for _ in range(rounds):
        for k, solver in enumerate(solvers):
            t = time.perf_counter()
            sweeps = []
            for p in (0, 1):
                solver.iterate(p)
                sweeps.append(solver.launches())
            ms[k].append((time.perf_counter() - t) * 1e3)
            launches[k] = sweeps
    for k, (label, _) in enumerate(cases):
        print("%-18s median %.3f ms per iteration (min %.3f, max %.3f), launches per sweep %s, %d bytes held" %
              (label, float(np.median(ms[k])), min(ms[k]), max(ms[k]), launches[k], solvers[k].nbytes))
    for solver in solvers:
        solver.destroy()


if __name__ == "__main__":
    main()
