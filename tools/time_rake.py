#!/usr/bin/env python3
"""Times the raked walks (rs_rake) beside the unraked ones on the same build.

    python tools/time_rake.py turn [rounds]     # 7h8hQc2d, HANDS (default 200) combos a side, one info set per (board, hand), one pot-size bet per street: one full-width
                                                # iteration (both traversers) of an unraked and a raked object taking turns round by round (tools/time_resolve.py's game)
    python tools/time_rake.py flop [rounds]     # 7h8hQc, the full 1 176-combo ranges (HANDS=n for fewer), the three-street tree, CLUSTERS (default 4096) random info sets per
                                                # round and player: best_response_rounds in RS_BR_MAX | RS_BR_SORTED, unraked and raked calls taking turns (each call prepares
                                                # the game and allocates its workspace, as a one-shot call does), then full-width iterations of an unraked and of a raked object
    rocprofv3 --kernel-trace --stats -d out -- python tools/time_rake.py flop 1      # the per-launch times of the raked and unraked leaf kernels profiles/rake.md records

Rake: 5 % capped at 30.  Prints medians on the host clock, the launches per sweep and the bytes held.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustsolver_amd as rs  # noqa: E402
from rustsolver_amd import _lib as L  # noqa: E402
from rustsolver_amd import abstraction as ab  # noqa: E402

RAKE = (0.05, 30.0)
CASES = [("unraked", None), ("raked", RAKE)]


def line(label, ms, extra=""):
    print("%-26s median %.3f ms (min %.3f, max %.3f) over %d%s" % (label, float(np.median(ms)), min(ms), max(ms), len(ms), extra), flush=True)


def iterations(solvers, rounds, what):
    ms, launches = [[] for _ in solvers], [None] * len(solvers)
    for _ in range(rounds):
        for k, solver in enumerate(solvers):
            t = time.perf_counter()
            sweeps = []
            for p in (0, 1):
                solver.iterate(p)
                sweeps.append(solver.launches())
            ms[k].append((time.perf_counter() - t) * 1e3)
            launches[k] = sweeps
    for k, (label, _) in enumerate(CASES):
        line("%s %s" % (label, what), ms[k], ", launches per sweep %s, %d bytes held" % (launches[k], solvers[k].nbytes))


def turn(rounds):
    n = int(os.environ.get("HANDS", "200"))
    rng = np.random.Generator(np.random.PCG64(11))
    mask = ab.card_mask("7h8hQc2d")
    board0 = [c for c in range(52) if mask >> c & 1]
    combos = ab.random_range(mask)
    hands = [combos[np.sort(rng.choice(len(combos), n, replace=False))] for _ in (0, 1)]
    clusters = [[(np.arange(pf, dtype=np.uint32)[:, None] * n + np.arange(n, dtype=np.uint32)[None, :]) for _ in (0, 1)] for pf in (1, 48)]
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=((1.0,), (1.0,)), raise_sizes=((), ())))
    solvers, tables = [], []
    for _, rake in CASES:                                                 # a table each: the sweeps write it
        tables.append(rs.create_infosets(n_actions, tree, [(n, n), (48 * n, 48 * n)], [1, 1], dtype=L.F32))
        solvers.append(rs.RangeCFR(tables[-1], tree, board0, hands[0], hands[1], clusters, rake=rake))
        solvers[-1].train(2)                                              # the workspace, the first launches
    iterations(solvers, rounds, "iteration")
    for solver in solvers:
        solver.destroy()


def flop(rounds):
    rng = np.random.Generator(np.random.PCG64(11))
    mask = ab.card_mask("7h8hQc")
    board0 = [c for c in range(52) if mask >> c & 1]
    hands = ab.random_range(mask)
    if os.environ.get("HANDS"):
        hands = hands[np.sort(rng.permutation(len(hands))[: int(os.environ["HANDS"])])]
    n, nc = len(hands), int(os.environ.get("CLUSTERS", "4096"))
    clusters = [[rng.integers(0, nc, size=(pf, n)).astype(np.uint32) for _ in (0, 1)] for pf in (1, 49, 49 * 48)]
    n_actions, tree = rs.build_game_tree(rs.three_street_options())
    table = rs.create_infosets(n_actions, tree, [(nc, nc)] * 3, [1] * 3, dtype=L.F32)
    for nd in tree.action_nodes():
        table.upload_node(nd.index, rng.standard_normal((nd.n_children, nc)).astype(np.float32), rng.random((nd.n_children, nc)).astype(np.float32))
    print("flop: %d combos a side, %d info sets per round and player, %d tree nodes" % (n, nc, tree.n_nodes), flush=True)
    ms, values = [[] for _ in CASES], [None] * len(CASES)
    for r in range(rounds + 1):                                           # round 0: the kernels' code
        for k, (_, rake) in enumerate(CASES):
            t = time.perf_counter()
            values[k] = table.best_response_rounds(tree, board0, hands, hands, clusters, L.BR_MAX | L.BR_SORTED, rake=rake)
            if r:
                ms[k].append((time.perf_counter() - t) * 1e3)
    for k, (label, _) in enumerate(CASES):
        line("%s best response" % label, ms[k], ", values %s" % values[k])
    for k, (label, rake) in enumerate(CASES):                             # one object at a time: each holds a level plan of its own
        solver = rs.RangeCFR(table, tree, board0, hands, hands, clusters, rake=rake)
        solver.train(1)
        it = []
        for _ in range(max(rounds, 3)):
            t = time.perf_counter()
            solver.iterate(0)
            solver.iterate(1)
            it.append((time.perf_counter() - t) * 1e3)
        line("%s iteration" % label, it, ", launches %d, %.2f GB held" % (solver.launches(), solver.nbytes / 1e9))
        solver.destroy()


def main():
    game = sys.argv[1] if len(sys.argv) > 1 else "turn"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else (10 if game == "turn" else 3)
    if game == "turn":
        turn(rounds)
    elif game == "flop":
        flop(rounds)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
