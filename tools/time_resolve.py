#!/usr/bin/env python3
"""Times one full-width iteration (both traversers) of a turn-start game without a gadget above the root and with one of either kind (rs_range_cfr_set_gadget,
rs_range_cfr_set_gadget_kind), and rs_best_response_hands against rs_best_response_raked on the same game.

    python tools/time_resolve.py [rounds] [--kind resolve|maxmargin|both]      # 7h8hQc2d, HANDS (default 200) combos a side, one info set per (board, hand), one pot-size bet per street
    rocprofv3 --kernel-trace --stats -d out -- python tools/time_resolve.py 5      # the per-kernel split profiles/resolve.md and profiles/maxmargin.md record

Prints the medians in milliseconds, the launches per sweep and the bytes the object holds; --kind both (the default) measures the two kinds in the same run.
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
    args = sys.argv[1:]
    kind = "both"
    if "--kind" in args:
        at = args.index("--kind")
        kind = args[at + 1]
        del args[at:at + 2]
    if kind not in ("resolve", "maxmargin", "both"):
        sys.exit("--kind is resolve, maxmargin or both")
    rounds = int(args[0]) if args else 10
    n = int(os.environ.get("HANDS", "200"))
    rng = np.random.Generator(np.random.PCG64(11))
    mask = ab.card_mask("7h8hQc2d")
    board0 = [c for c in range(52) if mask >> c & 1]
    combos = ab.random_range(mask)
    hands = [combos[np.sort(rng.choice(len(combos), n, replace=False))] for _ in (0, 1)]
    clusters = [[(np.arange(pf, dtype=np.uint32)[:, None] * n + np.arange(n, dtype=np.uint32)[None, :]) for _ in (0, 1)] for pf in (1, 48)]
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=((1.0,), (1.0,)), raise_sizes=((), ())))
    table = rs.create_infosets(n_actions, tree, [(n, n), (48 * n, 48 * n)], [1, 1], dtype=L.F32)
    solver = rs.RangeCFR(table, tree, board0, hands[0], hands[1], clusters)

    def measure(label):
        solver.train(2)                                   # the workspace, the first launches
        ms, launches = [], []
        for _ in range(rounds):
            t = time.perf_counter()
            for p in (0, 1):
                solver.iterate(p)
                launches.append(solver.launches())
            ms.append((time.perf_counter() - t) * 1e3)
        print("%-24s median %.3f ms per iteration (min %.3f), launches per sweep %s, %d bytes held" % (label, float(np.median(ms)), min(ms), launches[-2:], solver.nbytes))

    measure("without gadget")
    alt = rng.standard_normal(n) * 10.0
    for k in ("resolve", "maxmargin"):
        if kind in (k, "both"):
            solver.set_gadget(0, alt, kind=k)
            measure("with gadget, kind %s" % k)
    solver.destroy()

    def timed(label, call):
        call()                                            # the index kernels' first launches
        ms = []
        for _ in range(rounds):
            t = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t) * 1e3)
        print("%-44s median %.3f ms per call (min %.3f)" % (label, float(np.median(ms)), min(ms)))

    mode = L.BR_MAX | L.BR_REAL | L.BR_SORTED             # each call prepares the game, walks, and frees it: rs_best_response_raked both traversers, _hands one
    timed("rs_best_response_raked (two traversers)", lambda: table.best_response_rounds(tree, board0, hands[0], hands[1], clusters, mode))
    timed("rs_best_response_hands (traverser 1)", lambda: table.best_response_hands(tree, board0, hands[0], hands[1], clusters, 1, mode=mode))


if __name__ == "__main__":
    main()
