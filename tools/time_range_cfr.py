#!/usr/bin/env python3
"""Times one iteration (both traversers) of full-width CFR over hand ranges (DealTrainer.train_full_width, rs_deal_trainer_range_cfr) beside the call it grew out of:
rs_best_response_rounds in RS_BR_AVERAGE | RS_BR_SORTED on the same trainer, interleaved in one process.  That call walks the same leaves with the same reach kernels; the
ratio iteration : call is what the sweep adds (the traverser's own reach downwards, the info sets' sums and the row writes at its own nodes).

    python tools/time_range_cfr.py river [rounds]      # the river game of examples/solver_main.c, full 1 081-combo ranges, ISOMORPHIC river abstraction
    python tools/time_range_cfr.py turn [rounds]       # a turn start (7h8hQc2d), 200 combos a side, lossless abstractions, one pot-size bet per street
    python tools/time_range_cfr.py flop [rounds]       # the flop start tools/time_best_response.py times: 7h8hQc, full 1 176-combo ranges, the three-street tree
    HANDS=200 python tools/time_range_cfr.py flop      # ... with 200 combos a side
    RS_BR_DEPTH_FIRST=1 ...                            # one launch per tree node instead of the level plan
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab


def make(game):
    if game == "river":
        mask, tree_options, first, hands_n = ab.card_mask("4d5dAs3cKs"), rs.default_flop(), 2, None
    elif game == "turn":
        mask, tree_options, first, hands_n = ab.card_mask("7h8hQc2d"), rs.Options(n_board_cards=4, bet_sizes=((1.0,), (1.0,)), raise_sizes=((), ())), 1, 200
    elif game == "flop":
        mask, tree_options, first, hands_n = ab.card_mask("7h8hQc"), rs.three_street_options(), 0, None
    else:
        raise SystemExit(__doc__)
    hands = ab.random_range(mask)
    hands_n = int(os.environ["HANDS"]) if os.environ.get("HANDS") else hands_n
    if hands_n:
        hands = hands[np.random.Generator(np.random.PCG64(1)).permutation(len(hands))[:hands_n]]
    n_actions, tree = rs.build_game_tree(tree_options)
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, None) for r in range(first, 3)]
    tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, 1 << 12, seed=1, discount_interval=0, prune_threshold=None, scale=0.5, dtype=rs.F32)
    print("%s: %d combos a side, clusters %s, table %.3f GB" % (game, len(hands), [a.get_size(0) for a in card_abs], tr.infosets.nbytes / 1e9), flush=True)
    return tr


def main():
    game = sys.argv[1] if len(sys.argv) > 1 else "river"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    tr = make(game)
    mode = L.BR_AVERAGE | L.BR_SORTED

    def average():
        t0 = time.perf_counter()
        v = tr.best_response(mode)
        return time.perf_counter() - t0, v

    def iteration():
        t0 = time.perf_counter()
        v = tr.train_full_width(1)
        return time.perf_counter() - t0, v

    for name, fn in (("average-value call", average), ("full-width iteration", iteration)):   # warm-up: the prepared game, the workspace, the kernels' code
        dt, v = fn()
        print("warm-up %-22s %.3f s  values %s" % (name, dt, v), flush=True)
    print("best response holds %.2f GB (launches %d)" % (tr.br_bytes() / 1e9, tr.br_launches()), flush=True)
    times = {"avg": [], "cfr": []}
    for _ in range(rounds):
        times["avg"].append(average()[0])
        times["cfr"].append(iteration()[0])
    for key, name in (("avg", "average-value call"), ("cfr", "full-width iteration")):
        t = np.sort(times[key])
        print("%-22s median %.4f s  min %.4f  max %.4f  over %d rounds" % (name, np.median(t), t[0], t[-1], rounds))
    print("ratio iteration : call = %.2f (medians)" % (np.median(times["cfr"]) / np.median(times["avg"])))
    print("exploitability of the average strategy %.5f, of the current one %.5f" % (tr.exploitability(), tr.exploitability(current=True)))
    tr.destroy()


if __name__ == "__main__":
    main()
