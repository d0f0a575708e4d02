"""Rake (rs_rake): a percentage of the pot with a cap, taken from the winner at the tree's terminal nodes.

rake = (rate, cap) on InfosetTable.best_response_rounds, InfosetTable.node_report and RangeCFR.  With pot = float32(node.value) and r = min(cap, rate * pot), a winner is
paid pot - r, a loser -pot, a tie -r / 2; the folder of an uncontested terminal -pot, the other player pot - r.  UNITS: a leaf pays +-pot, the whole number in node.value,
not the opponent's half of it -- where both players have put in equal amounts a room's "5 % of the pot, capped at C" is rake = (0.10, 2 * C).  Nothing is converted.

The raked game is general-sum: the two players' values no longer add up to zero, and the exploitability of a profile takes the average-strategy values as well as the
best-response ones.  Pure numpy here apart from `arg`, which packs the C struct, and `payoffs`, which asks the library.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def arg(rake):
    """rake = None | (rate, cap) | (rate, cap, (reserved0, reserved1)) -> (a pointer to rs_rake or None, what must stay alive for the call); the library checks the values"""
    if rake is None:
        return None, None
    st = L.Rake()
    st.rate, st.cap = float(rake[0]), float(rake[1])
    if len(rake) > 2:
        st.reserved[0], st.reserved[1] = int(rake[2][0]), int(rake[2][1])
    return C.byref(st), st


def payoffs(tree, node, rake, player):
    """(win, tie, lose) of `player` at the terminal `node` (a tree node id) under rake (rs_rake_payoffs); an uncontested terminal: its one payoff three times"""
    out = np.full(3, np.nan, dtype=np.float64)
    rk, _alive = arg(rake)
    L.check(L.load().rs_rake_payoffs(tree._h, int(node), rk, int(player), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def paid(avg_values):
    """the expected rake per deal: -(v0 + v1) of the two players' values under the profile itself (BR_AVERAGE)"""
    return -(float(avg_values[0]) + float(avg_values[1]))


def exploitability(max_values, avg_values):
    """of a profile in the raked (general-sum) game: the mean of what each player gains by switching to its best response, ((max0 - avg0) + (max1 - avg1)) / 2 -- the
    BR_MAX and the BR_AVERAGE result of best_response_rounds under the same rake.  Without rake avg0 + avg1 = 0 and this is (max0 + max1) / 2"""
    return ((float(max_values[0]) - float(avg_values[0])) + (float(max_values[1]) - float(avg_values[1]))) / 2.0
