"""Weighted hand ranges (include/rustsolver_amd.h, rs_range_weights), restated in numpy on oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definition: the dense deal tensor W[b][h0][h1] is rebuilt from the per-hand weights W0[h0], W1[h1] for both deal
distributions; no lane rows, no split of the weight between a traverser's side and an opponent's reach.  np_br.best_response, np_range_cfr.sweep / train and
np_node_report.report take a `game` and read only W, S and blocked of it, so handed a WeightedGame they restate the weighted feature unchanged.

A deal (b, h0, h1) exists when the run-out b, h0 and h1 share no card.  With Z0(b) = the sum of W0 over player 0's hands that avoid b and Z1(b, h0) = the sum of W1 over
player 1's hands that avoid b and h0 (every sum sequential over ascending index from 0.0: np.cumsum; a hand that does not fit adds 0.0, which changes no bit of a sum of
positive terms):
    "sequential"   W = ((P(b) * W0[h0]) / (Z0(b) * Z1(b, h0))) * W1[h1]      generate_hand with weighted draws; a lane with Z1 = 0 has no deal: its share is lost
    "joint"        W = (W0[h0] / Z) * W1[h1]                                   Z = the sum over the lanes (b, h0) that are no blocked lane, ascending, of W0[h0] * Z1(b, h0)
and 0.0 where there is no deal.  None for a player's weights = 1.0 for every hand.
"""
import numpy as np

from oracle import np_br as nbr

DEALS = ("sequential", "joint")


class WeightedGame(nbr.Game):
    def __init__(self, board0, hands, weights=(None, None), deal="sequential"):
        super().__init__(board0, hands)
        assert deal in DEALS, deal
        w = [np.ones(self.n[p]) if weights[p] is None else np.asarray(weights[p], dtype=np.float64).reshape(-1) for p in (0, 1)]
        assert [len(x) for x in w] == self.n and all((x > 0).all() and np.isfinite(x).all() for x in w)
        self.weights, self.deal = w, deal
        hit = self.blocked
        share = (self.hands[0][:, None, :, None] == self.hands[1][None, :, None, :]).any(axis=(2, 3))      # [n0][n1]
        ok = ~hit[0][:, :, None] & ~hit[1][:, None, :] & ~share[None, :, :]                              # [NB][n0][n1]: a deal
        K, D = 5 - len(board0), 52 - len(board0)
        pb = 1.0 / float(np.prod([D - i for i in range(K)], dtype=np.int64)) if K else 1.0
        z0 = np.cumsum(np.where(~hit[0], w[0][None, :], 0.0), axis=1)[:, -1]                             # [NB]
        z1 = np.cumsum(np.where(ok, w[1][None, None, :], 0.0), axis=2)[:, :, -1]                         # [NB][n0]; 0.0 on a blocked lane
        self.Z0, self.Z1 = z0, z1
        if deal == "sequential":
            lane = np.where(z1 > 0, (pb * w[0][None, :]) / np.where(z1 > 0, z0[:, None] * z1, 1.0), 0.0)
        else:
            self.Z = float(np.cumsum(np.where(~hit[0], w[0][None, :] * z1, 0.0).reshape(-1))[-1])
            lane = np.where(z1 > 0, w[0][None, :] / (self.Z if self.Z > 0 else 1.0), 0.0)
        self.W = np.where(ok, lane[:, :, None] * w[1][None, None, :], 0.0)


def repeat_hands(hands, cids, p, k):
    """player p's range with hand h listed k[h] times (k integers >= 1), the columns of its cluster tables repeated with it: the range that integer weights k stand for"""
    k = np.asarray(k, dtype=np.int64)
    hands = [np.asarray(h) for h in hands]
    hands[p] = np.repeat(hands[p], k, axis=0)
    cids = [[np.repeat(np.asarray(row[q]).reshape(-1, len(k)), k, axis=1) if q == p else np.asarray(row[q]) for q in (0, 1)] for row in cids]
    return hands, cids
