"""The node report (include/rustsolver_amd.h, rs_node_report), restated in numpy from its definition on oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definition and np_br's dense deal matrices, not from the device code: no lane lists, no job table, no rank-order leaf.

For traverser p (opponent o) the walk of np_br.best_response(mode="avg") runs over every run-out b at once, with the traverser's own reach pi[b][h_p] (ones at the root,
times sigma(info set of the lane, a) at the traverser's nodes) taken down beside the opponent's q[b][h_o] (ones at the root: the deal weights sit in the leaf matrices
here).  sigma(index) is the caller's: np_br.final_strategy of the strategy sums, or np_restate.get_strategy(_f32) of the regrets.  At every action node n of round r,
acted by either player, with pp = the run-outs under a prefix of round r and fold(x)[f][h] = the sum of x[b][h] over the run-outs b of prefix f on which (b, h) is a deal,
in ascending run-out order from 0.0:
    cfv[a] = fold(vch[a])        vch[a] = the value row of child a (at an opponent's node it carries the opponent's probability of a)
    value  = fold(v)             v = sum_a sigma[a][c(lane)] * vch[a], a ascending from 0.0, at an own node; the children summed in action order at an opponent's
    mass   = fold(m)             m = np_br._leaf(fold matrix, q_n): an uncontested leaf of value 1.0 on the opponent's reach at n
    own    = pi on the lowest run-out of the prefix on which (b, h) is a deal, 0.0 where there is none
reverse: the SECOND summation order -- every fold from the last run-out of the prefix to the first, every leaf from the last opponent hand to the first (and own read
on the highest dealt run-out: pi is constant over a prefix's deals) -- for the tests that measure how far two orders of the same sums can be apart.
"""
import numpy as np

from oracle import np_br as nbr
from oracle import np_restate as npr

F32 = np.float32


def strategies(tables, current=False, dtype="f32"):
    """{action-node index: f32 [A][C]} from (R, S): the final strategy of the sums, or (current) get_strategy of the regrets as stored"""
    R, S = tables
    with np.errstate(over="ignore", invalid="ignore"):
        if not current:
            return {i: nbr.final_strategy(S[i]) for i in S}
        return {i: (npr.get_strategy(R[i]) if dtype == "i32" else npr.get_strategy_f32(R[i])) for i in R}


def report(nodes, sigma, game, cids, p, reverse=False):
    """-> {tree node id: dict(cfv=[A][F][H], value=[F][H], mass=[F][H], own=[F][H])} for every action node; sigma(index) -> f32 [A][clusters of the acting player]"""
    g, o = game, 1 - p
    NB, H = len(g.ro), g.n[p]
    live = (g.W > 0).astype(np.float64)
    if p == 0:
        M_fold, M_show = g.W, g.W * g.S
    else:
        M_fold, M_show, live = g.W.transpose(0, 2, 1), -(g.W * g.S).transpose(0, 2, 1), live.transpose(0, 2, 1)
    if reverse:
        M_fold, M_show, live = (np.ascontiguousarray(x[:, :, ::-1]) for x in (M_fold, M_show, live))
    dealt = ~g.blocked[p]
    out = {}

    def leaf(M, q):
        return nbr._leaf(M, live, np.ascontiguousarray(q[:, ::-1]) if reverse else q)

    def fold(x, r):
        pp = g.per_prefix[r]
        x = np.where(dealt, x, 0.0).reshape(NB // pp, pp, H)      # a lane that is no deal adds nothing
        acc = np.zeros((NB // pp, H))
        for k in (range(pp - 1, -1, -1) if reverse else range(pp)):
            acc = acc + x[:, k, :]
        return acc

    def first_deal(x, r):
        pp = g.per_prefix[r]
        d, x = dealt.reshape(NB // pp, pp, H), x.reshape(NB // pp, pp, H)
        k = (pp - 1 - np.argmax(d[:, ::-1, :], axis=1)) if reverse else np.argmax(d, axis=1)
        return np.where(d.any(axis=1), np.take_along_axis(x, k[:, None, :], axis=1)[:, 0, :], 0.0)

    def walk(i, q, pi):
        nd = nodes[i]
        if nd["kind"] == "terminal":
            pot = float(np.float32(nd["value"]))
            if nd["ttype"] == "UNCONTESTED":
                return leaf(M_fold, q) * (-pot if p == nd["last_to_act"] else pot)
            return leaf(M_show, q) * pot
        if nd["kind"] != "action":
            return walk(nd["children"][0], q, pi)
        r = nd["round_idx"]
        sig = np.asarray(sigma(nd["index"]), dtype=np.float32).astype(np.float64)
        if nd["player"] != p:
            so = sig[:, g.infoset_of(cids, r, o)]
            so = np.where(g.blocked[o][None, :, :], 0.0, so)
            vch = [walk(ch, q * so[a], pi) for a, ch in enumerate(nd["children"])]
            v = 0.0
            for a in range(len(vch)):
                v = v + vch[a]
        else:
            sk = sig[:, g.infoset_of(cids, r, p)]
            vch = [walk(ch, q, pi * sk[a]) for a, ch in enumerate(nd["children"])]
            v = np.zeros((NB, H))
            for a in range(len(vch)):
                v = v + sk[a] * vch[a]
            v = np.where(dealt, v, 0.0)
        out[i] = dict(cfv=np.stack([fold(x, r) for x in vch]), value=fold(v, r), mass=fold(leaf(M_fold, q), r), own=first_deal(pi, r))
        return v

    walk(0, np.ones((NB, g.n[o])), np.ones((NB, H)))
    return out
