"""Full-width CFR over hand ranges, restated in numpy from its definition (include/rustsolver_amd.h, rs_range_cfr_*) on oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definition and np_br's dense deal matrices, not from the device code: no lane lists, no job table, no rank-order leaf.

One traverser sweep (traverser p, opponent o) walks the public tree over every run-out b at once.  Two f64 reach vectors go down: the opponent's q[b][h_o] (ones at
the root: the deal weights sit in the leaf matrices here) is multiplied by sigma(info set of the lane, a) at the opponent's nodes, the traverser's own pi[b][h_p] (ones
at the root) at its own.  sigma = np_restate.get_strategy_f32 of the node's regret rows as they stand when the sweep reaches the node, widened to f64.  Leaves are
np_br._leaf; an opponent node sums its children's values in action order; an own node of round r computes, with c(lane) = cids[r][p][prefix_r(b)][h]:
    v[lane]  = sum_a sigma[a][c(lane)] * vch[a][lane]         a ascending from 0.0; 0.0 where the lane is no deal
    S[a][c]  = sum of vch[a][lane] over the dealt lanes of c   np.bincount over the flattened lanes: ascending lane order from 0.0
    P[c]     = sum of pi[lane] over the same lanes
    U[c]     = sum_a sigma[a][c] * S[a][c]                     a ascending from 0.0
    regret[a][c] = f32(f64(regret[a][c]) + (S[a][c] - U[c]))   rmplus: a result that is not > 0 becomes 0
    ssum[a][c]   = f32(f64(ssum[a][c]) + P[c] * sigma[a][c])
Info sets without a dealt lane keep their cells; the opponent's rows are not touched.  The sweep returns the sum of the root's values: the traverser's value per deal
under the current profile.  An iteration is traverser 0's sweep, then traverser 1's; a Discounted CFR tick follows iteration t (counted from t0) when t % interval == 0
and t <= cap, with the factors of tick number t / interval.
"""
import numpy as np

from oracle import np_br as nbr
from oracle import np_restate as npr

F32 = np.float32


def zero_tables(nodes, sizes):
    """R, S: {action-node index: f32 [A][clusters of the acting player in the node's round]}, all zero"""
    R, S = {}, {}
    for nd in nodes:
        if nd["kind"] == "action":
            shape = (len(nd["children"]), sizes[nd["round_idx"]][nd["player"]])
            R[nd["index"]], S[nd["index"]] = np.zeros(shape, dtype=F32), np.zeros(shape, dtype=F32)
    return R, S


def sweep(nodes, R, S, game, cids, p, rmplus=False, reverse=False):
    """one sweep of traverser p over the tables R, S (updated in place); returns the traverser's value per deal.
    reverse: the SECOND summation order -- the info sets' lanes from the last to the first, the leaves from the last opponent hand to the first -- for the tests that
    measure how far two orders of the same sums can be apart."""
    g, o = game, 1 - p
    live = (g.W > 0).astype(np.float64)
    if p == 0:
        M_fold, M_show = g.W, g.W * g.S
    else:
        M_fold, M_show, live = g.W.transpose(0, 2, 1), -(g.W * g.S).transpose(0, 2, 1), live.transpose(0, 2, 1)
    if reverse:
        M_fold, M_show, live = (np.ascontiguousarray(x[:, :, ::-1]) for x in (M_fold, M_show, live))
    dealt = ~g.blocked[p]

    def leaf(M, q):
        return nbr._leaf(M, live, np.ascontiguousarray(q[:, ::-1]) if reverse else q)

    def per_info_set(flat, x, C):
        w = np.where(dealt, x, 0.0).reshape(-1)
        if reverse:
            return np.bincount(flat[::-1], weights=w[::-1], minlength=C + 1)[:C]
        return np.bincount(flat, weights=w, minlength=C + 1)[:C]

    def walk(i, q, pi):
        nd = nodes[i]
        if nd["kind"] == "terminal":
            pot = float(np.float32(nd["value"]))
            if nd["ttype"] == "UNCONTESTED":
                return leaf(M_fold, q) * (-pot if p == nd["last_to_act"] else pot)
            return leaf(M_show, q) * pot
        if nd["kind"] != "action":
            return walk(nd["children"][0], q, pi)
        idx, r = nd["index"], nd["round_idx"]
        sig = npr.get_strategy_f32(R[idx]).astype(np.float64)                     # [A][C], before the node's update
        if nd["player"] != p:
            so = sig[:, g.infoset_of(cids, r, o)]
            so = np.where(g.blocked[o][None, :, :], 0.0, so)
            total = 0.0
            for a, ch in enumerate(nd["children"]):
                total = total + walk(ch, q * so[a], pi)
            return total
        k = g.infoset_of(cids, r, p)                                               # [NB][n_p]
        sk = sig[:, k]                                                             # [A][NB][n_p]
        vch = np.stack([walk(ch, q, pi * sk[a]) for a, ch in enumerate(nd["children"])])
        v = np.zeros(k.shape)
        for a in range(len(vch)):
            v = v + sk[a] * vch[a]
        C = sig.shape[1]
        flat = np.where(dealt, k, C).reshape(-1)                                   # lanes that are no deal belong to no info set
        sums = np.stack([per_info_set(flat, vch[a], C) for a in range(len(vch))])  # [A][C]
        P = per_info_set(flat, pi, C)
        U = np.zeros(C)
        for a in range(len(vch)):
            U = U + sig[a] * sums[a]
        used = np.bincount(flat, minlength=C + 1)[:C] > 0
        Rn = (R[idx].astype(np.float64) + (sums - U[None, :])).astype(F32)
        if rmplus:
            Rn = np.where(Rn > 0, Rn, F32(0.0)).astype(F32)
        Sn = (S[idx].astype(np.float64) + P[None, :] * sig).astype(F32)
        R[idx] = np.where(used[None, :], Rn, R[idx])
        S[idx] = np.where(used[None, :], Sn, S[idx])
        return np.where(dealt, v, 0.0)

    return float(walk(0, np.ones((len(g.ro), g.n[o])), np.ones((len(g.ro), g.n[p]))).sum())


def dcfr_factors(alpha, beta, gamma, tick):
    """(pos, neg, sum) of tick number `tick` > 0: x / (x + 1) for x = tick^alpha and tick^beta, (tick / (tick + 1))^gamma; f64, each rounded once to f32"""
    def ratio(e):
        if np.isinf(e):
            return 1.0 if e > 0 else 0.0
        x = float(tick) ** e
        return 1.0 if np.isinf(x) else x / (x + 1.0)
    return F32(ratio(alpha)), F32(ratio(beta)), F32((float(tick) / (float(tick) + 1.0)) ** gamma)


def discount(R, S, pos, neg, sm):
    """a tick on f32 tables: regrets > 0 times pos, the other regrets times neg, strategy sums times sm -- one f32 multiply per cell"""
    for i in R:
        R[i] = np.where(R[i] > 0, R[i] * F32(pos), R[i] * F32(neg)).astype(F32)
        S[i] = (S[i] * F32(sm)).astype(F32)


def train(nodes, R, S, game, cids, iterations, rmplus=False, dcfr=None, t0=0, after=None):
    """`iterations` iterations on R, S in place.  dcfr: None or (alpha, beta, gamma[, interval[, cap]]).  after(t): called after iteration t (and its tick).
    Returns the last iteration's two values."""
    values = [0.0, 0.0]
    t = t0
    for _ in range(iterations):
        for p in (0, 1):
            values[p] = sweep(nodes, R, S, game, cids, p, rmplus)
        t += 1
        if dcfr is not None:
            alpha, beta, gamma = dcfr[:3]
            interval = dcfr[3] if len(dcfr) > 3 else 1
            cap = dcfr[4] if len(dcfr) > 4 else None
            if t % interval == 0 and (cap is None or t <= cap):
                discount(R, S, *dcfr_factors(alpha, beta, gamma, t // interval))
        if after is not None:
            after(t)
    return np.array(values)


def exploitability(nodes, S, game, cids):
    """chips per deal: np_br.best_response "max" against the final strategy of the sums, (v0 + v1) / 2"""
    sig = {i: nbr.final_strategy(s) for i, s in S.items()}
    return float(nbr.best_response(nodes, sig.__getitem__, None, None, cids, "max", None, game).sum() / 2.0)


def profile_value(nodes, S, game, cids):
    """the two players' values when both play the final strategy of the sums ("avg")"""
    sig = {i: nbr.final_strategy(s) for i, s in S.items()}
    return nbr.best_response(nodes, sig.__getitem__, None, None, cids, "avg", None, game)
