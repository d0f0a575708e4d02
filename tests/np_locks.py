"""Node locks (include/rustsolver_amd.h, rs_node_locks), restated in numpy from their definition on oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definition and np_br's dense deal matrices, not from the device code: no lane lists, no job table, no rank-order leaf.  The
walks are this file's own -- modelled on oracle/np_br.py (best_response), tests/np_range_cfr.py (sweep) and tests/np_node_report.py (report), which stay as they are -- and
read only W, S and blocked of the game: np_br.Game and np_weighted.WeightedGame alike.

locks = {tree node id (the position in `nodes`): f64 [A][prefixes of the node's round][hands of the acting player]}.  With L[a][b][h] = lock[a][prefix_r(b)][h] on the
lanes, in every walk, whichever player traverses and whatever the mode:
    the acting player is the opponent    child a's reach is q * L[a] (lanes that are no deal carry nothing); the node's value is the sum of its children's, action order
    the acting player is the traverser   v = sum_a L[a] * vch[a], a ascending from 0.0; 0.0 where the lane is no deal.  "max": nothing is maximised there.  sweep: the
                                         node's regret and strategy-sum rows are neither read nor written, the children's own reach is pi * L[a].  report: cfv, mass
                                         and own as usual, value by the lock.
Nodes that are not locked are walked as the three sibling restatements walk them.  reverse: the SECOND summation order the siblings offer -- the info sets' lanes from
the last to the first, every fold from the last run-out of the prefix to the first, the leaves from the last opponent hand to the first, the root's row from its end.
"""
import numpy as np

from oracle import np_br as nbr
from oracle import np_restate as npr

F32 = np.float32


class _Walk:
    """what the three walks share for traverser p: the leaf matrices, the lanes that are deals, the locks on the lanes"""

    def __init__(self, nodes, game, cids, p, locks, reverse):
        g = self.g = game
        self.nodes, self.cids, self.p, self.o, self.reverse = nodes, cids, p, 1 - p, reverse
        self.locks = locks or {}
        live = (g.W > 0).astype(np.float64)
        if p == 0:
            M_fold, M_show = g.W, g.W * g.S
        else:
            M_fold, M_show, live = g.W.transpose(0, 2, 1), -(g.W * g.S).transpose(0, 2, 1), live.transpose(0, 2, 1)
        if reverse:
            M_fold, M_show, live = (np.ascontiguousarray(x[:, :, ::-1]) for x in (M_fold, M_show, live))
        self.M_fold, self.M_show, self.live = M_fold, M_show, live
        self.dealt = ~g.blocked[p]
        self.NB = len(g.ro)

    def leaf(self, M, q):
        return nbr._leaf(M, self.live, np.ascontiguousarray(q[:, ::-1]) if self.reverse else q)

    def terminal(self, nd, q):
        pot = float(np.float32(nd["value"]))
        if nd["ttype"] == "UNCONTESTED":
            return self.leaf(self.M_fold, q) * (-pot if self.p == nd["last_to_act"] else pot)
        return self.leaf(self.M_show, q) * pot

    def lanes(self, i):
        """the lock of node i on the lanes, [A][NB][hands of the acting player], or None"""
        if i not in self.locks:
            return None
        nd = self.nodes[i]
        lock = np.asarray(self.locks[i], dtype=np.float64)
        F = self.NB // self.g.per_prefix[nd["round_idx"]]
        assert lock.shape == (len(nd["children"]), F, self.g.n[nd["player"]]), (i, lock.shape)
        return lock[:, np.arange(self.NB) // self.g.per_prefix[nd["round_idx"]], :]

    def opp_sigma(self, i, sig):
        """[A][NB][n_o]: what the opponent plays at its node i on every lane; sig = its table strategy f64 [A][C] (not looked at where the node is locked)"""
        nd, g = self.nodes[i], self.g
        so = self.lanes(i)
        if so is None:
            so = sig[:, g.infoset_of(self.cids, nd["round_idx"], self.o)]
        return np.where(g.blocked[self.o][None, :, :], 0.0, so)                  # no deal there: carries nothing

    def per_info_set(self, flat, x, C):
        w = np.where(self.dealt, x, 0.0).reshape(-1)
        if self.reverse:
            return np.bincount(flat[::-1], weights=w[::-1], minlength=C + 1)[:C]
        return np.bincount(flat, weights=w, minlength=C + 1)[:C]

    def locked_value(self, L, vch):
        v = np.zeros(self.dealt.shape)
        for a in range(len(vch)):
            v = v + L[a] * vch[a]
        return np.where(self.dealt, v, 0.0)

    def total(self, v):
        return float((v.reshape(-1)[::-1] if self.reverse else v).sum())


def best_response(nodes, sigma, game, cids, mode="max", locks=None, reverse=False, real=False):
    """np_br.best_response with locks: sigma(index) -> f32 [A][clusters of the acting player]; mode "max" | "avg" -> the two players' values per deal.
    real ("max" only): RS_BR_REAL -- at its nodes that are not locked the traverser's info sets are the (prefix, hand) pairs, whatever its cluster tables say"""
    out = np.zeros(2)
    for p in (0, 1):
        w = _Walk(nodes, game, cids, p, locks, reverse)
        g = game

        def walk(i, q):
            nd = nodes[i]
            if nd["kind"] == "terminal":
                return w.terminal(nd, q)
            if nd["kind"] != "action":
                return walk(nd["children"][0], q)
            sig = np.asarray(sigma(nd["index"]), dtype=np.float32).astype(np.float64)
            r = nd["round_idx"]
            if nd["player"] != p:
                so = w.opp_sigma(i, sig)
                total = 0.0
                for a, ch in enumerate(nd["children"]):
                    total = total + walk(ch, q * so[a])
                return total
            vch = np.stack([walk(ch, q) for ch in nd["children"]])
            L = w.lanes(i)
            if L is not None:
                return w.locked_value(L, vch)
            k = g.infoset_of(cids, r, p)
            if mode != "max":
                v = np.zeros(k.shape)
                for a in range(len(vch)):
                    v = v + sig[a][k] * vch[a]
                return np.where(w.dealt, v, 0.0)
            C = sig.shape[1]
            if real:
                pp = g.per_prefix[r]
                k, C = (np.arange(w.NB) // pp)[:, None] * g.n[p] + np.arange(g.n[p])[None, :], (w.NB // pp) * g.n[p]
            flat = np.where(w.dealt, k, C).reshape(-1)
            sums = np.stack([w.per_info_set(flat, vch[a], C) for a in range(len(vch))])
            best, best_val = np.zeros(C, dtype=np.int64), sums[0].copy()
            for a in range(1, len(vch)):                                           # cfr.rs:684-690: strict <, the first maximum stays
                m = best_val < sums[a]
                best[m], best_val[m] = a, sums[a][m]
            chosen = best[np.where(w.dealt, k, 0)]
            return np.where(w.dealt, np.take_along_axis(vch, chosen[None, :, :], axis=0)[0], 0.0)

        out[p] = w.total(walk(0, np.ones((w.NB, g.n[1 - p]))))
    return out


def sweep(nodes, R, S, game, cids, p, rmplus=False, locks=None, reverse=False):
    """np_range_cfr.sweep with locks: one sweep of traverser p over the tables R, S (updated in place; a locked node's rows stay); returns the traverser's value per deal"""
    w = _Walk(nodes, game, cids, p, locks, reverse)
    g = game

    def walk(i, q, pi):
        nd = nodes[i]
        if nd["kind"] == "terminal":
            return w.terminal(nd, q)
        if nd["kind"] != "action":
            return walk(nd["children"][0], q, pi)
        idx, r = nd["index"], nd["round_idx"]
        L = w.lanes(i)
        sig = None if L is not None else npr.get_strategy_f32(R[idx]).astype(np.float64)   # before the node's update; a locked node's rows are not read
        if nd["player"] != p:
            so = w.opp_sigma(i, sig)
            total = 0.0
            for a, ch in enumerate(nd["children"]):
                total = total + walk(ch, q * so[a], pi)
            return total
        if L is not None:
            vch = np.stack([walk(ch, q, pi * L[a]) for a, ch in enumerate(nd["children"])])
            return w.locked_value(L, vch)
        k = g.infoset_of(cids, r, p)
        sk = sig[:, k]
        vch = np.stack([walk(ch, q, pi * sk[a]) for a, ch in enumerate(nd["children"])])
        v = np.zeros(k.shape)
        for a in range(len(vch)):
            v = v + sk[a] * vch[a]
        C = sig.shape[1]
        flat = np.where(w.dealt, k, C).reshape(-1)
        sums = np.stack([w.per_info_set(flat, vch[a], C) for a in range(len(vch))])
        P = w.per_info_set(flat, pi, C)
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
        return np.where(w.dealt, v, 0.0)

    return w.total(walk(0, np.ones((w.NB, g.n[1 - p])), np.ones((w.NB, g.n[p]))))


def train(nodes, R, S, game, cids, iterations, rmplus=False, locks=None):
    """`iterations` iterations (traverser 0's sweep, then traverser 1's) on R, S in place; returns the last iteration's two values"""
    values = [0.0, 0.0]
    for _ in range(iterations):
        for p in (0, 1):
            values[p] = sweep(nodes, R, S, game, cids, p, rmplus, locks)
    return np.array(values)


def report(nodes, sigma, game, cids, p, locks=None, reverse=False):
    """np_node_report.report with locks -> {tree node id: dict(cfv=[A][F][H], value=[F][H], mass=[F][H], own=[F][H])} for every action node"""
    w = _Walk(nodes, game, cids, p, locks, reverse)
    g = game
    NB, H = w.NB, g.n[p]
    out = {}

    def fold(x, r):
        pp = g.per_prefix[r]
        x = np.where(w.dealt, x, 0.0).reshape(NB // pp, pp, H)                    # a lane that is no deal adds nothing
        acc = np.zeros((NB // pp, H))
        for k in (range(pp - 1, -1, -1) if reverse else range(pp)):
            acc = acc + x[:, k, :]
        return acc

    def first_deal(x, r):
        pp = g.per_prefix[r]
        d, x = w.dealt.reshape(NB // pp, pp, H), x.reshape(NB // pp, pp, H)
        k = (pp - 1 - np.argmax(d[:, ::-1, :], axis=1)) if reverse else np.argmax(d, axis=1)
        return np.where(d.any(axis=1), np.take_along_axis(x, k[:, None, :], axis=1)[:, 0, :], 0.0)

    def walk(i, q, pi):
        nd = nodes[i]
        if nd["kind"] == "terminal":
            return w.terminal(nd, q)
        if nd["kind"] != "action":
            return walk(nd["children"][0], q, pi)
        r = nd["round_idx"]
        sig = np.asarray(sigma(nd["index"]), dtype=np.float32).astype(np.float64)
        if nd["player"] != p:
            so = w.opp_sigma(i, sig)
            vch = [walk(ch, q * so[a], pi) for a, ch in enumerate(nd["children"])]
            v = 0.0
            for a in range(len(vch)):
                v = v + vch[a]
        else:
            sk = w.lanes(i)
            if sk is None:
                sk = sig[:, g.infoset_of(cids, r, p)]
            vch = [walk(ch, q, pi * sk[a]) for a, ch in enumerate(nd["children"])]
            v = w.locked_value(sk, vch)                                            # (the unlocked expression is the same text: sum_a sk[a] * vch[a], 0.0 where no deal)
        out[i] = dict(cfv=np.stack([fold(x, r) for x in vch]), value=fold(v, r), mass=fold(w.leaf(w.M_fold, q), r), own=first_deal(pi, r))
        return v

    walk(0, np.ones((NB, g.n[1 - p])), np.ones((NB, H)))
    return out
