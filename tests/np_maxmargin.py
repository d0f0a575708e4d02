"""The max-margin gadget (include/rustsolver_amd.h: rs_range_cfr_set_gadget_kind, RS_GADGET_MAXMARGIN) and the per-hand root values of the best-response walk
(rs_best_response_hands), restated in numpy on np_resolve.walk and oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definitions in the header, not from the device code: dense deal matrices, no lane rows, no job table, no LDS staging.

  * root_hands(nodes, sigma, game, cids, traverser, mode, real, ...): (value, mass) per hand of the traverser -- the root's value row of np_locks.best_response's walk
    (np_rake's leaves where a rake is given) and the root's mass row (the uncontested leaf of value 1.0 on the opponent's initial reach of ones: the deal weights sit in
    the leaf matrices), each summed over the run-outs ascending from 0.0, lanes that are no deal not added.
  * rho_of(regret0, M): regret matching over the live hands, f64.
  * maxmargin_sweep(nodes, R, S, G, game, cids, p, ...): one sweep of the game with the max-margin gadget G = dict(resolver, alt [n_O] f64, regret and ssum f32 [2][n_O])
    above the root; row 0 is the hand-choice row, row 1 is never read and never written.  G["margin"] holds the margins after the opponent's sweep.
    reverse: the SECOND summation order -- np_resolve.walk's, every fold from the last run-out to the first, every sum over hands from the last hand to the first.
"""
import numpy as np

import np_locks as nl
import np_rake as nrk
import np_resolve as nr

F32 = np.float32


def _fold(x, dealt, reverse=False):
    """[NB][n] -> [n]: the sum over the run-outs in order from 0.0, lanes that are no deal not added"""
    acc = np.zeros(x.shape[1])
    for b in (range(len(x) - 1, -1, -1) if reverse else range(len(x))):
        acc = np.where(dealt[b], acc + x[b], acc)
    return acc


def _ordered(terms, live, reverse=False):
    """the sequential f64 sum of terms over the live hands, ascending (reverse: descending) from 0.0"""
    acc = 0.0
    idx = np.flatnonzero(live)
    for h in (idx[::-1] if reverse else idx):
        acc = acc + float(terms[h])
    return acc


def root_hands(nodes, sigma, game, cids, traverser, mode="max", real=False, reverse=False, locks=None, rake=None):
    """-> (value [n_p], mass [n_p]); sigma(index) -> f32 [A][C]; mode "max" | "avg"; real: RS_BR_REAL ("max" only)"""
    p, g = traverser, game
    with nrk._raked(rake):
        w = nl._Walk(nodes, game, cids, p, locks, reverse)

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
            lk = w.lanes(i)
            if lk is not None:
                return w.locked_value(lk, vch)
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
            for a in range(1, len(vch)):                                           # the first maximum stays
                m = best_val < sums[a]
                best[m], best_val[m] = a, sums[a][m]
            chosen = best[np.where(w.dealt, k, 0)]
            return np.where(w.dealt, np.take_along_axis(vch, chosen[None, :, :], axis=0)[0], 0.0)

        ones = np.ones((w.NB, g.n[1 - p]))
        v = walk(0, ones)
        m = w.leaf(w.M_fold, ones)                                                 # the mass row is never raked: an uncontested leaf of value 1.0
    return _fold(v, w.dealt, reverse), _fold(m, w.dealt, reverse)


def new_gadget(resolver, alt):
    G = nr.new_gadget(resolver, alt)
    G["margin"] = None
    return G


def mass_of(game, O, reverse=False):
    """M [n_O]: the root's mass row on O's side folded per hand, and whether the hand has a dealt lane"""
    M_fold, _, live = nr._matrices(game, O, reverse)
    m = nr._leaf(M_fold, live, np.ones((len(game.ro), game.n[1 - O])), reverse)
    dealt = ~game.blocked[O]
    return _fold(m, dealt, reverse), dealt.any(axis=0)


def rho_of(regret0, M, dealt_any, reverse=False):
    """-> rho [n] f64, live [n] bool"""
    live = dealt_any & (M > 0)
    with np.errstate(invalid="ignore"):
        pos = np.where(live & (regret0 > 0), regret0.astype(np.float64), 0.0)
    norm = _ordered(pos, np.ones(len(pos), dtype=bool), reverse)
    L = int(live.sum())
    if norm > 0:
        with np.errstate(invalid="ignore", over="ignore"):
            rho = pos / norm
    else:
        rho = np.where(live, 1.0 / L if L else 0.0, 0.0)
    return np.where(live, rho, 0.0), live


def maxmargin_sweep(nodes, R, S, G, game, cids, p, rmplus=False, reverse=False, detail=None):
    """one sweep of traverser p (R, S and, on the opponent's sweep, row 0 of G's rows and G["margin"] updated in place); returns the value"""
    g, P = game, G["resolver"]
    O = 1 - P
    NB, alt = len(g.ro), G["alt"]
    assert len(alt) == g.n[O]
    M, dealt_any = mass_of(g, O, reverse)
    rho, live = rho_of(G["regret"][0], M, dealt_any, reverse)
    Msafe = np.where(live, M, 1.0)
    if p == P:
        with np.errstate(over="ignore", invalid="ignore"):
            scale = np.where(live, rho / Msafe, 0.0)
            root = nr.walk(nodes, R, S, g, cids, p, np.ones((NB, g.n[O])) * scale[None, :], rmplus, reverse)
            A = _ordered(rho * alt, live, reverse)
        if detail is not None:
            detail.update(root=root, A=A, rho=rho, live=live, M=M)
        return float((root.reshape(-1)[::-1] if reverse else root).sum() + A)
    vF = nr.walk(nodes, R, S, g, cids, p, np.ones((NB, g.n[P])), rmplus, reverse)
    F = _fold(vF, ~g.blocked[O], reverse)
    with np.errstate(over="ignore", invalid="ignore"):
        fm = F / Msafe
        u = fm - alt
        U = _ordered(rho * u, live, reverse)
        Rn = (G["regret"][0].astype(np.float64) + (u - U)).astype(F32)
        if rmplus:
            Rn = np.where(Rn > 0, Rn, F32(0.0)).astype(F32)
        Sn = (G["ssum"][0].astype(np.float64) + rho).astype(F32)
        margin = np.where(live, alt - fm, np.nan)
    G["regret"] = G["regret"].copy()
    G["ssum"] = G["ssum"].copy()
    G["regret"][0] = np.where(live, Rn, G["regret"][0])
    G["ssum"][0] = np.where(live, Sn, G["ssum"][0])
    G["margin"] = margin
    if detail is not None:
        detail.update(F=F, M=M, u=u, rho=rho, live=live)
    return float(U)


def maxmargin_train(nodes, R, S, G, game, cids, iterations, rmplus=False, dcfr=None):
    """iterations of (traverser 0, traverser 1) with np_range_cfr.train's ticks (dcfr = (alpha, beta, gamma), a tick per iteration), both gadget rows included"""
    import np_range_cfr as nrc
    values = [0.0, 0.0]
    for t in range(1, iterations + 1):
        for p in (0, 1):
            values[p] = maxmargin_sweep(nodes, R, S, G, game, cids, p, rmplus)
        if dcfr is not None:
            f = nrc.dcfr_factors(dcfr[0], dcfr[1], dcfr[2], t)
            nrc.discount(R, S, *f)
            nr.gadget_discount(G, *f)
    return np.array(values)
