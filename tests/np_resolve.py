"""Safe subgame re-solving (include/rustsolver_amd.h: rs_tree_subtree, rs_range_cfr_set_gadget; rustsolver_amd/resolve.py), restated in numpy on oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definitions and np_br's dense deal matrices, not from the device code: no lane rows, no job table, no split of a deal's
weight between a traverser's side and an opponent's reach.  Trees are np_restate.build_tree's lists of dicts, tables {action-node index: f32 [A][C]}.

  * cut(nodes, node): the subtree below an action node -- nodes in the trunk's relative order with the root at 0 (parent -1), `index` renumbered 0..n_act in ascending
    order of the trunk's index, `round_idx` less the root's, everything else as it was -- and node_map[i] = the trunk id of the subtree's node i.
  * walk(...): np_range_cfr.sweep's walk with the opponent's root reach q0 handed in and the root ROW handed back.
  * gadget_sweep(...): one sweep of a game with the re-solving gadget above the root.  P = resolver, O = 1 - P; G = dict(resolver, alt [n_O] f64, regret and ssum f32
    [2][n_O]); row 0 is TERMINATE, row 1 FOLLOW; sigma = get_strategy_f32 of G["regret"] as it stands, as f64.
      traverser O:  vF = walk(q0 = ones); m = the uncontested leaf of value 1.0 on q = ones (the resolver's initial reach: the deal weights sit in the leaf matrices);
                    vT = alt[h] * m.  Per hand h with a dealt lane, over its dealt lanes in ascending run-out order from 0.0: S[0] = sum vT, S[1] = sum vF,
                    Pi = the count of dealt lanes, U = sigma[0] * S[0] + sigma[1] * S[1] (from 0.0), regret[a][h] = f32(regret[a][h] + (S[a] - U)) (rmplus: not > 0
                    becomes 0), ssum[a][h] = f32(ssum[a][h] + Pi * sigma[a]); v = sigma[0] * vT + sigma[1] * vF (from 0.0; 0.0 where no deal); value = v.sum().
      traverser P:  walk(q0 = ones * sigma[1][h]); value = the root row's sum + the sum of the TERMINATE leaf's row, the uncontested leaf of value -1.0 on
                    q = (ones * sigma[0][h]) * alt[h].  G's rows stay.
    reverse: the SECOND summation order (np_range_cfr.sweep's, and the gadget's folds from the last run-out to the first).
  * prepare / graft: the re-solve recipe of DESIGN.md 5e on these trees and tables (np_node_report.report for the node report).
"""
import numpy as np

import np_node_report as nnr
from oracle import np_br as nbr
from oracle import np_restate as npr

F32 = np.float32


# ---- the subtree cut ---------------------------------------------------------------------------------------------------------------------------------------------
def cut(nodes, node):
    if not (0 <= node < len(nodes)) or nodes[node]["kind"] != "action":
        raise ValueError("the root of a subtree is an action node")
    new_id, kept = {node: 0}, [node]
    for i in range(node + 1, len(nodes)):
        if nodes[i]["parent"] in new_id:
            new_id[i] = len(kept)
            kept.append(i)
    order = sorted(nodes[i]["index"] for i in kept if nodes[i]["kind"] == "action")
    renumber = {ix: k for k, ix in enumerate(order)}
    r0 = nodes[node]["round_idx"]
    sub = []
    for i in kept:
        nd = dict(nodes[i])
        nd["parent"] = -1 if i == node else new_id[nd["parent"]]
        nd["children"] = [new_id[c] for c in nd["children"]]
        if nd["kind"] == "action":
            nd["index"], nd["round_idx"] = renumber[nd["index"]], nd["round_idx"] - r0
        sub.append(nd)
    return sub, np.array(kept, dtype=np.int32)


def index_map(nodes, sub, node_map):
    """int [the subtree's action nodes]: the trunk's action index of the subtree's action index"""
    out = np.full(sum(nd["kind"] == "action" for nd in sub), -1, dtype=np.int64)
    for i, nd in enumerate(sub):
        if nd["kind"] == "action":
            out[nd["index"]] = nodes[int(node_map[i])]["index"]
    return out


# ---- the walk with a root reach ----------------------------------------------------------------------------------------------------------------------------------
def _matrices(g, p, reverse):
    live = (g.W > 0).astype(np.float64)
    if p == 0:
        M_fold, M_show = g.W, g.W * g.S
    else:
        M_fold, M_show, live = g.W.transpose(0, 2, 1), -(g.W * g.S).transpose(0, 2, 1), live.transpose(0, 2, 1)
    if reverse:
        M_fold, M_show, live = (np.ascontiguousarray(x[:, :, ::-1]) for x in (M_fold, M_show, live))
    return M_fold, M_show, live


def _leaf(M, live, q, reverse):
    return nbr._leaf(M, live, np.ascontiguousarray(q[:, ::-1]) if reverse else q)


def walk(nodes, R, S, game, cids, p, q0, rmplus=False, reverse=False):
    """one sweep of traverser p over R, S (updated in place) with the opponent's reach q0 [NB][n_o] at the root; returns the root row [NB][n_p]"""
    g, o = game, 1 - p
    M_fold, M_show, live = _matrices(g, p, reverse)
    dealt = ~g.blocked[p]

    def per_info_set(flat, x, C):
        w = np.where(dealt, x, 0.0).reshape(-1)
        if reverse:
            return np.bincount(flat[::-1], weights=w[::-1], minlength=C + 1)[:C]
        return np.bincount(flat, weights=w, minlength=C + 1)[:C]

    def rec(i, q, pi):
        nd = nodes[i]
        if nd["kind"] == "terminal":
            pot = float(np.float32(nd["value"]))
            if nd["ttype"] == "UNCONTESTED":
                return _leaf(M_fold, live, q, reverse) * (-pot if p == nd["last_to_act"] else pot)
            return _leaf(M_show, live, q, reverse) * pot
        if nd["kind"] != "action":
            return rec(nd["children"][0], q, pi)
        idx, r = nd["index"], nd["round_idx"]
        sig = npr.get_strategy_f32(R[idx]).astype(np.float64)
        if nd["player"] != p:
            so = np.where(g.blocked[o][None, :, :], 0.0, sig[:, g.infoset_of(cids, r, o)])
            total = 0.0
            for a, ch in enumerate(nd["children"]):
                total = total + rec(ch, q * so[a], pi)
            return total
        k = g.infoset_of(cids, r, p)
        sk = sig[:, k]
        vch = np.stack([rec(ch, q, pi * sk[a]) for a, ch in enumerate(nd["children"])])
        v = np.zeros(k.shape)
        for a in range(len(vch)):
            v = v + sk[a] * vch[a]
        C = sig.shape[1]
        flat = np.where(dealt, k, C).reshape(-1)
        sums = np.stack([per_info_set(flat, vch[a], C) for a in range(len(vch))])
        P = per_info_set(flat, pi, C)
        U = np.zeros(C)
        for a in range(len(vch)):
            U = U + sig[a] * sums[a]
        used = np.bincount(flat, minlength=C + 1)[:C] > 0
        with np.errstate(over="ignore", invalid="ignore"):
            Rn = (R[idx].astype(np.float64) + (sums - U[None, :])).astype(F32)
            if rmplus:
                Rn = np.where(Rn > 0, Rn, F32(0.0)).astype(F32)
            Sn = (S[idx].astype(np.float64) + P[None, :] * sig).astype(F32)
        R[idx] = np.where(used[None, :], Rn, R[idx])
        S[idx] = np.where(used[None, :], Sn, S[idx])
        return np.where(dealt, v, 0.0)

    return rec(0, np.asarray(q0, dtype=np.float64), np.ones((len(g.ro), g.n[p])))


# ---- the gadget ----------------------------------------------------------------------------------------------------------------------------------------------------
def new_gadget(resolver, alt):
    alt = np.asarray(alt, dtype=np.float64).reshape(-1)
    assert resolver in (0, 1) and np.isfinite(alt).all()
    return dict(resolver=resolver, alt=alt, regret=np.zeros((2, len(alt)), dtype=F32), ssum=np.zeros((2, len(alt)), dtype=F32))


def gadget_sweep(nodes, R, S, G, game, cids, p, rmplus=False, reverse=False, detail=None):
    """one sweep of traverser p of the game with gadget G above the root (R, S and, on the opponent's sweep, G's rows updated in place); returns the value.
    detail: a dict that receives S0, S1 (the opponent's sweep) or root, term (the resolver's)"""
    g, P = game, G["resolver"]
    O = 1 - P
    NB, alt = len(g.ro), G["alt"]
    assert len(alt) == g.n[O]
    with np.errstate(over="ignore", invalid="ignore"):
        sig = npr.get_strategy_f32(G["regret"]).astype(np.float64)                # [2][n_O]
    ones = np.ones((NB, g.n[O]))
    if p == P:
        root = walk(nodes, R, S, g, cids, p, ones * sig[1][None, :], rmplus, reverse)
        M_fold, _, live = _matrices(g, p, reverse)
        term = _leaf(M_fold, live, (ones * sig[0][None, :]) * alt[None, :], reverse) * -1.0
        if detail is not None:
            detail.update(root=root, term=term)
        return float(root.sum() + term.sum())
    vF = walk(nodes, R, S, g, cids, p, np.ones((NB, g.n[P])), rmplus, reverse)
    M_fold, _, live = _matrices(g, p, reverse)
    m = _leaf(M_fold, live, np.ones((NB, g.n[P])), reverse)
    dealt = ~g.blocked[O]
    with np.errstate(over="ignore", invalid="ignore"):
        vT = alt[None, :] * m
        S0, S1, Pi = np.zeros(g.n[O]), np.zeros(g.n[O]), np.zeros(g.n[O])
        for b in (range(NB - 1, -1, -1) if reverse else range(NB)):             # a lane that is no deal is not added
            S0 = np.where(dealt[b], S0 + vT[b], S0)
            S1 = np.where(dealt[b], S1 + vF[b], S1)
            Pi = np.where(dealt[b], Pi + 1.0, Pi)
        U = np.zeros(g.n[O])
        U = U + sig[0] * S0
        U = U + sig[1] * S1
        Rn = (G["regret"].astype(np.float64) + (np.stack([S0, S1]) - U[None, :])).astype(F32)
        if rmplus:
            Rn = np.where(Rn > 0, Rn, F32(0.0)).astype(F32)
        Sn = (G["ssum"].astype(np.float64) + Pi[None, :] * sig).astype(F32)
        v = np.zeros((NB, g.n[O]))
        v = v + sig[0][None, :] * vT
        v = v + sig[1][None, :] * vF
    used = dealt.any(axis=0)
    G["regret"] = np.where(used[None, :], Rn, G["regret"])
    G["ssum"] = np.where(used[None, :], Sn, G["ssum"])
    v = np.where(dealt, v, 0.0)
    if detail is not None:
        detail.update(S0=S0, S1=S1, used=used)
    return float(v.sum())


def gadget_discount(G, pos, neg, sm):
    """a Discounted CFR tick on the gadget rows: np_range_cfr.discount's rule, one f32 multiply per cell"""
    G["regret"] = np.where(G["regret"] > 0, G["regret"] * F32(pos), G["regret"] * F32(neg)).astype(F32)
    G["ssum"] = (G["ssum"] * F32(sm)).astype(F32)


def gadget_train(nodes, R, S, G, game, cids, iterations, rmplus=False, dcfr=None):
    """iterations of (traverser 0, traverser 1) with np_range_cfr.train's ticks (dcfr = (alpha, beta, gamma), a tick per iteration), gadget rows included"""
    import np_range_cfr as nrc
    values = [0.0, 0.0]
    for t in range(1, iterations + 1):
        for p in (0, 1):
            values[p] = gadget_sweep(nodes, R, S, G, game, cids, p, rmplus)
        if dcfr is not None:
            f = nrc.dcfr_factors(dcfr[0], dcfr[1], dcfr[2], t)
            nrc.discount(R, S, *f)
            gadget_discount(G, *f)
    return np.array(values)


# ---- the recipe ----------------------------------------------------------------------------------------------------------------------------------------------------
def prepare(nodes, tables, board0, hands, cids, node, prefix, resolver, current=False, prior=(None, None), game=None):
    """what rustsolver_amd.resolve.prepare returns, from the trunk's tables (R, S) and the trunk's game (np_br.Game or np_weighted.WeightedGame; default: Game)"""
    g = game or nbr.Game(board0, hands)
    P, O = resolver, 1 - resolver
    r0 = nodes[node]["round_idx"]
    sigma = nnr.strategies(tables, current=current).__getitem__
    rep = [nnr.report(nodes, sigma, g, cids, p)[node] for p in (0, 1)]
    board = [int(c) for c in g.ro[prefix * g.per_prefix[r0]][: len(board0) + r0]]
    pr = [np.ones(g.n[p]) if prior[p] is None else np.asarray(prior[p], dtype=np.float64) for p in (0, 1)]
    w = [None, None]
    w[P] = rep[P]["own"][prefix] * pr[P]
    w[O] = np.where((g.hands[O][:, :, None] == np.array(board)[None, None, :]).any(axis=(1, 2)), 0.0, pr[O])
    keep = [x != 0.0 for x in w]
    value, mass = rep[O]["value"][prefix], rep[O]["mass"][prefix]
    alt = np.where(mass > 0, value / np.where(mass > 0, mass, 1.0), 0.0)[keep[O]]
    pf0 = len(g.ro) // g.per_prefix[r0]                                            # prefixes of the node's round
    sub_cids, foreign = [], []
    for r in range(r0, len(cids)):
        k = (len(g.ro) // g.per_prefix[r]) // pf0                                   # prefixes of round r under one prefix of round r0
        rows, other = [], []
        for p in (0, 1):
            c = np.asarray(cids[r][p]).reshape(-1, g.n[p])
            mine = np.zeros(len(c), dtype=bool)
            mine[prefix * k:(prefix + 1) * k] = True
            rows.append(np.ascontiguousarray(c[mine][:, keep[p]]).astype(np.uint32))
            other.append(np.unique(c[~mine]))
        sub_cids.append(rows)
        foreign.append(other)
    sub, node_map = cut(nodes, node)
    return dict(nodes=sub, node_map=node_map, index_map=index_map(nodes, sub, node_map), board=board, hands=[g.hands[p][keep[p]] for p in (0, 1)], keep=keep,
                clusters=sub_cids, weights=[w[p][keep[p]] for p in (0, 1)], alt=alt, resolver=P, round0=r0, foreign=foreign)


def sub_tables(tables, prepared):
    """copies of the trunk's rows of the subtree's nodes, keyed by the subtree's action index (ids are kept: same shapes)"""
    R, S = tables
    return ({k: R[int(t)].copy() for k, t in enumerate(prepared["index_map"])}, {k: S[int(t)].copy() for k, t in enumerate(prepared["index_map"])})


def graft(sub, trunk, prepared, player):
    """the player's rows (regrets and strategy sums) of the subtree's nodes back into the trunk's tables, for the cluster ids that occur under the prefix"""
    for nd in prepared["nodes"]:
        if nd["kind"] != "action" or nd["player"] != player:
            continue
        r = nd["round_idx"]
        ids = np.unique(prepared["clusters"][r][player])
        if np.intersect1d(ids, prepared["foreign"][r][player]).size:
            raise ValueError("cluster ids of the subgame also occur under another prefix of the same round: the abstraction shares these cells across boards")
        t = int(prepared["index_map"][nd["index"]])
        for k in (0, 1):
            trunk[k][t][:, ids] = sub[k][nd["index"]][:, ids]
