"""Whole-sweep restatement of the reference tree walks (numpy, vectorised over lanes and deals).

TEST INFRASTRUCTURE ONLY -- PARITY UNPINNED (see oracle/rs_oracle.h).  This is the second reading of the
walks of src/solver/cfr.rs, written from the Rust source and the lane / deal models of DESIGN.md section 2,
NOT from the C oracle (rs_oracle.c): it never loads librs_oracle.so.  Tests compare the two readings with each
other (tests/test_np_walk_cpu.py) and the device with this one directly (tests/test_gpu_walk_restated.py), so
that a misreading shared by the C oracle and the kernels written to match it does not go unseen.

The per-node arithmetic is np_restate's (get_strategy, update, update_f32, node_util, weighted_index,
sample_bits, discount).  What this file adds is the recursion:

  * mccfr()  cfr.rs:299-479 -- chance nodes pass through (:306-313), the opponent samples ONE action
    (:467-476), the traverser prunes (:379-386, :413-441);
  * cfr()    cfr.rs:481-627 -- public chance enumerates (:502-522), every opponent action is recursed with
    reach * sigma[a] (:583-586) and util summed (:588), the traverser update without clamp (:612-621);
  * train()  cfr.rs:188-265 -- both players per iteration, then the discount thread's tick rule (:239-263).

Lanes (iterate_lanes): lane = board * n_clusters + cluster of the node's round; get_cluster() returns the
lane (cfr.rs:361-365 / :564-568), evaluate() is replaced by leaf inputs.  Deals (iterate_deals): a deal carries
one cluster id per (round, player); the sweep is batch-synchronous.

Every f32 sum here is sequential, in the order the Rust adds: no np.sum, no matmul, no reduceat.
"""
import numpy as np

from oracle import np_restate as npr

F32 = np.float32
U32 = np.uint32
PRUNE_THRESHOLD = npr.PRUNE_THRESHOLD            # cfr.rs:352 (i32 regrets)

# node kinds (nodes.rs:46-52) and terminal types (nodes.rs:16-21) as np_restate.build_tree spells them
PRIVATE, PUBLIC, ACTION, TERMINAL = "private_chance", "public_chance", "action", "terminal"
_KIND = {0: PRIVATE, 1: PUBLIC, 2: ACTION, 3: TERMINAL}
_TTYPE = {0: "ALLIN", 1: "SHOWDOWN", 2: "UNCONTESTED"}


def tree_from_records(records):
    """Node dicts (np_restate.build_tree's form) from the C-ABI node records of rs.GameTree.nodes (kind, parent, n_children,
    children[], index, player, round_idx, value, ttype, last_to_act, round), numbered as given."""
    out = []
    for rec in records:
        d = dict(kind=_KIND[int(rec.kind)], parent=int(rec.parent), children=[int(rec.children[k]) for k in range(int(rec.n_children))])
        if d["kind"] == ACTION:
            d.update(player=int(rec.player), index=int(rec.index), round_idx=int(rec.round_idx))
        elif d["kind"] == TERMINAL:
            d.update(value=int(rec.value), ttype=_TTYPE[int(rec.ttype)], last_to_act=int(rec.last_to_act), round=int(rec.round))
        out.append(d)
    return out


def _terminal(nd, player, leaf, where):
    """cfr.rs:314-348 (== :523-557).  leaf = ("sign", buf) | ("util", buf) | None; `where` indexes buf (lanes or deals)."""
    v = F32(nd["value"])                                            # tn.value as f32
    n = len(where)
    if nd["ttype"] == "UNCONTESTED":                                # :316-322
        return np.full(n, F32(-1.0) * v if player == nd["last_to_act"] else F32(1.0) * v, dtype=F32)
    kind, buf = leaf
    x = np.asarray(buf, dtype=F32)[where]
    if kind == "util":                                              # a leaf input: the traverser's utility, verbatim
        return x.copy()
    # SHOWDOWN :323-334 / ALLIN :335-347: buf = sign(score0 - score1); equal scores -> 0.0, else +-value for the traverser
    wins = x > 0 if player == 0 else x < 0
    return np.where(x == 0, F32(0.0), np.where(wins, F32(1.0) * v, F32(-1.0) * v)).astype(F32)


def _visit_i32(R, S, U, reach, scale, mode, rmplus, prune_lane):
    """the traverser's update of cfr.rs:413-464 (clamp) / :612-621 (wrap) over lanes; prune_lane: bool per lane, the `prune` argument
    of mccfr() (cfr.rs:379-386 and :415-441: util over explored actions only, explored cells only updated).  RM+ floors the clamped
    regret at 0 (extension, clamp arithmetic only)."""
    m = "rmplus" if rmplus else mode
    util = np.zeros(R.shape[1], dtype=F32)
    Rn, Sn = R.copy(), S.copy()
    for flag in (False, True):
        sel = prune_lane == flag
        if sel.any():
            util[sel], Rn[:, sel], Sn[:, sel] = npr.update(R[:, sel], S[:, sel], U[:, sel], reach[sel], scale, m, prune=flag)
    return util, Rn, Sn


class _Walk:
    def __init__(self, nodes, leaves, player, scale, mode, prune, rmplus, dtype, opp, seed):
        if dtype not in ("i32", "f32", "f16") or mode not in ("clamp", "wrap") or opp not in ("full", "sample"):
            raise ValueError("bad dtype / mode / opp")
        if prune and dtype != "i32":
            raise ValueError("prune compares i32 regrets (cfr.rs:352)")
        self.nodes, self.leaves, self.player = nodes, leaves, player
        self.scale, self.mode, self.prune, self.rmplus, self.dtype, self.opp, self.seed = F32(scale), mode, prune, rmplus, dtype, opp, seed

    def strategy(self, R):                                          # infoset.rs:83-102 (float tables: the same formula)
        return npr.get_strategy(R) if self.dtype == "i32" else npr.get_strategy_f32(R)

    def opponent(self, nd, sig, reach, hash_lane, recurse):
        """cfr.rs:467-476 (SAMPLE) or :576-589 (FULL) at an opponent node; recurse(child, subset, reach) -> util of the subset"""
        A, n = sig.shape
        if self.opp == "sample":
            a_idx = npr.weighted_index(sig, npr.sample_bits(self.seed, nd["index"], hash_lane))
            util = np.zeros(n, dtype=F32)
            for i, ch in enumerate(nd["children"]):
                sel = np.nonzero(a_idx == i)[0]
                if len(sel):
                    util[sel] = recurse(ch, sel, (reach[sel] * sig[i, sel]).astype(F32))   # cfr_reach * strategy[a_idx]
            return util
        U = np.zeros((A, n), dtype=F32)
        for i, ch in enumerate(nd["children"]):
            U[i] = recurse(ch, np.arange(n), (sig[i] * reach).astype(F32))                  # strategy[i] * cfr_reach
        return npr.node_util(sig, U)                                                       # util += utils[i] * strategy[i], in order


# ---------------------------------------------------------------------------------------------------
# lane sweeps: one cfr() / mccfr() per lane of the root round (DESIGN.md section 2 "Lane model")
# ---------------------------------------------------------------------------------------------------
def iterate_lanes(nodes, table, leaves, n_boards, n_clusters, player, scale=10000.0, mode="wrap", prune=False, rmplus=False,
                  dtype="i32", chance="enum", opp="full", seed=0):
    """One sweep of traverser `player` over every lane of the root round; updates `table` in place and returns the root utilities
    [n_boards[0] * n_clusters].

    nodes: np_restate.build_tree / tree_from_records dicts.  table: {ActionNode.index: (R, S)}, arrays [A, n_boards[round] * n_clusters]
    (int32, or float32 holding binary32 / binary16 values).  leaves: {node id: ("sign" | "util", float32 [lanes of that round])} for every
    showdown / all-in terminal.  chance: "enum" (cfr.rs:502-522) or "pass" (:306-313).  opp: "full" (:583-588) or "sample" with the
    sweep's seed (:467-476).  mode: "clamp" (:445-461) or "wrap" (:616-619); prune: cfr.rs:379-386; rmplus: regrets floored at 0 on write."""
    w = _Walk(nodes, leaves, player, scale, mode, prune, rmplus, dtype, opp, seed)
    C = int(n_clusters)

    def walk(nid, lanes, reach, r):
        nd = nodes[nid]
        if nd["kind"] == PRIVATE:                                   # cfr.rs:310-313: the hole-card combos ARE the lanes
            return walk(nd["children"][0], lanes, reach, r)
        if nd["kind"] == PUBLIC:
            if chance == "pass":                                    # cfr.rs:306-309: the lane's own board is the deal
                return walk(nd["children"][0], lanes, reach, r + 1)
            fan = int(n_boards[r + 1]) // int(n_boards[r])          # possible_deals.len()
            child_reach = (reach * (F32(1.0) / F32(fan))).astype(F32)   # cfr_reach * (1.0 / len as f32), cfr.rs:508
            b, c = lanes // C, lanes % C
            kids = ((b[:, None] * fan + np.arange(fan)[None, :]) * C + c[:, None]).reshape(-1)   # board b' = b * fan + d
            u = walk(nd["children"][0], kids, np.repeat(child_reach, fan), r + 1).reshape(len(lanes), fan)
            util = np.zeros(len(lanes), dtype=F32)
            for d in range(fan):                                    # util.store(util.load() + u), deals in order, cfr.rs:519
                util = (util + u[:, d]).astype(F32)
            return util
        if nd["kind"] == TERMINAL:
            return _terminal(nd, player, leaves.get(nid), lanes)
        R, S = table[nd["index"]]
        Rl, Sl = R[:, lanes], S[:, lanes]
        sig = w.strategy(Rl)
        A, n = Rl.shape
        if nd["player"] != player:
            return w.opponent(nd, sig, reach, lanes, lambda ch, sel, rr: walk(ch, lanes[sel], rr, r))
        explored = (Rl > PRUNE_THRESHOLD) if prune else np.ones((A, n), dtype=bool)   # cfr.rs:380
        U = np.zeros((A, n), dtype=F32)                             # skipped children keep utils[i] = 0 (cfr.rs:372)
        for i, ch in enumerate(nd["children"]):
            sel = np.nonzero(explored[i])[0]
            if len(sel):
                U[i, sel] = walk(ch, lanes[sel], reach[sel], r)
        if dtype == "i32":
            util, Rn, Sn = _visit_i32(Rl, Sl, U, reach, scale, mode, rmplus, np.full(n, bool(prune)))
        else:
            util, Rn, Sn = npr.update_f32(Rl, Sl, U, reach, scale, rmplus=rmplus, f16=(dtype == "f16"))
        R[:, lanes], S[:, lanes] = Rn, Sn                           # lanes never share cells: one visit per cell and sweep
        return util

    n0 = int(n_boards[0]) * C
    with np.errstate(all="ignore"):
        return walk(0, np.arange(n0), np.ones(n0, dtype=F32), 0)   # self.cfr(0, player, hand, 1f32, ..), cfr.rs:217/:222


# ---------------------------------------------------------------------------------------------------
# deal sweeps: sampled mccfr() over a batch of deals, batch-synchronous (DESIGN.md section 2 "Deal batches")
# ---------------------------------------------------------------------------------------------------
def _deal_order_sums(cells, deltas, n_cells):
    """out[c] = ((0.0 + d_k0) + d_k1) + ..., the deltas of cell c in the order given (deal order): a stable sort by cell, each member's rank
    inside its cell, then one vector add per rank -- sequential per cell, vectorised across cells"""
    acc = np.zeros(n_cells, dtype=F32)
    if len(cells) == 0:
        return acc
    order = np.argsort(cells, kind="stable")
    cs = cells[order]
    first = np.r_[True, cs[1:] != cs[:-1]]
    run_start = np.maximum.accumulate(np.where(first, np.arange(len(cs)), 0))
    rank = np.arange(len(cs)) - run_start
    dv = deltas[order]
    for k in range(int(rank.max()) + 1):
        m = rank == k
        acc[cs[m]] = (acc[cs[m]] + dv[m]).astype(F32)               # cells are distinct within one rank
    return acc


def iterate_deals(nodes, table, leaves, cidx, player, scale=100.0, mode="clamp", prune=False, prune_deal=None, rmplus=False,
                  dtype="i32", opp="sample", seed=0, lane_base=0):
    """One batch-synchronous sweep of traverser `player` over a batch of deals; updates `table` in place, returns the root utility per deal.

    table: {ActionNode.index: (R, S)}, arrays [A, clusters of (round_idx, player) of that node] (infoset.rs:28-32).  cidx[(round_idx,
    player)]: uint32 [n_deals], what get_cluster() returned (cfr.rs:361-365).  leaves: {node id: ("sign" | "util", float32 [n_deals])}.
    prune_deal: uint8 [n_deals], the `prune` argument of mccfr() per deal (cfr.rs:213-221; None = every deal); lane_base: global number of
    deal 0, the lane of the sampling hash (data-parallel batches).

    Every deal reads the table as it was when the sweep started.  i32: each traverser visit becomes the wrapping delta new - old against
    that snapshot; the deltas of a cell are added with wrapping adds and applied after the sweep.  f32 / f16: a visit contributes
    (scale*reach)*(u - util) and (scale*reach)*sigma; a cell's contributions are summed from 0.0 in deal order, added to the cell and
    rounded once to the storage type, the RM+ floor applied there; every cell of the traverser's rows is written, nobody else's."""
    w = _Walk(nodes, leaves, player, scale, mode, prune, rmplus, dtype, opp, seed)
    n_deals = len(next(iter(cidx.values())))
    flags = np.ones(n_deals, dtype=bool) if prune_deal is None else np.asarray(prune_deal).astype(bool)
    touched = {}                                                    # index -> [(clusters, dR, dS)] (float) or (DR, DS) (i32)

    def walk(nid, deals, reach):
        nd = nodes[nid]
        if nd["kind"] in (PRIVATE, PUBLIC):                         # cfr.rs:306-313: one run-out per deal
            return walk(nd["children"][0], deals, reach)
        if nd["kind"] == TERMINAL:
            return _terminal(nd, player, leaves.get(nid), deals)
        cl = np.asarray(cidx[(nd["round_idx"], nd["player"])], dtype=np.int64)[deals]
        R, S = table[nd["index"]]
        Rl, Sl = R[:, cl], S[:, cl]                                 # the snapshot
        sig = w.strategy(Rl)
        A, n = Rl.shape
        if nd["player"] != player:
            return w.opponent(nd, sig, reach, np.uint64(lane_base) + deals.astype(np.uint64), lambda ch, sel, rr: walk(ch, deals[sel], rr))
        pr = flags[deals] if prune else np.zeros(n, dtype=bool)
        explored = (Rl > PRUNE_THRESHOLD) | ~pr[None, :]            # cfr.rs:379-386 where this deal prunes
        U = np.zeros((A, n), dtype=F32)
        for i, ch in enumerate(nd["children"]):
            sel = np.nonzero(explored[i])[0]
            if len(sel):
                U[i, sel] = walk(ch, deals[sel], reach[sel])
        if dtype == "i32":
            util, Rn, Sn = _visit_i32(Rl, Sl, U, reach, scale, mode, rmplus, pr)
            DR, DS = touched.setdefault(nd["index"], (np.zeros(R.shape, dtype=U32), np.zeros(S.shape, dtype=U32)))
            for i in range(A):                                      # uint32 adds wrap: the order does not matter
                np.add.at(DR[i], cl, Rn[i].view(U32) - Rl[i].view(U32))
                np.add.at(DS[i], cl, Sn[i].view(U32) - Sl[i].view(U32))
            return util
        util = npr.node_util(sig, U)                                # cfr.rs:384/:391
        k = (w.scale * reach).astype(F32)                           # (100.0 * cfr_reach) first, cfr.rs:445
        dR = (k * (U - util).astype(F32)).astype(F32)
        dS = (k * sig).astype(F32)
        touched.setdefault(nd["index"], []).append((cl, dR, dS))
        return util

    with np.errstate(all="ignore"):
        root = walk(0, np.arange(n_deals), np.ones(n_deals, dtype=F32))
        for nd in nodes:
            if nd["kind"] != ACTION:
                continue
            idx = nd["index"]
            R, S = table[idx]
            if dtype == "i32":
                if idx in touched:
                    DR, DS = touched[idx]
                    table[idx] = ((R.view(U32) + DR).view(np.int32), (S.view(U32) + DS).view(np.int32))
                continue
            if nd["player"] != player:
                continue
            parts = touched.get(idx, [])
            A, n_cells = R.shape
            cells = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
            Rn, Sn = np.empty_like(R), np.empty_like(S)
            for i in range(A):
                accR = _deal_order_sums(cells, np.concatenate([p[1][i] for p in parts]) if parts else np.zeros(0, F32), n_cells)
                accS = _deal_order_sums(cells, np.concatenate([p[2][i] for p in parts]) if parts else np.zeros(0, F32), n_cells)
                r = (R[i] + accR).astype(F32)
                if rmplus:
                    r = np.where(r > 0, r, F32(0.0)).astype(F32)     # !(r > 0) -> 0: NaN too
                s = (S[i] + accS).astype(F32)
                Rn[i], Sn[i] = (npr.round_f16(r), npr.round_f16(s)) if dtype == "f16" else (r, s)
            table[idx] = (Rn, Sn)
    return root


# ---------------------------------------------------------------------------------------------------
# discount and train() (cfr.rs:188-265)
# ---------------------------------------------------------------------------------------------------
def discount_table(table, d, dtype="i32"):
    """cfr.rs:250-258 over every info set: x = (x as f32 * d) as i32; float tables: x * d in f32, rounded to the storage type"""
    d = F32(d)
    for idx, (R, S) in list(table.items()):
        if dtype == "i32":
            table[idx] = (npr.discount(R, d), npr.discount(S, d))
        else:
            with np.errstate(all="ignore"):
                r, s = (R * d).astype(F32), (S * d).astype(F32)
            table[idx] = (npr.round_f16(r), npr.round_f16(s)) if dtype == "f16" else (r, s)


def train_lanes(nodes, table, leaves, n_boards, n_clusters, iterations, discount_interval=100_000, discount_cap=20_000_000, dtype="i32",
                seed_of_sweep=None, **kw):
    """train() made deterministic over lanes: per iteration both players sweep (cfr.rs:216-224), t += 1 (:226); the discount thread's
    check then runs once: it stops for good once t > DISCOUNT_CAP (:240-242), and when t > threshold it discounts every info set by
    d = p / (p + 1), p = (t / DISCOUNT_INTERVAL) as f32 (:243-258), and moves threshold to t + DISCOUNT_INTERVAL (:262).
    seed_of_sweep(k): the sampling seed of the k-th sweep (opp="sample" only)."""
    t, threshold, sweeps = 0, discount_interval, 0
    while t < iterations:                                           # cfr.rs:207
        for player in (0, 1):
            seed = seed_of_sweep(sweeps) if seed_of_sweep else 0
            iterate_lanes(nodes, table, leaves, n_boards, n_clusters, player, dtype=dtype, seed=seed, **kw)
            sweeps += 1
        t += 1
        if t > discount_cap:
            continue
        if t > threshold:
            discount_table(table, npr.discount_factor(t, discount_interval), dtype)
            threshold = t + discount_interval
    return t
