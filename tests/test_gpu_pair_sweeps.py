"""GPU: pair sweeps (rs_kernel_forms.pair_sweeps) -- both traversers of a chance-free lane tree in one launch, every node's regrets carried in registers from the first walk
to the second -- must leave what two separate sweeps leave, bit for bit: tables, both root utilities, the sampling seed's progress.  And a held traverser-0 sweep must come
out as a plain sweep in front of whatever else the caller does next."""
import ctypes as C

import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from test_gpu_walk_restated import assert_same, edge_float, edge_i32, edge_utils, float_utils

pytestmark = pytest.mark.gpu
ON, OFF = {"pair_sweeps": L.FORM_ON}, {"pair_sweeps": L.FORM_OFF}


def build(forms, C_=250, B=3, dtype=rs.I32, mode=rs.UPD_CLAMP_I64, opp=rs.OPP_FULL, util_leaves=False, scale=100.0, seed=5, table=None, graph=False):
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    if table is None:
        table = rs.create_infosets(n_actions, tree, [C_], [B], dtype, 0)
        if dtype == rs.F16:
            table.fill_random(seed, (-2000, 2000), (0, 2000))
        else:
            table.fill_random(seed, (-10**6, 10**6), (0, 10**6))
    lv = [{}, {}]
    bufs = {}
    for i, nd in enumerate(tree.nodes):
        if nd.kind == rs.NODE_TERMINAL and nd.ttype != rs.TERM_UNCONTESTED:
            parent = tree.nodes[nd.parent]
            n = table.pitch(parent.index)
            for p in (0, 1):
                key = (p if util_leaves else 0, parent.round_idx)
                if key not in bufs:
                    bufs[key] = table.lane_buffer(parent.index, 1)
                    lo, hi = (-300.0, 300.0) if util_leaves else (-1.0, 1.0)
                    L.check(L.load().rs_fill_uniform_f32(table._h, bufs[key].ptr, n, seed + 17 + 3 * p, lo, hi))
                lv[p][i] = (rs.LEAF_UTIL if util_leaves else rs.LEAF_SIGN, bufs[key])
    tr = rs.MCCFRTrainer(tree, table, lv[0], leaves_p1=lv[1], scale=scale, mode=mode, chance_mode=rs.CHANCE_PASS, fuse_subtrees=1, opp_mode=opp,
                         sample_seed=seed + 1, forms=forms, use_graph=graph)
    tr._keep = bufs
    table.sync()
    return tree, table, tr


def root_buffers(tree, table):
    root = tree.nodes[tree.nodes[0].children[0]]
    return root.index, table.lane_buffer(root.index, 1), table.lane_buffer(root.index, 1)


def state(tree, table):
    samples = []
    rng = np.random.Generator(np.random.PCG64(11))
    for nd in tree.nodes:
        if nd.kind == rs.NODE_ACTION and nd.n_children > 0:
            lanes = rng.integers(0, table.node_desc(nd.index).n_boards * table.node_desc(nd.index).n_clusters, size=64)
            samples.append(table.get_infosets(nd.index, lanes))
    return table.checksum(), samples


def same_state(a, b):
    assert a[0] == b[0], "table checksums differ"
    for (ra, sa), (rb, sb) in zip(a[1], b[1]):
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes()


CASES = {
    "clamp": dict(),
    "wrap": dict(mode=rs.UPD_WRAP_I32, scale=10000.0),
    "prune": dict(mode=rs.UPD_CLAMP_I64 | rs.UPD_PRUNE),
    "f32": dict(dtype=rs.F32, scale=1.0),
    "f16": dict(dtype=rs.F16, scale=1.0),
    "sampled": dict(opp=rs.OPP_SAMPLE, mode=rs.UPD_WRAP_I32, scale=10000.0),
    "leaf_util_p1": dict(util_leaves=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("size", ["small", "tiled"])
def test_pair_on_equals_pair_off(case, size):
    kw = dict(CASES[case])
    if size == "tiled":   # 1 100 000 lanes per node: tiled node blocks
        kw.update(C_=1000, B=1100)
    outs = []
    for forms in (ON, OFF):
        tree, table, tr = build(forms, **kw)
        assert tr.paired == (forms is ON)
        assert tr.n_launches(0) + tr.n_launches(1) == ((2 if case == "sampled" else 1) if forms is ON else (4 if case == "sampled" else 2))
        idx, u0, u1 = root_buffers(tree, table)
        utils = []
        for it in range(3):
            L.check(L.load().rs_iterate(tr._h, 0, u0.ptr if it != 1 else None))
            L.check(L.load().rs_iterate(tr._h, 1, u1.ptr))
            utils.append((table.read_lane_buffer(u0, idx)[0].tobytes() if it != 1 else b"", table.read_lane_buffer(u1, idx)[0].tobytes()))
        outs.append((state(tree, table), utils))
        tr.destroy()
        table.destroy()
    same_state(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1], "root utilities differ"


# Edge inputs (tests/test_gpu_walk_restated.py), pair ON against pair OFF.  The float ones overflow on BOTH players' nodes in the first iteration, so the second reads
# sigma = inf / inf = NaN: what a NaN reach does is the convention both forms share (test_float_nan_reach_still_updates), and they must still agree bit for bit -- the
# inputs test_pair_float_edges_lanes has to keep away from the numpy walk.  The i32 ones: INT32_MIN / MAX, the prune threshold, deltas across 2^31 and 2^32 under RM+.
EDGE_CASES = {
    "f16-overflow": dict(dtype="f16", iters=2),
    "f16-rmplus-overflow": dict(dtype="f16", rmplus=True, iters=2),
    "f32-overflow": dict(dtype="f32", iters=2),
    "f32-rmplus-overflow": dict(dtype="f32", rmplus=True, iters=2),
    "i32-edges-rmplus": dict(dtype="i32", rmplus=True, iters=3),
    "i32-edges-rmplus-prune": dict(dtype="i32", rmplus=True, prune=True, iters=3),
}


def run_edges(forms, dtype, iters, rmplus=False, prune=False, n=1021, seed=91):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [n], [1], {"i32": rs.I32, "f32": rs.F32, "f16": rs.F16}[dtype], 0)
    half = dtype == "f16"
    for nd in tree.action_nodes():
        R, S = edge_i32(rng, nd.n_children, n) if dtype == "i32" else edge_float(half, big_rows=True)(rng, nd.n_children, n)
        table.upload_node(nd.index, R, S)
    lv = [{}, {}]
    for i, nd in enumerate(tree.nodes):
        if nd.kind == rs.NODE_TERMINAL and nd.ttype != rs.TERM_UNCONTESTED:
            for p in (0, 1):   # LEAF_UTIL rows of each traverser's own
                u = edge_utils(rng, n) if dtype == "i32" else float_utils(half)(rng, 0, n)[1]
                lv[p][i] = (rs.LEAF_UTIL, table.lane_buffer(tree.nodes[nd.parent].index, 1, u))
    mode = rs.UPD_CLAMP_I64 | (rs.UPD_RMPLUS if rmplus else 0) | (rs.UPD_PRUNE if prune else 0)
    tr = rs.MCCFRTrainer(tree, table, lv[0], leaves_p1=lv[1], scale=100.0 if dtype == "i32" else 1.0, mode=mode, chance_mode=rs.CHANCE_PASS, fuse_subtrees=1, forms=forms)
    assert tr.paired == (forms is ON)
    assert tr.n_launches(0) + tr.n_launches(1) == (1 if forms is ON else 2)
    idx, u0, u1 = root_buffers(tree, table)
    out = []
    for it in range(iters):
        L.check(L.load().rs_iterate(tr._h, 0, u0.ptr))
        L.check(L.load().rs_iterate(tr._h, 1, u1.ptr))
        out.append(("root util p0 it=%d" % it, table.read_lane_buffer(u0, idx)[0]))
        out.append(("root util p1 it=%d" % it, table.read_lane_buffer(u1, idx)[0]))
    for nd in tree.action_nodes():
        r, s_ = table.download_node(nd.index)
        out += [("regrets of node %d" % nd.index, r), ("strategy sums of node %d" % nd.index, s_)]
    tr.destroy()
    table.destroy()
    return out


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_pair_on_equals_pair_off_at_edges(case):
    a, b = run_edges(ON, **EDGE_CASES[case]), run_edges(OFF, **EDGE_CASES[case])
    if not case.startswith("i32"):   # the case is about what follows an overflow: it must have happened
        assert any(np.isinf(x).any() for what, x in b if what.startswith("regrets"))
    for (what, x), (_, y) in zip(a, b):
        assert_same(x, y, what)   # bit for bit, every NaN one value


def run_interleaved(forms, what):
    tree, table, tr = build(forms, C_=1000, B=2)
    got = None
    node = next(nd.index for nd in tree.nodes if nd.kind == rs.NODE_ACTION and nd.n_children > 0 and nd.player == 0)
    lanes = np.arange(0, 2000, 7, dtype=np.uint32)
    for it in range(2):
        tr.iterate(0)
        if what == "get_infosets":
            got = table.get_infosets(node, lanes)
        elif what == "discount":
            table.discount(0.75)
        elif what == "sync_d2h":
            table.sync()
            got = table.download_node(node)
        elif what == "iterate0_again":
            tr.iterate(0)
        elif what == "other_solver":
            _, _, tr2 = build(forms, table=table)
            tr2.iterate(0)
            tr2.iterate(1)
            tr2.destroy()
        elif what == "destroy":
            tr.destroy()
            return state(tree, table), None
        tr.iterate(1)
    return state(tree, table), got


@pytest.mark.parametrize("what", ["get_infosets", "discount", "sync_d2h", "iterate0_again", "other_solver", "destroy"])
def test_held_sweep_interleavings(what):
    a, ga = run_interleaved(ON, what)
    b, gb = run_interleaved(OFF, what)
    same_state(a, b)
    if ga is not None:
        for x, y in zip(ga, gb):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_train_and_graph_replay_pair():
    """rs_train and hipGraph replay take the pair path and match the plain sweeps"""
    res = []
    for forms in (ON, OFF):
        tree, table, tr = build(forms, C_=1000, B=2, graph=True)
        tr.train(4, discount_interval=2, discount_cap=10)
        tr.iterate(0)
        tr.iterate(1)
        res.append(state(tree, table))
        tr.destroy()
    same_state(res[0], res[1])
