"""CPU: the numpy restatement of the node report (tests/np_node_report.py) against the identities its definition implies, on the cases tests/test_gpu_node_report.py
holds the device to.

  * a second summation order (every fold and every leaf reversed) agrees with the restatement's own within RTOL, ATOL of test_np_br_cpu ("two summation orders of the
    same f64 sums"): the tolerance of the GPU comparison;
  * the root's mass sums to 1 (the deal weights are a distribution) and the root's value to np_br.best_response(mode="avg");
  * sum over (f, h) of own * mass is the probability of reaching the node: the same number from either traverser's report;
  * at an own node value = sum_a sigma[a][cluster] * cfv[a]; a child action node's value is its parent's cfv[a], folded over the child's prefixes where a chance node
    lies between them.
"""
import numpy as np
import pytest

import np_node_report as nnr
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_gpu_range_cfr import make_case
from test_np_br_cpu import ATOL, FLOP, RTOL, pick_ranges, random_cids
from test_range_cfr_cpu import FLOP_TREE, random_tables

CASES = ["river_lanes", "river_wave_35", "turn_imperfect_recall", "turn_one_hand", "turn_no_opponent", "flop_three_rounds"]

# games in which some run-outs admit no deal at all (a one-hand range that two turn cards block; hands that meet no opponent): generate_hand has nothing to draw there, the
# weights of the run-outs that do admit one sum to less than 1, and so does the root's mass
DEGENERATE = {"turn_one_hand", "turn_no_opponent"}


def report_case(name):
    """-> board0, hands, cids, table sizes, (bet sizes, raise sizes): test_gpu_range_cfr.make_case's, and one flop-start game -- 6 x 5 hands, three rounds, 2 352 run-outs,
    one bet size per round: the fold lengths 2 352 / 48 / 1 in one call"""
    if name != "flop_three_rounds":
        return make_case(name)
    rng = np.random.Generator(np.random.PCG64(7))
    h = pick_ranges(rng, FLOP, 6, 5)
    sizes = [(2, 3), (3, 2), (4, 3)]
    return FLOP, h, random_cids(rng, FLOP, h, sizes), sizes, FLOP_TREE


_SETUPS = {}


def setup(name):
    """the case with its restated tree, game and random f32 tables; built once and left unchanged"""
    if name not in _SETUPS:
        board0, h, cids, sizes, tree = report_case(name)
        nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
        tables = random_tables(np.random.Generator(np.random.PCG64(61)), nodes, sizes)
        _SETUPS[name] = dict(board0=board0, h=h, cids=cids, sizes=sizes, tree=tree, nodes=nodes, game=nbr.Game(board0, h), tables=tables)
    return _SETUPS[name]


_REPORTS = {}


def restated(name, p, current=False, reverse=False):
    key = (name, p, current, reverse)
    if key not in _REPORTS:
        s = setup(name)
        sig = nnr.strategies(s["tables"], current)
        _REPORTS[key] = nnr.report(s["nodes"], sig.__getitem__, s["game"], s["cids"], p, reverse)
    return _REPORTS[key]


def first_action(nodes):
    """the root of the betting: the tree's node 0 is the deal"""
    i = 0
    while nodes[i]["kind"] != "action":
        i = nodes[i]["children"][0]
    return i


def rows_of(block):
    return [("cfv", block["cfv"]), ("value", block["value"]), ("mass", block["mass"]), ("own", block["own"])]


def close(a, b, what, rtol=RTOL, atol=ATOL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (what, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name", CASES)
def test_every_action_node_is_reported_in_the_shape_of_its_round(name):
    s = setup(name)
    g = s["game"]
    for p in (0, 1):
        rep = restated(name, p)
        assert sorted(rep) == [i for i, nd in enumerate(s["nodes"]) if nd["kind"] == "action"]
        for i, block in rep.items():
            nd = s["nodes"][i]
            F = len(g.ro) // g.per_prefix[nd["round_idx"]]
            assert block["cfv"].shape == (len(nd["children"]), F, g.n[p])
            assert block["value"].shape == block["mass"].shape == block["own"].shape == (F, g.n[p])
    if name == "flop_three_rounds":
        assert len(g.ro) == 2352 and g.per_prefix == [2352, 48, 1] and g.n == [6, 5]


@pytest.mark.parametrize("current", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_a_second_summation_order_agrees(name, current):
    """forward and reverse folds and leaves, every row of every node, both traversers"""
    for p in (0, 1):
        fwd, rev = restated(name, p, current), restated(name, p, current, reverse=True)
        for i in fwd:
            for (row, a), (_, b) in zip(rows_of(fwd[i]), rows_of(rev[i])):
                close(a, b, (name, p, i, row))


@pytest.mark.parametrize("name", CASES)
def test_the_root_holds_the_whole_distribution_and_the_profiles_value(name):
    s = setup(name)
    first = first_action(s["nodes"])
    sig = nnr.strategies(s["tables"])
    want = nbr.best_response(s["nodes"], sig.__getitem__, None, None, s["cids"], "avg", None, s["game"])
    for p in (0, 1):
        root = restated(name, p)[first]
        assert abs(root["mass"].sum() - s["game"].W.sum()) <= 1e-12, (name, p, root["mass"].sum())
        if name not in DEGENERATE:
            assert abs(root["mass"].sum() - 1.0) <= 1e-12, (name, p, root["mass"].sum())
        assert (root["own"][~s["game"].blocked[p].all(axis=0)[None, :]] == 1.0).all()
        close(root["value"].sum(), want[p], (name, p, "root value"))


@pytest.mark.parametrize("name", CASES)
def test_own_reach_times_mass_is_the_probability_of_reaching_the_node(name):
    r0, r1 = restated(name, 0), restated(name, 1)
    seen = 0.0
    for i in r0:
        a, b = (r0[i]["own"] * r0[i]["mass"]).sum(), (r1[i]["own"] * r1[i]["mass"]).sum()
        close(a, b, (name, i))
        assert -ATOL <= a <= 1.0 + ATOL
        seen = max(seen, a)
    assert abs(seen - setup(name)["game"].W.sum()) <= 1e-12         # the root is reached by every deal


@pytest.mark.parametrize("name", CASES)
def test_values_of_parents_and_children_fit_together(name):
    s = setup(name)
    nodes, g, sig = s["nodes"], s["game"], nnr.strategies(s["tables"])
    own_nodes = same_round = behind_chance = 0
    for p in (0, 1):
        rep = restated(name, p)
        for i, block in rep.items():
            nd = nodes[i]
            r = nd["round_idx"]
            if nd["player"] == p:                                   # value = sum_a sigma[a][cluster] * cfv[a]
                k = np.asarray(s["cids"][r][p]).reshape(-1, g.n[p]).astype(np.int64)
                sk = sig[nd["index"]].astype(np.float64)[:, k]
                close((sk * block["cfv"]).sum(axis=0), block["value"], (name, p, i, "own node"))   # (a pair that is no deal looks an ignored id up: its rows are 0.0)
                no_deal = g.blocked[p].reshape(-1, g.per_prefix[r], g.n[p]).all(axis=1)
                assert all((x[..., no_deal] == 0).all() for _, x in rows_of(block)), (name, p, i)
                own_nodes += 1
            for a, ch in enumerate(nd["children"]):
                chance = False
                while nodes[ch]["kind"] not in ("action", "terminal"):
                    ch, chance = nodes[ch]["children"][0], True
                if nodes[ch]["kind"] != "action":
                    continue
                v = rep[ch]["value"]
                if chance:                                          # the child's prefixes under each of the parent's
                    F = block["value"].shape[0]
                    v = v.reshape(F, -1, g.n[p]).sum(axis=1)
                    behind_chance += 1
                else:
                    assert nodes[ch]["round_idx"] == r
                    same_round += 1
                close(v, block["cfv"][a], (name, p, i, a, "child"))
    assert own_nodes and same_round and (behind_chance or len(s["board0"]) == 5)


def test_block_layout_and_the_refusals_that_need_no_device():
    """rs_node_report_size against the shapes of the restatement; a bad request is refused before the game is prepared, with the output buffer untouched"""
    import ctypes as C

    import rustsolver_amd as rs
    from rustsolver_amd import _lib as L

    s = setup("turn_imperfect_recall")
    lib = L.load()
    _, tree = rs.build_game_tree(rs.Options(n_board_cards=len(s["board0"]), bet_sizes=s["tree"][0], raise_sizes=s["tree"][1]))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for p in (0, 1):
        rep = restated("turn_imperfect_recall", p)
        ids = np.array(sorted(rep)[::-1], dtype=np.int32)           # any order: the blocks follow the request
        off = np.zeros(len(ids), dtype=np.uint64)
        total = lib.rs_node_report_size(tree._h, len(s["board0"]), s["game"].n[p], vp(ids), len(ids), vp(off))
        sizes = [rep[int(i)]["cfv"].size + 3 * rep[int(i)]["value"].size for i in ids]
        assert total == sum(sizes) and off.tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    ids = np.array(sorted(rep), dtype=np.int32)
    terminal = next(i for i, nd in enumerate(s["nodes"]) if nd["kind"] == "terminal")
    for bad in ([0], [terminal], [int(ids[0]), int(ids[0])], [len(s["nodes"])], [-1], []):
        n = np.array(bad, dtype=np.int32)
        assert lib.rs_node_report_size(tree._h, len(s["board0"]), 9, vp(n), len(n), None) == 0, bad
        assert lib.rs_last_error().startswith(b"rs_node_report"), bad
    assert lib.rs_node_report_size(tree._h, 2, 9, vp(ids), len(ids), None) == 0 and lib.rs_node_report_size(tree._h, 4, 0, vp(ids), len(ids), None) == 0
    out = np.full(8, 7.0)
    call = lambda mode, p, n, doubles: lib.rs_node_report(None, tree._h, None, 4, None, 9, None, 7, None, 2, mode, p, vp(n), len(n), vp(out), doubles)
    for mode in (L.BR_MAX, L.BR_MAX | L.BR_SORTED, L.BR_MAX | L.BR_REAL, L.BR_AVERAGE | L.BR_REAL, L.BR_MAX | L.BR_CURRENT):
        assert call(mode, 0, ids, 8) == L.ERR_INVALID and b"report" in lib.rs_last_error(), mode
    assert call(L.BR_AVERAGE, 2, ids, 8) == L.ERR_INVALID and call(L.BR_AVERAGE, -1, ids, 8) == L.ERR_INVALID
    assert call(L.BR_AVERAGE, 0, np.array([terminal], dtype=np.int32), 8) == L.ERR_INVALID
    assert call(L.BR_AVERAGE | L.BR_CURRENT | L.BR_SORTED, 0, ids, 8) == L.ERR_INVALID and b"too small" in lib.rs_last_error()
    assert (out == 7.0).all()
