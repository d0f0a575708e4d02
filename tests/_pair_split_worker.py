"""Worker of tests/test_gpu_pair_split.py::test_split_on_equals_split_off: one process per RS_JIT_SPLIT setting.  Runs pair launches on the river tree over 4 099 lanes
(at most 3 workgroups: several trips and a ragged tail) with edge regrets and LEAF_UTIL rows of each traverser's own, the root-utility pointers null in turn, for i32
(clamp + RM+) and f16 tables, and writes the solver's forms, every root-utility buffer after every iteration and the final tables to the .npz named on the command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import rustsolver_amd as rs  # noqa: E402
from rustsolver_amd import _lib as L  # noqa: E402
from test_gpu_walk_restated import SENTINEL, carry_f16, carry_f16_utils, edge_i32, edge_utils  # noqa: E402

os.environ["RS_JIT_MAX_BLOCKS"] = "3"
N = 4099
PATTERN = [(False, False), (True, False), (False, True), (True, True)]
out = {}
lib = L.load()
for dtype in ("i32", "f16"):
    rng = np.random.Generator(np.random.PCG64(191))
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [N], [1], rs.I32 if dtype == "i32" else rs.F16, 0)
    for nd in tree.action_nodes():
        R, S = edge_i32(rng, nd.n_children, N) if dtype == "i32" else carry_f16(rng, nd.n_children, N)
        table.upload_node(nd.index, R, S)
    lv = [{}, {}]
    for i, nd in enumerate(tree.nodes):
        if nd.kind == rs.NODE_TERMINAL and nd.ttype != rs.TERM_UNCONTESTED:
            for p in (0, 1):   # J1.leaf != J.leaf: the second walk reads rows of its own
                u = edge_utils(rng, N) if dtype == "i32" else carry_f16_utils(rng, 0, N)[1]
                lv[p][i] = (rs.LEAF_UTIL, table.lane_buffer(tree.nodes[nd.parent].index, 1, u))
    mode = rs.UPD_CLAMP_I64 | (rs.UPD_RMPLUS if dtype == "i32" else 0)
    tr = rs.MCCFRTrainer(tree, table, lv[0], leaves_p1=lv[1], scale=100.0 if dtype == "i32" else 1.0, mode=mode, chance_mode=rs.CHANCE_PASS, fuse_subtrees=1)
    forms = lib.rs_solver_forms(tr._h)
    assert out.setdefault("forms", np.int64(forms)) == forms
    assert tr.n_launches(0) + tr.n_launches(1) == 1
    root = tree.nodes[tree.nodes[0].children[0]].index
    u = [table.lane_buffer(root, 1), table.lane_buffer(root, 1)]
    sent = np.full(table.pitch(root), SENTINEL, dtype=np.float32)
    for it, null in enumerate(PATTERN):
        for b in u:
            b.upload(sent)
        L.check(lib.rs_iterate(tr._h, 0, None if null[0] else u[0].ptr))
        L.check(lib.rs_iterate(tr._h, 1, None if null[1] else u[1].ptr))
        for p in (0, 1):
            got = table.read_lane_buffer(u[p], root)[0]
            if null[p]:
                assert (got == SENTINEL).all(), "a null root-utility pointer's buffer was written"
            out["%s root util p%d it=%d" % (dtype, p, it)] = got
    for nd in tree.action_nodes():
        r, s = table.download_node(nd.index)
        out["%s regrets of node %d" % (dtype, nd.index)] = r
        out["%s strategy sums of node %d" % (dtype, nd.index)] = s
    tr.destroy()
    table.destroy()
np.savez(sys.argv[1], **out)
