"""GPU (-m gpu): the split form of the pair kernel (rs_jit.cpp, rs_solver_forms bit 3).  A lane vector's subtree is cut below its root; waves of one kind walk the
subtree under one group of the root's children (part A), waves of the other kind the root and the rest (part B), and reaches and utilities cross through LDS between
barriers.  What comes out must be what one thread per lane vector leaves, bit for bit (NaN counted as one value): against the numpy walk at the numeric edges, at lane
counts that leave surplus threads in both parts and make several trips with a ragged tail, over plain and tiled rows, eager and replayed, and against the unsplit kernel
(RS_JIT_SPLIT=0) in a process of its own.  Sampled opponents and pruning keep the unsplit kernel.

All cases drive real pair launches: rs_iterate(h, 0, u0), rs_iterate(h, 1, u1) with nothing in between (run_pair_lanes of test_gpu_walk_restated.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rustsolver_amd as rs
import test_gpu_walk_restated as wr
from rustsolver_amd import _lib as L
from test_gpu_walk_restated import I32_UTILS, assert_same, carry_f16, carry_f16_utils, edge_float, edge_i32, float_utils, run_pair_lanes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: these tests need a real MI355X (there is no CPU fallback)")


@pytest.fixture
def checked(monkeypatch):
    """every solver run_pair_lanes creates must be paired, one launch per iteration, and in the form the case expects: checked(True) = split, checked(False) = unsplit"""
    def want(split):
        seen = []

        class Checked(rs.MCCFRTrainer):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                forms = L.load().rs_solver_forms(self._h)
                assert forms & 4, "not a paired solver"
                assert bool(forms & 8) == split, "forms = %d" % forms
                assert self.split_pair == split
                if kw.get("opp_mode", rs.OPP_FULL) == rs.OPP_FULL:
                    assert self.n_launches(0) + self.n_launches(1) == 1
                seen.append(forms)
        monkeypatch.setattr(wr.rs, "MCCFRTrainer", Checked)
        return seen
    monkeypatch.delenv("RS_JIT_SPLIT", raising=False)
    return want


def lane_case(C, layout, monkeypatch):
    """37 lanes: one partial workgroup, surplus threads in both parts.  4 099 lanes on at most 3 workgroups: 17 trips' worth of lane vectors, so several trips each and a
    ragged tail (the last trip leaves workgroups without a vector, and one with surplus threads)"""
    if layout == "tiled64":
        monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    if C == 4099:
        monkeypatch.setenv("RS_JIT_MAX_BLOCKS", "3")


@pytest.mark.parametrize("mode", ["clamp", "wrap", "clamp+rmplus"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("layout", ["plain", "tiled64"])
@pytest.mark.parametrize("C", [37, 4099])
def test_split_i32_edges_against_numpy_walk(mode, graph, layout, C, checked, monkeypatch):
    """edge regrets (INT32_MIN / MAX, the prune threshold, all non-positive rows), LEAF_UTIL leaves of each traverser's own whose deltas straddle 2^31 and 2^32; 3 iterations"""
    lane_case(C, layout, monkeypatch)
    seen = checked(True)
    run_pair_lanes(rs.default_flop(), [1], C, edge_i32, I32_UTILS, mode=mode.split("+")[0], rmplus="rmplus" in mode, scale=10000.0 if mode == "wrap" else 100.0,
                   graph=graph, seed=171, iters=3)
    assert seen


@pytest.mark.parametrize("dtype", ["f16", "f16+rmplus", "f32", "f32+rmplus"])
def test_split_float_edges_against_numpy_walk(dtype, checked):
    """the float edge inputs of test_pair_float_edges_lanes (NaN cells and utilities, -0.0, subnormal halves, rows near the largest finite value where no later walk reads
    what overflows), one iteration"""
    half = dtype.startswith("f16")
    seen = checked(True)
    run_pair_lanes(rs.default_flop(), [1], 1021, (edge_float(half, big_rows=False), edge_float(half)), (float_utils(half, big=False), float_utils(half)),
                   rmplus="rmplus" in dtype, dtype=dtype.split("+")[0], scale=1.0, seed=175, iters=1)
    assert seen


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("layout", ["plain", "tiled64"])
@pytest.mark.parametrize("C", [37, 4099])
def test_split_f16_carry_ties_and_subnormals(graph, layout, C, checked, monkeypatch):
    """binary16 rows whose updates round (ties to even, subnormal halves, spacing 32 below 65 504): the root's regrets cross from the first walk to the second inside part B,
    the others inside part A, each as binary16 would give them back; 3 iterations"""
    lane_case(C, layout, monkeypatch)
    seen = checked(True)
    run_pair_lanes(rs.default_flop(), [1], C, carry_f16, carry_f16_utils, dtype="f16", scale=1.0, graph=graph, seed=173, iters=3)
    assert seen


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_split_null_root_utilities(graph, checked, monkeypatch):
    """either root-utility pointer null, 4 099 lanes over several trips: the null side's buffer keeps its sentinel"""
    lane_case(4099, "plain", monkeypatch)
    pattern = [(False, False), (True, False), (False, True), (True, True), (True, False)]
    seen = checked(True)
    run_pair_lanes(rs.default_flop(), [1], 4099, edge_i32, I32_UTILS, rmplus=True, graph=graph, seed=183, iters=len(pattern), nulls=lambda it: pattern[it])
    assert seen


@pytest.mark.parametrize("case", ["prune", "sampled"])
def test_pruned_and_sampled_pairs_keep_the_unsplit_kernel(case, checked):
    """those walks diverge per lane at the root: forms & 8 == 0, and the pair still matches the numpy walk"""
    seen = checked(False)
    if case == "prune":
        run_pair_lanes(rs.default_flop(), [1], 4099, edge_i32, I32_UTILS, prune=True, seed=185, iters=2)
    else:
        run_pair_lanes(rs.default_flop(), [3], 1367, edge_i32, I32_UTILS, prune=True, opp="sample", seed=181, iters=2)
    assert seen


def test_split_on_equals_split_off(tmp_path):
    """RS_JIT_SPLIT=1 against RS_JIT_SPLIT=0, one fresh process per setting (tests/_pair_split_worker.py): tables and root utilities bit-equal, with per-traverser leaf
    rows that differ and either root-utility pointer null (the null side's buffer keeps its sentinel)"""
    outs = []
    for setting in ("1", "0"):
        env = dict(os.environ, RS_JIT_SPLIT=setting)
        path = str(tmp_path / ("split%s.npz" % setting))
        r = subprocess.run([sys.executable, os.path.join(HERE, "_pair_split_worker.py"), path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        outs.append(dict(np.load(path)))
    on, off = outs
    assert int(on["forms"]) & 4 and int(on["forms"]) & 8, on["forms"]
    assert int(off["forms"]) & 4 and not int(off["forms"]) & 8, off["forms"]
    assert sorted(on) == sorted(off) and len(on) > 20
    for k in sorted(on):
        if k != "forms":
            assert_same(on[k], off[k], k)
