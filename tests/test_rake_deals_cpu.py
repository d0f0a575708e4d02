"""CPU: rake on the deal path (rs_solver_create_deals_raked, rs_jit_check_tree_deals_raked) as far as no device is needed.

  * the helper tests/np_rake_deals.py, which tests/test_gpu_rake_deals.py measures the device with, is pinned: without rake its retyped tree and utility rows give
    oracle/np_walk.iterate_deals the tables the original tree gives it with sign leaves (i32 clamp and f32), bit for bit;
  * the raked forms of every generated deal kernel compile, as many as unraked; a rake that is none goes through the library's own check that it changes no source;
  * the raked, sampled, pruned kernels of a two-round tree use no scratch (three reach-down kernels, two walks with three-valued leaves), compiled as hipRTC compiles them;
  * the refusals that need no device.
Rake (0.3, cap), the cap asserted to cap some terminals of the tree and not others.
"""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import np_rake_deals as nrd
import rustsolver_amd as rs
from oracle import np_walk as npw
from rustsolver_amd import _lib as L

F32 = np.float32
RIVER_RAKE = (0.3, 60.0)      # the default river tree's pots are 35 to 1035: those above 200 are capped
TWO_ROUND_RAKE = (0.3, 30.0)  # pots above 100 are capped
TWO_ROUND = dict(n_board_cards=4, bet_sizes=((0.5,), (1.0,)), raise_sizes=((3.0,), (3.0,)))   # the tree of test_generated_deal_kernels_use_no_scratch


def need_jit():
    if not L.load().rs_jit_available():
        pytest.skip("libhiprtc.so not present")


def both_sides_of_the_cap(tree, rake):
    capped, free = nrd.capped_terminals(tree, rake)
    assert capped and free, (rake, len(capped), len(free))


def signs(rng, n):
    """-1, 0 and +1, each on at least an eighth of the deals"""
    s = rng.integers(-1, 2, size=n).astype(F32)
    for v in (-1, 0, 1):
        assert (s == v).sum() * 8 >= n
    return s


@pytest.mark.parametrize("dtype", ["i32", "f32"])
def test_helper_without_rake_is_the_sign_walk(dtype):
    rng = np.random.Generator(np.random.PCG64(31))
    _, tree = rs.build_game_tree(rs.default_flop())
    nodes, renodes = npw.tree_from_records(tree.nodes), nrd.retyped_nodes(tree)
    assert all(d["ttype"] == "SHOWDOWN" for d in renodes if d["kind"] == npw.TERMINAL)
    n, sizes = 257, (7, 5)
    sign = signs(rng, n)
    cidx = {(0, p): rng.integers(0, sizes[p], size=n).astype(np.uint32) for p in (0, 1)}
    tabs = [{}, {}]
    for nd in tree.action_nodes():
        shape = (nd.n_children, sizes[nd.player])
        if dtype == "i32":
            R, S = rng.integers(-10**6, 10**6, size=shape).astype(np.int32), rng.integers(0, 10**6, size=shape).astype(np.int32)
        else:
            R, S = rng.uniform(-1e3, 1e3, size=shape).astype(F32), rng.uniform(0, 1e3, size=shape).astype(F32)
        for tab in tabs:
            tab[nd.index] = (R.copy(), S.copy())
    sign_leaves = {i: ("sign", sign) for i, d in enumerate(nodes) if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"}
    for k, player in enumerate((0, 1, 0, 1)):
        kw = dict(scale=100.0, mode="clamp", dtype=dtype, opp="sample", seed=1000 + k)
        want = npw.iterate_deals(nodes, tabs[0], sign_leaves, cidx, player, **kw)
        got = npw.iterate_deals(renodes, tabs[1], nrd.util_leaves(tree, None, sign, player), cidx, player, **kw)
        assert got.tobytes() == want.tobytes(), (dtype, k)
    for idx in tabs[0]:
        for a, b in zip(tabs[0][idx], tabs[1][idx]):
            assert a.tobytes() == b.tobytes(), (dtype, idx)
    # ... and the rake reaches the rows: other numbers at a capped and at an uncapped terminal
    capped, free = nrd.capped_terminals(tree, RIVER_RAKE)
    plain, raked = nrd.util_rows(tree, None, sign, 0), nrd.util_rows(tree, RIVER_RAKE, sign, 0)
    assert any((plain[i] != raked[i]).any() for i in capped) and any((plain[i] != raked[i]).any() for i in free)


def test_raked_river_forms_compile():
    need_jit()
    _, tree = rs.build_game_tree(rs.default_flop())
    both_sides_of_the_cap(tree, RIVER_RAKE)
    for mode in (rs.UPD_CLAMP_I64, rs.UPD_CLAMP_I64 | rs.UPD_PRUNE):
        plain = rs.jit_check_tree_deals(tree, mode, rs.OPP_SAMPLE)
        assert rs.jit_check_tree_deals(tree, mode, rs.OPP_SAMPLE, rake=RIVER_RAKE) == plain > 0


def test_raked_two_round_forms_compile():
    need_jit()
    _, tree = rs.build_game_tree(rs.Options(**TWO_ROUND))
    both_sides_of_the_cap(tree, TWO_ROUND_RAKE)
    plain = rs.jit_check_tree_deals(tree, rs.UPD_WRAP_I32, rs.OPP_FULL)
    assert rs.jit_check_tree_deals(tree, rs.UPD_WRAP_I32, rs.OPP_FULL, rake=TWO_ROUND_RAKE) == plain > 0


def test_a_rake_that_is_none_changes_no_source():
    """the library compares the sources itself (RS_ERR_MISMATCH): NULL, rate 0 and cap 0 must give the unraked emission of the same inputs"""
    need_jit()
    _, tree = rs.build_game_tree(rs.default_flop())
    plain = rs.jit_check_tree_deals(tree, rs.UPD_CLAMP_I64, rs.OPP_SAMPLE)
    for rake in ((0.0, 0.0), (0.0, 5.0), (0.3, 0.0)):
        assert rs.jit_check_tree_deals(tree, rs.UPD_CLAMP_I64, rs.OPP_SAMPLE, rake=rake) == plain
    n = C.c_int()
    L.check(L.load().rs_jit_check_tree_deals_raked(tree._h, rs.UPD_CLAMP_I64, rs.OPP_SAMPLE, None, C.byref(n)))
    assert n.value == plain


def test_raked_deal_kernels_use_no_scratch(monkeypatch):
    """the selects of sign_to_util3 take three wave-uniform numbers: nothing is indexed by a runtime value, so no kernel may spill to private memory"""
    need_jit()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    monkeypatch.setenv("RS_JIT_DUMP", "1")
    t0 = time.time() - 1.0
    _, tree = rs.build_game_tree(rs.Options(**TWO_ROUND))
    assert rs.jit_check_tree_deals(tree, rs.UPD_CLAMP_I64 | rs.UPD_PRUNE, rs.OPP_SAMPLE, rake=TWO_ROUND_RAKE) > 8
    fresh = {}
    for f in glob.glob("/tmp/rs_tree_kernel_*.hip"):
        if os.path.getmtime(f) >= t0:
            text = open(f).read()
            if "void sign_to_util3(" in text:   # a raked walk's kernel: the definition follows its prelude
                fresh[f] = text
    down = sorted(f for f, text in fresh.items() if "_deals_down_sampled" in text and re.search(r"hand_pick<\d+>\(", text))
    walks = sorted(f for f, text in fresh.items() if f not in down and re.search(r"\n\s+sign_to_util3\(", text))
    assert len(down) >= 3 and len(walks) >= 2, (len(fresh), len(down), len(walks))
    picked = down[:3] + walks[:2]
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-include", "hip/hip_runtime.h", "-c", f, "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for f in picked]
    for f, pr in zip(picked, procs):
        out = pr.communicate()[0]
        assert pr.returncode == 0, out[-2000:]
        sizes = [l.split("ScratchSize [bytes/lane]:")[1].split()[0] for l in out.splitlines() if "ScratchSize [bytes/lane]:" in l]
        assert sizes and all(x == "0" for x in sizes), (f, sizes)


@pytest.mark.parametrize("rake", [(-0.1, 5.0), (1.5, 5.0), (float("nan"), 5.0), (float("inf"), 5.0), (0.3, -1.0), (0.3, float("nan")), (0.3, 5.0, (1, 0)), (0.3, 5.0, (0, 7))])
def test_refusals_without_a_device(rake):
    _, tree = rs.build_game_tree(rs.default_flop())
    with pytest.raises(rs.RsError) as e:
        rs.jit_check_tree_deals(tree, rs.UPD_CLAMP_I64, rs.OPP_SAMPLE, rake=rake)
    assert e.value.code == L.ERR_INVALID
