"""CPU (-m "not gpu"): the split form of the pair kernel (rs_jit.cpp).  The emitter cuts a chance-free subtree below its root into two parts that two threads of one
workgroup walk for the same lanes; it does so only where the root has at least two action children and the larger part keeps at most two thirds of the carried cells.
The form exists to run at two waves per SIMD: 512 registers per SIMD lane / 2 waves = 256 VGPRs + AGPRs at most, and no scratch."""
import glob
import os
import re
import shutil
import subprocess

import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L

needs_rtc = pytest.mark.skipif(not L.load().rs_jit_available(), reason="libhiprtc.so cannot be loaded here")


def dumped_pair_sources(tree, monkeypatch, dtype=L.I32, mode=L.UPD_CLAMP_I64, opp=L.OPP_FULL):
    """[(path, text)] of the pair kernels rs_jit_check_pair generates (and compiles) for `tree`"""
    monkeypatch.setenv("RS_JIT_DUMP", "1")
    before = {f: os.stat(f).st_mtime_ns for f in glob.glob("/tmp/rs_tree_kernel_*.hip")}
    assert rs.jit_check_pair(tree, dtype, mode, opp) == 1
    out = []
    for f in glob.glob("/tmp/rs_tree_kernel_*.hip"):
        if before.get(f) != os.stat(f).st_mtime_ns:
            text = open(f).read()
            if "void rs_tree_pair_lanes" in text:
                out.append((f, text))
    assert out, "no pair kernel was dumped"
    return out


def entry_of(text):
    return re.search(r"void (rs_tree_pair_lanes\w*)\(", text).group(1)


def one_child_tree():
    """player 0 {fold, continue -> player 1's node}, player 1 {fold, call}: the root has ONE action child"""
    nodes = [L.TreeNode() for _ in range(6)]

    def fill(i, kind, parent, children=(), **kw):
        nd = nodes[i]
        nd.kind, nd.parent, nd.n_children = kind, parent, len(children)
        for k, c in enumerate(children):
            nd.children[k] = c
        for key, v in kw.items():
            setattr(nd, key, v)
    fill(0, rs.NODE_PRIVATE_CHANCE, -1, (1,))
    fill(1, rs.NODE_ACTION, 0, (2, 3), index=0, player=0, round_idx=0)
    fill(2, rs.NODE_TERMINAL, 1, value=3, ttype=rs.TERM_UNCONTESTED, last_to_act=0, round=0)
    fill(3, rs.NODE_ACTION, 1, (4, 5), index=1, player=1, round_idx=0)
    fill(4, rs.NODE_TERMINAL, 3, value=6, ttype=rs.TERM_UNCONTESTED, last_to_act=1, round=0)
    fill(5, rs.NODE_TERMINAL, 3, value=6, ttype=rs.TERM_SHOWDOWN, last_to_act=1, round=0)
    return rs.tree_from_nodes(nodes)


@needs_rtc
def test_headline_tree_splits_evenly(monkeypatch):
    """river tree: {action 0} against {root, actions 1, 2}: 7 action nodes and 19 regret cells each"""
    monkeypatch.delenv("RS_JIT_SPLIT", raising=False)
    _, tree = rs.build_game_tree(rs.default_flop())
    (_, text), = dumped_pair_sources(tree, monkeypatch)
    assert entry_of(text) == "rs_tree_pair_lanes_l2_sp"
    m = re.search(r"// split form: part A (\d+) nodes, (\d+) cells; part B (\d+) nodes, (\d+) cells", text)
    assert m and [int(x) for x in m.groups()] == [7, 19, 7, 19]
    body = text[text.index("void rs_tree_pair_lanes"):]
    assert body.count("// part A\n") == 1 and body.count("// part B\n") == 1
    a, b = body[body.index("// part A\n"):body.index("// part B\n")], body[body.index("// part B\n"):]
    assert "R::load(" in a and "R::store(" in a and "lanes_visit<" in a   # the cut really holds part A's walk
    assert "J.reg[0]" not in a and "J.ssm[0]" not in a, "part A touches a root row"
    assert "J.reg[0]" in b and "J.ssm[0]" in b
    assert a.count("__syncthreads()") == b.count("__syncthreads()") == 3   # every thread of the workgroup meets every barrier of a trip


@needs_rtc
def test_switch_and_unsplittable_shapes_keep_the_pair_form(monkeypatch):
    """RS_JIT_SPLIT=0, pruning and sampled opponents keep the existing entry on the headline tree; so does a tree whose root has one action child"""
    _, tree = rs.build_game_tree(rs.default_flop())
    monkeypatch.setenv("RS_JIT_SPLIT", "0")
    (_, text), = dumped_pair_sources(tree, monkeypatch)
    assert entry_of(text) == "rs_tree_pair_lanes_l2"
    monkeypatch.delenv("RS_JIT_SPLIT")
    (_, text), = dumped_pair_sources(tree, monkeypatch, mode=L.UPD_CLAMP_I64 | L.UPD_PRUNE)
    assert entry_of(text) == "rs_tree_pair_lanes_prune_l2"
    (_, text), = dumped_pair_sources(tree, monkeypatch, mode=L.UPD_WRAP_I32, opp=L.OPP_SAMPLE)
    assert entry_of(text) == "rs_tree_pair_lanes_sampled_l2"
    (_, text), = dumped_pair_sources(one_child_tree(), monkeypatch)
    assert entry_of(text) == "rs_tree_pair_lanes_l2" and "XS[" not in text


@needs_rtc
def test_split_kernel_fits_two_waves_per_simd_without_scratch(monkeypatch):
    """the dumped split kernels of the headline tree -- i32 clamp, i32 wrap, f32, f16 -- compiled with hipcc as hipRTC compiles them: 0 bytes of scratch and
    VGPRs + AGPRs <= 256, i.e. two waves per SIMD"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    monkeypatch.delenv("RS_JIT_SPLIT", raising=False)
    _, tree = rs.build_game_tree(rs.default_flop())
    files = []
    for dt, mode in [(L.I32, L.UPD_CLAMP_I64), (L.I32, L.UPD_WRAP_I32), (L.F32, L.UPD_CLAMP_I64), (L.F16, L.UPD_CLAMP_I64)]:
        (f, text), = dumped_pair_sources(tree, monkeypatch, dtype=dt, mode=mode)
        assert entry_of(text).endswith("_sp")
        files.append(f)
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-include", "hip/hip_runtime.h", "-c", f, "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for f in files]
    for f, pr in zip(files, procs):
        out = pr.communicate()[0]
        assert pr.returncode == 0, out[-2000:]

        def field(name):
            vals = [int(l.split(name)[1].split()[0]) for l in out.splitlines() if name in l]
            assert len(vals) == 1, (f, name, vals)
            return vals[0]
        vgprs, agprs, scratch, occupancy = field(" VGPRs:"), field(" AGPRs:"), field("ScratchSize [bytes/lane]:"), field("Occupancy [waves/SIMD]:")
        print(os.path.basename(f), "VGPRs", vgprs, "AGPRs", agprs, "scratch", scratch, "waves/SIMD", occupancy)
        assert scratch == 0, (f, scratch)
        assert vgprs + agprs <= 256, (f, vgprs, agprs)
        assert occupancy >= 2, (f, occupancy)
