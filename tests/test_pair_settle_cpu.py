"""CPU: paired lane solvers hold a traverser-0 sweep until traverser 1's comes (rs_iterate, include/rustsolver_amd.h).  Every other C entry point that takes a table, a solver
or a trainer must issue such a held sweep first -- through table_settle / solvers_settle_held / solver_settle_held (csrc/rs_table.cpp, rs_solver.cpp) -- or be one of the few
that only read metadata fixed at creation.  This scan keeps the next entry point from forgetting it.  And the pair kernel's generated source compiles without private memory."""
import glob
import os
import re
import shutil
import subprocess
import time

import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rustsolver_amd", "csrc")

SETTLES = ("table_settle(", "solvers_settle_held(", "solver_settle_held(")
# entry points that read what creation fixed (shapes, pointers, counters kept on the host) or touch neither table contents nor the stream's work
METADATA = {
    "rs_table_n_nodes", "rs_table_dtype", "rs_table_lane_pitch", "rs_table_cell_offset", "rs_table_bytes", "rs_table_deltas", "rs_table_device", "rs_table_node_desc",
    "rs_table_cells", "rs_table_tile_lanes", "rs_deal_trainer_table", "rs_deal_trainer_solver",
    "rs_solver_workspace_bytes", "rs_solver_exchange_bytes", "rs_solver_forms", "rs_solver_n_launches", "rs_solver_exchange_info",
    "rs_deal_trainer_iterations", "rs_deal_trainer_cards", "rs_deal_trainer_signs", "rs_deal_trainer_prune_flags", "rs_deal_trainer_clusters",
    "rs_deal_trainer_set_tick_br", "rs_deal_trainer_last_br", "rs_deal_trainer_br_launches", "rs_deal_trainer_br_bytes",
    "rs_solver_create", "rs_solver_create_deals",   # a new solver holds nothing yet
}
TYPES = re.compile(r"\b(rs_table|rs_solver|rs_deal_trainer)\s*\*")
DEF = re.compile(r"^(?:[A-Za-z_][\w\s\*]*?)\b(rs_\w+)\s*\(([^)]*)\)\s*\{", re.M)


def entry_points():
    """(name, body) of every extern "C" function definition of the library that takes one of the three handles"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(path).read()
        if 'extern "C"' not in src:
            continue
        for m in DEF.finditer(src):
            name, args = m.group(1), m.group(2)
            if not TYPES.search(args) or m.group(0).lstrip().startswith("static"):
                continue
            depth, i = 0, m.end() - 1
            while True:
                if src[i] == "{":
                    depth += 1
                elif src[i] == "}":
                    depth -= 1
                    if depth == 0:
                        break
                i += 1
            out.append((os.path.basename(path), name, src[m.end():i]))
    return out


def settles(body, bodies, seen=()):
    if any(s in body for s in SETTLES):
        return True
    # through another entry point or a static helper of the library that settles
    for callee in re.findall(r"\b(rs_\w+|\w+_impl|board_copy|node_kernel|\w+)\s*\(", body):
        if callee in bodies and callee not in seen and settles(bodies[callee], bodies, seen + (callee,)):
            return True
    return False


def all_bodies():
    bodies = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(path).read()
        for m in re.finditer(r"^(?:static\s+)?(?:[A-Za-z_][\w:<>\s\*&]*?)\b(\w+)\s*\([^;{)]*\)\s*\{", src, re.M):
            depth, i = 0, m.end() - 1
            while i < len(src):
                if src[i] == "{":
                    depth += 1
                elif src[i] == "}":
                    depth -= 1
                    if depth == 0:
                        break
                i += 1
            bodies.setdefault(m.group(1), src[m.end():i])
    return bodies


def test_every_entry_point_settles_held_sweeps():
    eps = entry_points()
    names = {n for _, n, _ in eps}
    assert {"rs_iterate", "rs_sync", "rs_d2h", "rs_discount", "rs_get_infosets", "rs_solver_destroy", "rs_table_destroy"} <= names, sorted(names)
    bodies = all_bodies()
    missing = [(f, n) for f, n, b in eps if n not in METADATA and not settles(b, bodies)]
    assert not missing, "entry points that neither settle a held pair sweep nor are metadata getters: %s" % missing
    stale = METADATA - names
    assert not stale, "metadata list names functions that no longer exist: %s" % sorted(stale)


def test_stream_and_sync_settle():
    """rs_sync and rs_stream hand the stream to the host: a held sweep must be on it first"""
    src = open(os.path.join(CSRC, "rs_table.cpp")).read()
    for fn in ("rs_sync", "rs_stream"):
        body = src[src.index(fn + "(rs_table *t)"):]
        body = body[:body.index("\n}\n")]
        assert "table_settle(" in body, fn


def test_pair_kernel_uses_no_scratch(monkeypatch):
    """the pair kernel of the headline tree (its carried state is every node's regrets) -- dumped by the compile check, compiled here with hipcc as hipRTC compiles it --
    must report `ScratchSize [bytes/lane]: 0` in every form the sweeps can take"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not L.load().rs_jit_available() or not os.path.exists(hipcc):
        pytest.skip("libhiprtc.so or hipcc not present")
    monkeypatch.setenv("RS_JIT_DUMP", "1")
    t0 = time.time() - 1.0
    _, tree = rs.build_game_tree(rs.default_flop())
    for dt, mode, opp in [(L.I32, L.UPD_CLAMP_I64, L.OPP_FULL), (L.I32, L.UPD_CLAMP_I64 | L.UPD_PRUNE, L.OPP_FULL), (L.F16, L.UPD_CLAMP_I64, L.OPP_FULL),
                          (L.I32, L.UPD_WRAP_I32, L.OPP_SAMPLE)]:
        assert rs.jit_check_pair(tree, dt, mode, opp) == 1
    fresh = [f for f in glob.glob("/tmp/rs_tree_kernel_*.hip") if os.path.getmtime(f) >= t0 and "rs_tree_pair_lanes" in open(f).read()]
    assert len(fresh) >= 4, fresh
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-include", "hip/hip_runtime.h", "-c", f, "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for f in fresh]
    for f, pr in zip(fresh, procs):
        out = pr.communicate()[0]
        assert pr.returncode == 0, out[-2000:]
        sizes = [l.split("ScratchSize [bytes/lane]:")[1].split()[0] for l in out.splitlines() if "ScratchSize [bytes/lane]:" in l]
        assert sizes and all(x == "0" for x in sizes), (f, sizes)
