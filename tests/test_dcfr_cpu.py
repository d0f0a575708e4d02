"""CPU (-m "not gpu"): Discounted CFR's host side -- the symbols, the three factors against the float64 formula, refused arguments, and the discounted variant of the
headline tree's lane kernels: it compiles for gfx950 without scratch, and asking for it leaves the plain kernels' source where it was."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L

F32 = np.float32
SYMBOLS = ["rs_dcfr_params_default", "rs_dcfr_factors", "rs_discount_dcfr", "rs_train_dcfr", "rs_solver_dcfr_fused", "rs_deal_trainer_set_dcfr"]
INF = float("inf")


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = C.CDLL(L.SO_PATH)
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n in L.SYMBOLS, n
    assert lib.rs_abi_version() == 6
    p = rs.dcfr_params()
    assert (p.alpha, p.beta, p.gamma, p.interval, p.cap, p.t0, p.fused, p.reserved) == (1.5, 0.0, 2.0, 1, 2**64 - 1, 0, L.FORM_DEFAULT, 0)
    assert C.sizeof(L.DcfrParams) == 56


def formula(alpha, beta, gamma, p):
    """float32(float64 formula); an infinite exponent is its limit, for every p"""
    p = np.float64(p)

    def ratio(e):
        if np.isinf(e):
            return np.float64(1.0 if e > 0 else 0.0)
        x = np.power(p, np.float64(e))
        return x / (x + 1.0)
    return np.array([ratio(alpha), ratio(beta), np.power(p / (p + 1.0), np.float64(gamma))], dtype=np.float64).astype(F32)


def ulps_apart(a, b):
    a, b = np.asarray(a, dtype=F32).view(np.int32).astype(np.int64), np.asarray(b, dtype=F32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@pytest.mark.parametrize("abg", [(1.5, 0.0, 2.0), (1.0, 1.0, 1.0), (INF, -INF, 0.0)])
@pytest.mark.parametrize("p", [1, 2, 3, 1000, 2**40])
def test_factors_against_the_float64_formula(abg, p):
    """at most one f32 ulp apart: libm's and numpy's pow may differ in the last bit of the double that is then rounded"""
    got = rs.dcfr_factors(*abg, p)
    want = formula(*abg, p)
    print("dcfr_factors", abg, p, got, want)
    assert got.dtype == F32 and (ulps_apart(got, want) <= 1).all(), (got, want)
    assert ((got >= 0) & (got <= 1)).all()


def test_factors_are_exact_at_the_limits():
    for p in (1, 2, 1000, 2**40):
        got = rs.dcfr_factors(INF, -INF, 0.0, p)
        assert got.tolist() == [1.0, 0.0, 1.0], (p, got)
    assert rs.dcfr_factors(1.0, 1.0, 1.0, 1).tolist() == [0.5, 0.5, 0.5]
    assert rs.dcfr_factors(1.5, 0.0, 2.0, 1).tolist() == [0.5, 0.5, 0.25]
    assert rs.dcfr_factors(1.5, 0.0, 2.0, 7)[1] == 0.5          # beta = 0: negative regrets halve at every tick
    assert rs.dcfr_factors(400.0, -400.0, 2.0, 2**40).tolist()[:2] == [1.0, 0.0]   # p^alpha overflows double: the limit, not NaN
    lin = rs.dcfr_factors(1.0, 1.0, 1.0, 3)
    assert lin[0] == lin[1] == lin[2] == F32(0.75)               # Linear CFR: one factor, rs_discount's p / (p + 1)


def test_bad_arguments_are_refused():
    lib = L.load()
    out = (C.c_float * 3)()
    assert lib.rs_dcfr_factors(1.5, 0.0, 2.0, 0, out) == L.ERR_INVALID                  # p = 0
    assert lib.rs_dcfr_factors(1.5, 0.0, 2.0, 1, None) == L.ERR_INVALID
    assert lib.rs_dcfr_factors(float("nan"), 0.0, 2.0, 1, out) == L.ERR_INVALID
    assert lib.rs_dcfr_factors(1.5, 0.0, INF, 1, out) == L.ERR_INVALID
    assert lib.rs_dcfr_params_default(None) == L.ERR_INVALID
    assert lib.rs_discount_dcfr(None, 0.5, 0.5, 0.25) == L.ERR_INVALID
    p = rs.dcfr_params()
    assert lib.rs_train_dcfr(None, 1, C.byref(p)) == L.ERR_INVALID
    assert lib.rs_solver_dcfr_fused(None) == L.ERR_INVALID
    assert lib.rs_deal_trainer_set_dcfr(None, C.byref(p)) == L.ERR_INVALID
    with pytest.raises(rs.RsError) as e:
        rs.dcfr_factors(1.5, 0.0, 2.0, 0)
    assert e.value.code == L.ERR_INVALID and "p must be > 0" in str(e.value)


def test_interval_zero_and_null_params_are_refused_before_the_solver_is_touched():
    """rs_train_dcfr checks its arguments in front of everything else: a (never dereferenced) non-null solver pointer is enough to reach the checks without a GPU"""
    lib = L.load()
    fake = C.create_string_buffer(8)   # never read: both calls fail on `params`
    assert lib.rs_train_dcfr(C.cast(fake, C.c_void_p), 1, None) == L.ERR_INVALID
    assert "NULL" in lib.rs_last_error().decode()
    assert lib.rs_train_dcfr(C.cast(fake, C.c_void_p), 1, C.byref(rs.dcfr_params(interval=0))) == L.ERR_INVALID
    assert "interval" in lib.rs_last_error().decode()
    bad = rs.dcfr_params()
    bad.fused = 7
    assert lib.rs_train_dcfr(C.cast(fake, C.c_void_p), 1, C.byref(bad)) == L.ERR_INVALID
    assert lib.rs_train_dcfr(C.cast(fake, C.c_void_p), 1, C.byref(rs.dcfr_params(gamma=INF))) == L.ERR_INVALID


CASES = [("i32 clamp", L.I32, L.UPD_CLAMP_I64), ("i32 wrap", L.I32, L.UPD_WRAP_I32), ("f32", L.F32, L.UPD_CLAMP_I64), ("f16", L.F16, L.UPD_CLAMP_I64)]


def test_discounted_variant_compiles_without_scratch_and_leaves_the_plain_source_alone(monkeypatch):
    """the 14-node river tree: the plain lane kernels' sources are dumped first, then the discounted variants are requested (the check itself fails if the plain source
    generated after the variant differs from the one generated before it), then the plain kernels again: the same files with the same bytes.  The variants -- compiled here
    with hipcc as hipRTC compiles them -- report `ScratchSize [bytes/lane]: 0`, for i32 clamp, i32 wrap, f32 and f16."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not L.load().rs_jit_available() or not os.path.exists(hipcc):
        pytest.skip("libhiprtc.so or hipcc not present")
    monkeypatch.setenv("RS_JIT_DUMP", "1")
    _, tree = rs.build_game_tree(rs.default_flop())
    assert tree.n_action_nodes == 14
    variants, known = [], set()
    for name, dt, mode in CASES:
        t0 = time.time() - 1.0
        assert rs.jit_check_tree(tree, dt, mode) == 2
        plain = {f: open(f).read() for f in glob.glob("/tmp/rs_tree_kernel_*.hip") if os.path.getmtime(f) >= t0 and f not in known and "_lanes(" in open(f).read()}
        assert len(plain) == 2 and not any("dcfr" in s for s in plain.values()), (name, sorted(plain))
        assert rs.jit_check_dcfr(tree, dt, mode) == 2
        fresh = [f for f in glob.glob("/tmp/rs_tree_kernel_*.hip") if os.path.getmtime(f) >= t0 and f not in known and "_lanes_dcfr(" in open(f).read()]
        assert len(fresh) == 2, (name, fresh)
        variants += [(name, f) for f in fresh]
        known |= set(plain) | set(fresh)
        for f in plain:               # the dumps are named by a hash of the source: the plain kernels generated NOW must bring the same files back, with the same bytes
            os.unlink(f)
        assert rs.jit_check_tree(tree, dt, mode) == 2
        for f, s in plain.items():
            assert os.path.exists(f) and open(f).read() == s, (name, f)
        for f in fresh:               # the variant is the plain kernel plus the discount: without it, the plain text
            v = open(f).read()
            assert "dcfr_regrets<" in v and "dcfr_sums<" in v and "DcfrSide dc[2];" in v
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-include", "hip/hip_runtime.h", "-c", f, "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for _, f in variants]
    for (name, f), pr in zip(variants, procs):
        out = pr.communicate()[0]
        assert pr.returncode == 0, out[-2000:]
        sizes = [l.split("ScratchSize [bytes/lane]:")[1].split()[0] for l in out.splitlines() if "ScratchSize [bytes/lane]:" in l]
        vgprs = [l.split("VGPRs:")[1].split()[0] for l in out.splitlines() if " VGPRs:" in l]
        print("dcfr variant", name, os.path.basename(f), "VGPRs", vgprs, "scratch", sizes)
        assert sizes and all(x == "0" for x in sizes), (name, f, sizes)
