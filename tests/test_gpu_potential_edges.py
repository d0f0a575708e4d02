"""GPU (-m gpu): rs_pa_predict and rs_pa_fit at the edges test_gpu_potential.py does not reach -- neighbour ranks above 511 (4099 next buckets, and RS_PA_MAX_NEXT = 8192
once), the second trips of the grid-stride loops of k_pa_assign and k_pa_sums, rs_pa_fit with a malformed row, means that are all zero or hold -0.0 and subnormals,
totals that overflow to +inf, n_draws of 1, 2 and 45 -- bit for bit against the numpy restatement tests/np_potential.py.  No tolerance anywhere.  The inputs and what the
restatement makes of them come from tests/potential_edge_inputs.py, where tests/test_potential_cpu.py holds the host distance to them.  Every predict goes into outputs
filled with a sentinel, so a datum that was not written shows.  Every test prints its figures on a line that starts with POTENTIAL (pytest -s)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd.solver import DeviceBuffer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_potential as npp  # noqa: E402
import potential_edge_inputs as pe  # noqa: E402
from test_gpu_potential import SENTINEL, bits, device_rows, make_means, report  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


@pytest.fixture(scope="module")
def table():
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    return rs.create_infosets(n_actions, tree, [4], [1])


def sentinel_outputs(table, n):
    lib = L.load()
    dc, dm = DeviceBuffer(table, n * 4), DeviceBuffer(table, n * 4)
    for b in (dc, dm):
        L.check(lib.rs_dmemset(table._h, b.ptr, 0xCD, b.nbytes))
    return dc, dm


def raw_predict(table, km, dr, means, sel=None):
    """rs_pa_predict into sentinel-filled outputs -> (return code, clusters, the bits of the distances)"""
    m = np.ascontiguousarray(means, dtype=F32)
    ds = DeviceBuffer.from_numpy(table, np.ascontiguousarray(sel, dtype=np.uint32)) if sel is not None else None
    n = len(sel) if sel is not None else dr.rows
    dc, dm = sentinel_outputs(table, n)
    rc = L.load().rs_pa_predict(table._h, km._h, dr.ptr, ds.ptr if ds else None, n, dr.n_draws, m.ctypes.data, len(m), dc.ptr, dm.ptr)
    got = dc.download(np.uint32, n), dm.download(np.uint32, n)
    for b in (dc, dm, ds):
        if b is not None:
            b.free()
    return (rc,) + got


def differing(table, km, dr, means, want, sel=None):
    """all the means at once against the restatement's choice, then every mean alone, so that the distance of EVERY (row, mean) pair is compared and not only the
    smallest of a row -> (data whose cluster or distance differs, (row, mean) pairs whose distance differs)"""
    want = want if sel is None else want[sel]
    want_c, want_d = pe.choice_of(want)
    rc, got_c, got_d = raw_predict(table, km, dr, means, sel)
    assert rc == L.OK
    chosen = int(((got_c != want_c) | (got_d != bits(want_d))).sum())
    pairs = 0
    for k in range(len(means)):
        rc, one_c, one_d = raw_predict(table, km, dr, means[k:k + 1], sel)
        assert rc == L.OK and not one_c.any()
        pairs += int((one_d != bits(want[:, k])).sum())
    return chosen, pairs, got_c


# ---- 1. ranks above 511 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["ties", "duplicates"])
def high(request, table):
    """4099 next buckets under one ground matrix: the case, its rows on the device and the metric (a stable sort of 4099 rows on the host), made once"""
    t0 = time.perf_counter()
    c = pe.high_rank_case(4099, request.param)
    t1 = time.perf_counter()
    dr = device_rows(table, c["rows"], c["n_draws"])
    km = ab.PotentialKmeans(table, dr, c["ground"])
    report("fixture 4099 next buckets, %s" % request.param, restatement_s=t1 - t0, metric_s=time.perf_counter() - t1)
    yield request.param, c, dr, km
    dr.buffer.free()


@pytest.mark.parametrize("use_sel", [False, True], ids=["rows", "sel"])
def test_ranks_above_511_equal_the_restatement(table, high, use_sel):
    which, c, dr, km = high
    t0 = time.perf_counter()
    # the premise, from the restatement's own trace: in some pair two entries take at r1 < r2 with r1 >= 512 and (r1 & 511) > (r2 & 511), so that only bits 9 and up of
    # the lowest-rank search put r1 first; and a take stands in the last, ragged round of 64 ranks
    assert c["pairs_ordered_by_a_high_bit"] >= 1 and c["highest_take_rank"] > 4032
    sel = c["sel"] if use_sel else None
    chosen, pairs, got_c = differing(table, km, dr, c["means"], c["want"], sel)
    report("predict 4099 next buckets, %s, sel %s" % (which, use_sel), data=len(got_c), means=len(c["means"]), data_that_differ=chosen, pairs_that_differ=pairs,
           pairs_ordered_by_a_high_bit=c["pairs_ordered_by_a_high_bit"], highest_take_rank=c["highest_take_rank"],
           second_of_two_equal_means_chosen=int((got_c == 1).sum()), wall_s=time.perf_counter() - t0)
    assert chosen == 0 and pairs == 0 and not (got_c == 1).any()


def test_the_most_next_buckets_there_can_be(table):
    """RS_PA_MAX_NEXT = 8192: 33 KB of dynamic LDS, ids up to 8191 in the 16-bit `order`, a take at rank 8191.  The cost is the host's: the 256 MB ground matrix, its
    argsort and the metric's stable sort"""
    t0 = time.perf_counter()
    c = pe.high_rank_case(8192, "ties")
    t1 = time.perf_counter()
    assert c["pairs_ordered_by_a_high_bit"] >= 1 and c["highest_take_rank"] == 8191 and int((c["rows"] >> 8).max()) > 4096
    dr = device_rows(table, c["rows"], c["n_draws"])
    km = ab.PotentialKmeans(table, dr, c["ground"])
    t2 = time.perf_counter()
    chosen, pairs, got_c = differing(table, km, dr, c["means"], c["want"])
    dr.buffer.free()
    del km
    report("predict 8192 next buckets", data=len(got_c), means=len(c["means"]), data_that_differ=chosen, pairs_that_differ=pairs, highest_take_rank=c["highest_take_rank"],
           restatement_s=t1 - t0, metric_s=t2 - t1, device_s=time.perf_counter() - t2, wall_s=time.perf_counter() - t0)
    assert chosen == 0 and pairs == 0 and len(got_c) == 8


# ---- 2. past the grid caps ------------------------------------------------------------------------------------------------------------------------------------------------
def test_predict_past_the_grid_cap_of_the_assignment(table):
    t0 = time.perf_counter()
    c = pe.long_predict_case()
    n = len(c["rows"])
    assert n == (1 << 16) + 3 and c["means"].shape == (2, 2) and len(set(c["want_c"][-3:].tolist())) == 2      # the second trip's rows do not all go one way
    dr = device_rows(table, c["rows"], c["n_draws"])
    km = ab.PotentialKmeans(table, dr, c["ground"])
    rc, got_c, got_d = raw_predict(table, km, dr, c["means"])
    dr.buffer.free()
    differ = int(((got_c != c["want_c"]) | (got_d != bits(c["want_d"]))).sum())
    report("predict 65 536 + 3 rows", rows_compared=n, differ=differ, left_unwritten=int((got_c == SENTINEL).sum()), per_cluster=np.bincount(c["want_c"]).tolist(),
           wall_s=time.perf_counter() - t0)
    assert rc == L.OK and differ == 0


def test_fit_past_the_grid_cap_of_the_sums(table):
    t0 = time.perf_counter()
    c = pe.long_fit_case()
    t1 = time.perf_counter()
    n = len(c["rows"])
    per_cluster = np.bincount(c["want_c"], minlength=2)
    assert n == (1 << 18) + 5 and len(c["want_changed"]) == 3 and c["want_changed"][0] == n and c["want_changed"][2] > 0 and per_cluster.min() > 0
    assert len(set(c["want_c"][-5:].tolist())) == 2      # the five data of k_pa_sums' second trip are not all in one cluster: both means would miss them
    dr = device_rows(table, c["rows"], c["n_draws"])
    got_c, got_m, got_d, got_ch = ab.PotentialKmeans(table, dr, c["ground"]).fit(c["means"], iterations=3)
    dr.buffer.free()
    report("fit 262 144 + 5 rows, 2 means, 3 iterations", changed=got_ch.tolist(), per_cluster=per_cluster.tolist(), clusters_differ=int((got_c != c["want_c"]).sum()),
           means_differ=int((bits(got_m) != bits(c["want_m"])).sum()), distances_differ=int((bits(got_d) != bits(c["want_d"])).sum()), restatement_s=t1 - t0,
           wall_s=time.perf_counter() - t0)
    assert got_ch.tolist() == c["want_changed"].tolist() and (got_c == c["want_c"]).all()
    assert (bits(got_m) == bits(c["want_m"])).all() and (bits(got_d) == bits(c["want_d"])).all()


# ---- 3. rs_pa_fit with a row that is not well-formed --------------------------------------------------------------------------------------------------------------------
def test_fit_leaves_a_malformed_row_in_no_cluster_and_fits_the_others(table):
    t0 = time.perf_counter()
    rng = np.random.Generator(np.random.PCG64(7033))
    n_next, n_draws, iterations = 65, 47, 3
    g = npp.tie_ground(n_next)
    rows = npp.random_rows(rng, 70, n_next, n_draws)
    means = make_means(rng, rows, 5, n_next, n_draws)
    ok = np.arange(70) != 33
    want_c, want_m, want_d, want_ch = npp.fit(rows[ok], means, g, n_draws, iterations)
    assert len(want_ch) >= 2 and want_ch[0] == 69 and want_ch[1] > 0
    lib = L.load()
    for name, bad in (("not ascending", npp.pack_row([9, 4], [20, 27])), ("a bucket past n_next", npp.pack_row([4, 65], [20, 27])),
                      ("a count of 0 ahead of a used word", np.concatenate([[4 << 8 | 20, 6 << 8, 9 << 8 | 27], np.zeros(45)]).astype(np.uint32)),
                      ("counts short of n_draws", npp.pack_row([4, 9], [20, 26])), ("no entry", np.zeros(48, dtype=np.uint32))):
        x = rows.copy()
        x[33] = bad
        dr = device_rows(table, x, n_draws)
        km = ab.PotentialKmeans(table, dr, g)
        dc, dm = sentinel_outputs(table, 70)
        m = means.copy()
        changed, ran = np.full(iterations, SENTINEL, dtype=np.uint32), C.c_int(-1)
        rc = lib.rs_pa_fit(table._h, km._h, dr.ptr, None, 70, n_draws, m.ctypes.data, 5, iterations, dc.ptr, dm.ptr, changed.ctypes.data, C.byref(ran))
        got_c, got_d = dc.download(np.uint32, 70), dm.download(np.uint32, 70)
        for b in (dc, dm, dr.buffer):
            b.free()
        assert rc == L.ERR_INVALID, name
        assert changed[0] == 70 and ran.value == len(want_ch) and changed[1:ran.value].tolist() == want_ch[1:].tolist(), (name, changed, ran.value, want_ch)
        assert got_c[33] == npp.NO_CLUSTER and got_d[33] == SENTINEL, name
        assert (got_c[ok] == want_c).all() and (got_d[ok] == bits(want_d)).all() and (bits(m) == bits(want_m)).all(), name
    report("fit with a malformed row, five kinds", changed_of_the_others=want_ch.tolist(), wall_s=time.perf_counter() - t0)


# ---- 4. values ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pe.VALUE_CASES)
def test_predict_at_value_edges_equals_the_restatement(table, name):
    t0 = time.perf_counter()
    c = pe.value_case(name)
    pe.value_premises(name, c)                       # what the case is there for, from the restatement alone
    dr = device_rows(table, c["rows"], c["n_draws"])
    km = ab.PotentialKmeans(table, dr, c["ground"])
    chosen, pairs, got_c = differing(table, km, dr, c["means"], c["want"])
    dr.buffer.free()
    tiny = np.finfo(F32).tiny
    report("predict, %s" % name, data=len(got_c), n_draws=c["n_draws"], data_that_differ=chosen, pairs_that_differ=pairs, per_mean=np.bincount(pe.choice_of(c["want"])[0], minlength=len(c["means"])).tolist(),
           infinite_distances=int(np.isinf(c["want"]).sum()), subnormal_distances=int(((c["want"] > 0) & (c["want"] < tiny)).sum()), wall_s=time.perf_counter() - t0)
    assert chosen == 0 and pairs == 0
