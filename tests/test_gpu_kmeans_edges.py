"""GPU (-m gpu): the k-means training loops (rs_kmeans.hip: init_s, reassign, fit_regular, fit_growbatch; predict and update_min_dists at the long size) at the width,
cluster-count, list-length, size and value edges of tests/kmeans_edge_inputs.py, against the oracle (oracle/kmeans_fit.c), bit for bit: clusters, centres, bounds and
inertia / stats, every element, no tolerance.  tests/test_kmeans_cpu.py shows with the oracle alone that each case reaches its edge.  Inputs: finite, non-negative bins
with a finite f32 sum."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rustsolver_amd as rs
from oracle import orc
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd.solver import DeviceBuffer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_edge_inputs as kei  # noqa: E402

pytestmark = pytest.mark.gpu
assert (ab.DIST_EMD, ab.DIST_L2) == (orc.DIST_EMD, orc.DIST_L2) == kei.DISTS
BOTH = pytest.mark.parametrize("dist", kei.DISTS, ids=["emd", "l2"])


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


@pytest.fixture(scope="module")
def table():
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    return rs.create_infosets(n_actions, tree, [4], [1])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((bits(got) if got.dtype == np.float32 else got).ravel() != (bits(want) if want.dtype == np.float32 else want).ravel())[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def check_fit_regular(km, data, centres, dist, rounds):
    got = km.fit_regular(centres, dist, rounds)
    want = orc.kmeans_fit_regular(data, centres, dist, rounds)
    for g, w, what in zip(got, want, ("clusters", "centres", "bounds", "inertia")):
        same(g, w, "fit_regular " + what)
    return want


def check_fit_growbatch(km, data, order, batch, centres, dist):
    got = km.fit_growbatch(order, batch, centres, dist)
    want = orc.kmeans_fit_growbatch(data, order, batch, centres, dist)
    for g, w, what in zip(got, want, ("clusters", "centres", "bounds", "stats")):
        same(g, w, "fit_growbatch " + what)
    return want


def check_reassign(km, data, centres, s, clusters, bounds, dist, order=None):
    oc, ob = clusters.copy(), bounds.copy()
    orc.kmeans_reassign(data, centres, s, oc, ob, dist, order=order)
    gc, gb = km.reassign(centres, s, clusters, bounds, dist, order=order)
    same(gc, oc, "reassign clusters")
    same(gb, ob, "reassign bounds")
    return oc, ob


# ---- widths: every instantiated NB of the training kernels' dispatch and the width just above it; 63 and 64 = the last lanes of k_kmeans_center_sums' wave --------------

@BOTH
@pytest.mark.parametrize("n_bins", kei.WIDTHS)
def test_widths_init_s_and_reassign(table, n_bins, dist):
    c = kei.width_case(n_bins)
    data, centres = c["data"], c["dup"]
    km = ab.Kmeans(table, data)
    s = np.full(len(centres), kei.FLT_MAX, dtype=np.float32)
    for _ in range(2):                                   # s is in/out: the second call starts from the halved values
        got = km.init_s(centres, s, dist)
        same(got, orc.kmeans_init_s(centres, s.copy(), dist), "init_s")
        s = got
    check_reassign(km, data, centres, s, c["clusters"], c["bounds"], dist)
    m = len(c["sub"])
    check_reassign(km, data, centres, s, c["clusters"][:m], c["bounds"][:m], dist, order=c["sub"])
    zeroed = c["zeroed"]                                 # a zero centre: emd_1d's zero-sum shortcut on the datum side of init_s and the centre side of reassign
    s0 = np.full(len(zeroed), kei.FLT_MAX, dtype=np.float32)
    got = km.init_s(zeroed, s0, dist)
    same(got, orc.kmeans_init_s(zeroed, s0.copy(), dist), "init_s, zero centre")
    check_reassign(km, data, zeroed, s, c["clusters"], c["bounds"], dist)


@BOTH
@pytest.mark.parametrize("n_bins", kei.WIDTHS)
def test_widths_fit_regular(table, n_bins, dist):
    c = kei.width_case(n_bins)
    check_fit_regular(ab.Kmeans(table, c["data"]), c["data"], c["centres"], dist, kei.WIDTH_ROUNDS)


@BOTH
@pytest.mark.parametrize("n_bins", kei.WIDTHS[:-1])      # 64 bins: test_refusals_leave_the_outputs_untouched
def test_widths_fit_growbatch(table, n_bins, dist):
    c = kei.width_case(n_bins)
    check_fit_growbatch(ab.Kmeans(table, c["data"]), c["data"], c["order"], kei.WIDTH_BATCH, c["centres"], dist)


# ---- cluster counts ---------------------------------------------------------------------------------------------------------------------------------------------------

COUNTS = [(k, dist, fit) for k in kei.COUNT_CASES for dist in kei.COUNT_CASES[k][3] for fit in ("regular", "growbatch")]


@pytest.mark.parametrize("k,dist,fit", COUNTS, ids=["%d-%s-%s" % (k, "emd" if d == kei.DIST_EMD else "l2", f) for k, d, f in COUNTS])
def test_cluster_counts(table, k, dist, fit):
    c = kei.count_case(k)
    km = ab.Kmeans(table, c["data"])
    if fit == "regular":
        check_fit_regular(km, c["data"], c["centres"], dist, c["rounds"])
    else:
        check_fit_growbatch(km, c["data"], c["order"], c["batch"], c["centres"], dist)


# ---- member lists of 0, 1, 2, 3, 31, 32 and 33 and every start alignment of a lane's staged row --------------------------------------------------------------------------

@BOTH
def test_list_lengths(table, dist):
    c = kei.lists_case()
    km = ab.Kmeans(table, c["data"])
    for rounds in range(1, kei.LIST_ROUNDS + 1):
        check_fit_regular(km, c["data"], c["centres"], dist, rounds)
    check_fit_growbatch(km, c["data"], c["order"], len(c["data"]), c["centres"], dist)


# ---- sizes: 1, 7, 8 and 9 tiles of the counting sort, one item short of a tile and one past it ---------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("k", kei.SIZE_KS)
@pytest.mark.parametrize("n", kei.SIZES)
def test_sizes(table, n, k, dist):
    c = kei.size_case(n, k)
    km = ab.Kmeans(table, c["data"])
    check_fit_regular(km, c["data"], c["centres"], dist, kei.SIZE_ROUNDS)
    for batch in sorted({n} | ({b for b in kei.SIZE_BATCHES} if n == kei.SIZES[-1] else set())):
        want = check_fit_growbatch(km, c["data"], c["order"], batch, c["centres"], dist)
        if batch == 1:
            assert np.isinf(want[3][0])                  # one item: every count <= 1, sd = inf


# ---- the second trip of the grid-stride loops (n > 16 384 workgroups x 256) ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_km(table):
    return ab.Kmeans(table, kei.long_case()["data"])


@BOTH
def test_long_predict_and_update_min_dists(long_km, dist):
    c = kei.long_case()
    cl, md = long_km.predict(c["centres"], dist)
    ocl, omd = orc.kmeans_predict(c["data"], c["centres"], dist, threads=8)
    same(cl, ocl, "predict clusters")
    same(md, omd, "predict distances")
    want = np.full(kei.LONG_N, 0.125, dtype=np.float32)
    got = long_km.update_min_dists(want, c["centres"][1], dist)
    orc.update_min_dists(want, c["data"], c["centres"][1], dist)
    same(got, want, "update_min_dists")
    assert 0 < (want < 0.125).sum() < kei.LONG_N


@BOTH
def test_long_reassign_with_an_order(long_km, dist):
    c = kei.long_case()
    before = c["bounds"]
    _, ob = check_reassign(long_km, c["data"], c["centres"], c["s"], c["clusters"], before, dist, order=c["order"])
    assert 0 < (ob[:, 1] == before[:, 1]).sum() < kei.LONG_N


def test_long_fit_regular(long_km):
    c = kei.long_case()
    check_fit_regular(long_km, c["data"], c["centres"], kei.DIST_L2, 2)


def test_long_fit_growbatch(long_km):
    c = kei.long_case()
    check_fit_growbatch(long_km, c["data"], c["order"], kei.LONG_N, c["centres"], kei.DIST_L2)


# ---- the f32 member counter of a list of more than 2^24 members ---------------------------------------------------------------------------------------------------------

def test_member_counter_sticks_at_two_to_the_24(table):
    c = kei.counter_case()
    check_fit_regular(ab.Kmeans(table, c["data"]), c["data"], c["centres"], kei.DIST_L2, 1)


# ---- values inside a fit --------------------------------------------------------------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("which", kei.VALUE_CASES)
def test_value_edges(table, which, dist):
    c = kei.value_case(which)
    km = ab.Kmeans(table, c["data"])
    check_fit_regular(km, c["data"], c["centres"], dist, kei.VALUE_ROUNDS)
    check_fit_growbatch(km, c["data"], c["order"], c["batch"], c["centres"], dist)


# ---- optional outputs, one round, one table reused at changing k and width --------------------------------------------------------------------------------------------------

def raw_fit_regular(table, data_buf, n, centres, dist, rounds, clusters0, bounds0, want_inertia=True):
    """rs_kmeans_fit_regular as it is: clusters0 / bounds0 are what the output buffers hold before the call (bounds0 None: d_bounds = NULL)
    -> (return code, clusters, centres, bounds or None, inertia or None)"""
    c = np.array(centres, dtype=np.float32, order="C")
    k, n_bins = c.shape
    dc = DeviceBuffer.from_numpy(table, clusters0)
    db = None if bounds0 is None else DeviceBuffer.from_numpy(table, bounds0)
    inertia = C.c_float(-1.0)
    rc = L.load().rs_kmeans_fit_regular(table._h, dist, data_buf.ptr, n, c.ctypes.data, k, n_bins, rounds, dc.ptr, None if db is None else db.ptr,
                                        C.byref(inertia) if want_inertia else None)
    table.sync()
    return rc, dc.download(np.uint32, n), c, None if db is None else db.download(np.float32, 2 * n).reshape(n, 2), np.float32(inertia.value) if want_inertia else None


def raw_fit_growbatch(table, data_buf, n, order, batch, centres, dist, clusters0, bounds0, want_stats=True):
    c = np.array(centres, dtype=np.float32, order="C")
    k, n_bins = c.shape
    do = DeviceBuffer.from_numpy(table, np.ascontiguousarray(order, dtype=np.uint32))
    dc, db = DeviceBuffer.from_numpy(table, clusters0), DeviceBuffer.from_numpy(table, bounds0)
    stats = np.full(2, -1.0, dtype=np.float32)
    rc = L.load().rs_kmeans_fit_growbatch(table._h, dist, data_buf.ptr, n, do.ptr, batch, c.ctypes.data, k, n_bins, dc.ptr, db.ptr, stats.ctypes.data if want_stats else None)
    table.sync()
    return rc, dc.download(np.uint32, batch), c, db.download(np.float32, 2 * batch).reshape(batch, 2), stats if want_stats else None


def sentinels(n):
    return np.full(n, 0xdeadbeef, dtype=np.uint32), np.full((n, 2), -7.25, dtype=np.float32)


@BOTH
def test_optional_outputs_may_be_null(table, dist):
    c = kei.value_case("zero_rows")
    data, centres, n = c["data"], c["centres"], len(c["data"])
    buf = DeviceBuffer.from_numpy(table, data)
    cl0, b0 = sentinels(n)
    want = orc.kmeans_fit_regular(data, centres, dist, kei.VALUE_ROUNDS)
    for bounds0, want_inertia in ((b0, True), (None, True), (b0, False), (None, False)):
        rc, cl, cent, b, inertia = raw_fit_regular(table, buf, n, centres, dist, kei.VALUE_ROUNDS, cl0, bounds0, want_inertia)
        L.check(rc)
        same(cl, want[0], "clusters")
        same(cent, want[1], "centres")
        if b is not None:
            same(b, want[2], "bounds")
        if want_inertia:
            same(inertia, want[3], "inertia")
    gw = orc.kmeans_fit_growbatch(data, c["order"], c["batch"], centres, dist)
    cl0, b0 = sentinels(c["batch"])
    for want_stats in (True, False):
        rc, cl, cent, b, stats = raw_fit_growbatch(table, buf, n, c["order"], c["batch"], centres, dist, cl0, b0, want_stats)
        L.check(rc)
        for g, w, what in zip((cl, cent, b), gw, ("clusters", "centres", "bounds")):
            same(g, w, "fit_growbatch " + what)
        if want_stats:
            same(stats, gw[3], "stats")


@BOTH
def test_one_round(table, dist):
    c = kei.value_case("centre_rows")
    check_fit_regular(ab.Kmeans(table, c["data"]), c["data"], c["centres"], dist, 1)


@BOTH
def test_one_table_at_changing_k_and_width(table, dist):
    """the table's centre scratch only grows, and reassign finds the zero flags behind the centres from k and the padded width of ITS call"""
    for i in range(len(kei.REUSE)):
        c = kei.reuse_case(i)
        km = ab.Kmeans(table, c["data"])
        check_fit_regular(km, c["data"], c["centres"], dist, 3)
        check_fit_growbatch(km, c["data"], c["order"], c["batch"], c["centres"], dist)


# ---- refusals: before anything is written ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["regular-16385", "growbatch-16385", "growbatch-64-bins"])
def test_refusals_leave_the_outputs_untouched(table, which):
    rng = np.random.Generator(np.random.PCG64(9))
    n, k, n_bins = (300, 16385, 2) if which.endswith("16385") else (300, 5, 64)
    data = kei.histograms(rng, n, n_bins, "dense")
    centres = kei.histograms(rng, k, n_bins, "dense")
    order = rng.permutation(n).astype(np.uint32)
    buf = DeviceBuffer.from_numpy(table, data)
    cl0, b0 = sentinels(n)
    if which.startswith("regular"):
        rc, cl, cent, b, _ = raw_fit_regular(table, buf, n, centres, kei.DIST_L2, 2, cl0, b0)
    else:
        rc, cl, cent, b, _ = raw_fit_growbatch(table, buf, n, order, n, centres, kei.DIST_L2, cl0, b0)
    with pytest.raises(rs.RsError):
        L.check(rc)
    assert (cl == cl0).all() and b.tobytes() == b0.tobytes() and cent.tobytes() == centres.tobytes()
    km = ab.Kmeans(table, data)                              # the same table then fits: the largest legal count / width
    if which.endswith("16385"):
        small = data[rng.choice(n, size=7, replace=False)]
        check_fit_regular(km, data, small, kei.DIST_EMD, 2)
        check_fit_growbatch(km, data, order, n, small, kei.DIST_EMD)
    else:
        check_fit_regular(km, data, centres, kei.DIST_EMD, 2)             # 64 bins are fit_regular's to take
