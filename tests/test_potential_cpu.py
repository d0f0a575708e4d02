"""CPU: the greedy earth mover's distance of the potential-aware abstraction on the host (rs_pa_distance) against the numpy restatement tests/np_potential.py, bit for
bit; the restatement's own identities; every refusal of a malformed row, mean or ground.  No GPU, no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_potential as npp  # noqa: E402
import potential_edge_inputs as pe  # noqa: E402

F32 = np.float32
SIZES = [1, 2, 3, 7, 64, 65, 300]
PAIRS = {1: 300, 2: 400, 3: 400, 7: 400, 64: 250, 65: 250, 300: 120}      # 2 120 pairs


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


class Rows:      # what PotentialKmeans asks of its rows on the host
    def __init__(self, n_draws):
        self.n_draws, self.rows = n_draws, 0


def host_metric(ground, n_draws):
    return ab.PotentialKmeans(None, Rows(n_draws), ground)


def random_means(rng, rows, n_next, n_draws):
    """one mean per row: a dense random one, a sparse one, the mean of two points, the point itself; masses below, at and above 1"""
    out = np.zeros((len(rows), n_next), dtype=F32)
    dense = npp.dense(rows, n_next, n_draws)
    for i in range(len(rows)):
        kind = i % 5
        if kind == 0:
            q = rng.random(n_next).astype(F32)
            q = q / q.sum(dtype=F32)
        elif kind == 1:
            q = np.where(rng.random(n_next) < 0.3, rng.random(n_next), 0).astype(F32)
            q = q / max(q.sum(dtype=F32), F32(1))
        elif kind == 2:
            q = ((dense[i].astype(np.float64) + dense[(i + 1) % len(rows)]) / 2).astype(F32)
        elif kind == 3:
            q = dense[i] * F32(0.5)                                  # mass 0.5: targets stay unfinished
        else:
            q = rng.random(n_next).astype(F32) * F32(4.0 / n_next)   # mass about 2
        out[i] = q
    return out


@pytest.fixture(scope="module")
def cases():
    """per n_next: (ground, n_draws, rows, means, restated distances), computed once"""
    out = {}
    for n_next in SIZES:
        rng = np.random.Generator(np.random.PCG64(1000 + n_next))
        for which, ground in (("ties", npp.tie_ground(n_next)), ("random", npp.random_ground(rng, n_next, duplicates=2))):
            n_draws = 47 if which == "ties" else 46
            rows = npp.random_rows(rng, PAIRS[n_next] // 2, n_next, n_draws)
            means = random_means(rng, rows, n_next, n_draws)
            want = npp.distances(rows, means, ground, n_draws)
            for a in (ground, rows, means, want):
                a.setflags(write=False)
            out[(n_next, which)] = (ground, n_draws, rows, means, want)
    return out


# ---- the restatement's identities ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_next", [2, 7, 65])
def test_a_point_is_at_distance_zero_from_itself(cases, n_next):
    ground, n_draws, rows, _, _ = cases[(n_next, "random")]
    d = npp.distances(rows, npp.dense(rows, n_next, n_draws), ground, n_draws)
    assert (bits(d) == 0).all()                                           # +0.0


def test_one_bucket_gives_zero(cases):
    for which in ("ties", "random"):
        ground, n_draws, rows, means, want = cases[(1, which)]
        assert (bits(want) == 0).all() and (means > 0).any()


@pytest.mark.parametrize("n_next", [3, 64, 300])
def test_the_early_exits_do_not_change_bits(cases, n_next):
    for which in ("ties", "random"):
        ground, n_draws, rows, means, want = cases[(n_next, which)]
        few = slice(0, 40)
        ranks = []
        full = npp.distances(rows[few], means[few], ground, n_draws, exits=False, ranks=ranks)
        assert ranks == [n_next] and (bits(full) == bits(want[few])).all()
        one_by_one = [npp.distances(rows[i:i + 1], means[i:i + 1], ground, n_draws)[0] for i in range(10)]
        assert (bits(np.asarray(one_by_one, dtype=F32)) == bits(want[:10])).all()


def test_a_mean_of_mass_one_half_leaves_targets_unfinished_and_still_returns():
    ground = npp.tie_ground(7)
    row = npp.pack_row([1, 5], [20, 27])
    q = npp.dense(row, 7, 47)[0] * F32(0.5)
    ranks = []
    d = npp.distances(row, q, ground, 47, ranks=ranks)
    assert bits(d)[0] == 0 and ranks[0] < 7                                # everything it could take lay at distance 0; then nothing is positive
    q2 = np.zeros(7, dtype=F32)
    q2[3] = 0.5
    d2 = npp.distances(row, q2, ground, 47)[0]                              # entry 0 takes 20/47 from two steps away, entry 1 the rest
    t0 = F32(20) / F32(47)
    assert d2 == (F32(0) + t0 * F32(2)) + (F32(0.5) - t0) * F32(2)
    assert host_metric(ground, 47).distance(row, q2) == d2


# ---- rs_pa_distance -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ties", "random"])
@pytest.mark.parametrize("n_next", SIZES)
def test_the_host_distance_equals_the_restatement(cases, n_next, which):
    ground, n_draws, rows, means, want = cases[(n_next, which)]
    km = host_metric(ground, n_draws)
    got = np.asarray([km.distance(r, q) for r, q in zip(rows, means)], dtype=F32)
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (n_next, which, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    entries = (rows != 0).sum(axis=1)
    assert {1, min(2, n_next)} <= set(entries.tolist()) and entries.max() == min(47, n_next, n_draws)


def test_the_cases_are_about_two_thousand_pairs(cases):
    assert sum(len(c[2]) for c in cases.values()) == 2120


# ---- ranks above 511, the values at the edges: the inputs test_gpu_potential_edges.py runs on the device (tests/potential_edge_inputs.py) ---------------------------
def test_a_trace_only_listens(cases):
    ground, n_draws, rows, means, want = cases[(65, "random")]
    trace = []
    assert (bits(npp.distances(rows, means, ground, n_draws, trace=trace)) == bits(want)).all()
    assert len(trace) > len(rows) and all(0 <= p < len(rows) and 0 <= r < 65 and rows[p, e] != 0 for p, r, e in trace)
    for pair in (0, 1, 2, len(rows) - 1):            # one pair's takes come in the definition's order: by rank, then by entry
        own = [(r, e) for p, r, e in trace if p == pair]
        assert own == sorted(own) and len(set(own)) == len(own) > 0
    facts = pe.rank_facts([(0, 600, 1), (0, 1030, 0), (1, 600, 1), (1, 1030, 1), (2, 100, 0), (2, 513, 1), (3, 1023, 0), (3, 1024, 1), (3, 5000, 1)])
    assert facts == ([0, 3], 5000)                   # pair 1: one entry; pair 2: the first take is below 512


@pytest.mark.parametrize("n_next,which", pe.HIGH_RANK_CASES)
def test_the_high_rank_inputs_hold_their_premises(n_next, which):
    c = pe.high_rank_case(n_next, which)
    entries = (c["rows"] != 0).sum(axis=1)
    assert all(npp.well_formed(r, n_next, c["n_draws"]) for r in c["rows"]) and int((c["rows"] >> 8).max()) > n_next // 2
    assert c["pairs_ordered_by_a_high_bit"] >= 1     # two entries of one pair take at r1 < r2, r1 >= 512, (r1 & 511) > (r2 & 511): bits 9 and up put r1 first
    assert c["highest_take_rank"] == n_next - 1 > 4032      # a take in the last, ragged round of 64 ranks (4099) or at the last rank there can be (8192)
    assert np.isfinite(c["want"]).all()
    if n_next == 8192:
        assert len(c["rows"]) == 8 and entries.max() == 4 and c["means"].shape == (3, 8192)
    else:
        assert len(c["rows"]) == 40 and {1, 2, 47} <= set(entries.tolist()) and c["means"].shape == (6, 4099)
        assert (bits(c["means"][0]) == bits(c["means"][1])).all() and not (pe.choice_of(c["want"])[0] == 1).any()
        mass = c["means"].sum(axis=1, dtype=np.float64)
        assert abs(mass[3] - 0.5) < 1e-6 and abs(mass[4] - 1.5) < 1e-6 and (c["means"][5] > 0).sum() == 5
        assert which != "ties" or c["five_lowest_rank"] >= 512      # the five buckets of 0.2 lie above rank 512 from every bucket of the 34 rows below 1024


@pytest.mark.parametrize("n_next,which", pe.HIGH_RANK_CASES)
def test_the_host_distance_equals_the_restatement_at_high_ranks(n_next, which):
    c = pe.high_rank_case(n_next, which)
    km = host_metric(c["ground"], c["n_draws"])
    got = np.asarray([[km.distance(r, q) for q in c["means"]] for r in c["rows"]], dtype=F32)
    bad = np.argwhere(bits(got) != bits(c["want"]))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("name", pe.VALUE_CASES)
def test_the_host_distance_equals_the_restatement_at_value_edges(name):
    c = pe.value_case(name)
    pe.value_premises(name, c)
    km = host_metric(c["ground"], c["n_draws"])
    got = np.asarray([[km.distance(r, q) for q in c["means"]] for r in c["rows"]], dtype=F32)
    bad = np.argwhere(bits(got) != bits(c["want"]))
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), got[tuple(bad[:5].T)], c["want"][tuple(bad[:5].T)])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def raw_distance(metric, row, n_draws, mean):
    out = C.c_float(-1.0)
    r = np.ascontiguousarray(row, dtype=np.uint32)
    m = np.ascontiguousarray(mean, dtype=F32)
    return L.load().rs_pa_distance(metric._h, r.ctypes.data, n_draws, m.ctypes.data, C.byref(out)), out.value


def test_malformed_rows_and_means_are_refused():
    km = host_metric(npp.tie_ground(7), 47)
    mean = np.full(7, 1 / 7, dtype=F32)
    good = npp.pack_row([1, 5], [20, 27])
    assert raw_distance(km, good, 47, mean)[0] == L.OK
    bad_rows = {
        "not ascending": npp.pack_row([5, 1], [20, 27]),
        "a bucket twice": npp.pack_row([5, 5], [20, 27]),
        "a bucket past n_next": npp.pack_row([1, 7], [20, 27]),
        "a count of 0 ahead of a used word": np.concatenate([[1 << 8 | 20, 3 << 8, 5 << 8 | 27], np.zeros(45)]).astype(np.uint32),
        "a zero word ahead of a used word": np.concatenate([[1 << 8 | 20, 0, 5 << 8 | 27], np.zeros(45)]).astype(np.uint32),
        "bucket 0 with count 0 first": np.concatenate([[0, 5 << 8 | 47], np.zeros(46)]).astype(np.uint32),
        "a last count of 0": npp.pack_row([1, 5], [47, 0]),
        "counts short of n_draws": npp.pack_row([1, 5], [20, 26]),
        "counts past n_draws": npp.pack_row([1, 5], [20, 28]),
        "no entry": np.zeros(48, dtype=np.uint32),
    }
    for name, row in bad_rows.items():
        assert not npp.well_formed(row, 7, 47), name
        rc, out = raw_distance(km, row, 47, mean)
        assert rc == L.ERR_INVALID and out == -1.0, name
    assert npp.well_formed(good, 7, 47) and raw_distance(km, good, 46, mean)[0] == L.ERR_INVALID      # the counts sum to 47
    for n_draws in (0, -1, 48):
        assert raw_distance(km, good, n_draws, mean)[0] == L.ERR_INVALID
    for value in (-1e-6, np.nan, np.inf, -np.inf):
        q = mean.copy()
        q[4] = value
        assert raw_distance(km, good, 47, q)[0] == L.ERR_INVALID, value
    q = mean.copy()
    q[4] = -0.0                                                               # -0.0 is not negative
    assert raw_distance(km, good, 47, q)[0] == L.OK
    lib = L.load()
    out = C.c_float()
    assert lib.rs_pa_distance(None, good.ctypes.data, 47, mean.ctypes.data, C.byref(out)) == L.ERR_INVALID
    assert lib.rs_pa_distance(km._h, None, 47, mean.ctypes.data, C.byref(out)) == L.ERR_INVALID
    assert lib.rs_pa_distance(km._h, good.ctypes.data, 47, None, C.byref(out)) == L.ERR_INVALID
    assert lib.rs_pa_distance(km._h, good.ctypes.data, 47, mean.ctypes.data, None) == L.ERR_INVALID


def test_bad_grounds_are_refused():
    lib = L.load()
    h = C.c_void_p()
    good = npp.tie_ground(3)
    for value in (-1.0, np.nan, np.inf):
        g = good.copy()
        g[1, 2] = value
        assert lib.rs_pa_metric_create(None, g.ctypes.data, 3, C.byref(h)) == L.ERR_INVALID and not h.value, value
    for n_next in (0, -1, ab.PA_MAX_NEXT + 1):
        assert lib.rs_pa_metric_create(None, good.ctypes.data, n_next, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.rs_pa_metric_create(None, None, 3, C.byref(h)) == L.ERR_INVALID
    assert lib.rs_pa_metric_create(None, good.ctypes.data, 3, None) == L.ERR_INVALID
    lib.rs_pa_metric_destroy(None)                                           # like free
    with pytest.raises(ValueError):
        ab.PotentialKmeans(None, Rows(47), np.zeros((3, 4), dtype=F32))


def test_equal_distances_go_to_the_lower_id():
    """|i - j| from bucket 3 of 7: 3, then 2 before 4, 1 before 5, 0 before 6.  A mean on {2, 4} alone is emptied in that order"""
    assert npp.order_of(npp.tie_ground(7))[3].tolist() == [3, 2, 4, 1, 5, 0, 6]
    km = host_metric(npp.tie_ground(7), 47)
    row = npp.pack_row([3], [47])
    q = np.zeros(7, dtype=F32)
    q[2], q[4], q[6] = 0.75, 0.125, 0.5
    want = ((F32(0.75) * F32(1)) + F32(0.125) * F32(1)) + F32(0.125) * F32(3)
    assert km.distance(row, q) == want == npp.distances(row, q, npp.tie_ground(7), 47)[0]


def test_dense_rows_and_sparse_rows_agree():
    rng = np.random.Generator(np.random.PCG64(5))
    rows = npp.random_rows(rng, 20, 65, 46)
    assert (bits(ab.dense_rows(rows, 65, 46)) == bits(npp.dense(rows, 65, 46))).all()
    assert ab.dense_rows(rows[0], 65, 46).shape == (65,)
    assert (npp.counts_of(rows, 65).sum(axis=1) == 46).all() and all(npp.well_formed(r, 65, 46) for r in rows)
