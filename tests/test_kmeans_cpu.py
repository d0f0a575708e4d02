"""CPU (-m "not gpu"): the abstraction generator's distance functions.

  * the oracle (oracle/kmeans_emd.c, a literal restatement of emd.rs:53-113 / kmeans.rs:622-630) against the reference's OWN known answers
    (gen_abstraction/emd.rs:122-180, tolerance ERROR = 0.01 from emd.rs:120);
  * the product's host-side distance (rs_histogram_distance: the bitmask formulation the GPU kernel uses) against the oracle, bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

import rustsolver_amd as rs
from oracle import orc
from rustsolver_amd import abstraction as ab

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_edge_inputs as kei  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return json.load(open(os.path.join(golden_dir, "kmeans_emd.json")))


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def test_oracle_meets_the_reference_known_answers(fx):
    tol = fx["reference"]["tolerance"]
    for c in fx["reference"]["cases"]:
        got = float(orc.emd_1d(c["p"], c["q"]))
        assert abs(got - c["emd"]) < tol, (c["name"], got, c["emd"])   # assert!(emd < actual + ERROR && emd > actual - ERROR)


def test_emd_of_a_histogram_with_itself_is_three_ulps_not_zero(fx):
    """emd.rs:136 asserts emd(h, h) == 0.0 inside a #[bench].  Evaluated in f32 as written, w = sum of the normalised bins = 1 - 2^-24 for that
    histogram, u = 3, so the function returns (1 - w) * u = 3 * 2^-24: far inside ERROR = 0.01, not equal to 0.0 (numpy float32 agrees)."""
    c = fx["reference"]["cases"][0]
    p = np.array(c["p"], dtype=np.float32)
    s = np.float32(0)
    for x in p:
        s = np.float32(s + x)
    w = np.float32(0)
    for x in p:
        w = np.float32(w + np.float32(x / s))
    assert w == np.float32(1) - np.float32(2.0 ** -24)
    assert orc.emd_1d(p, p) == np.float32(3 * 2.0 ** -24)


def test_oracle_and_host_restated_fixture(fx):
    for c in fx["restated"]:
        p = np.array(c["p_bits"], dtype=np.uint32).view(np.float32)
        q = np.array(c["q_bits"], dtype=np.uint32).view(np.float32)
        assert f32bits(orc.emd_1d(p, q)) == c["emd_bits"] and f32bits(orc.l2_dist(p, q)) == c["l2_bits"]
        assert f32bits(ab.histogram_distance(p, q)) == c["emd_bits"]
        assert f32bits(ab.histogram_distance(p, q, ab.DIST_L2)) == c["l2_bits"]
    for c in fx["reference"]["cases"]:
        assert f32bits(ab.histogram_distance(c["p"], c["q"])) == f32bits(orc.emd_1d(c["p"], c["q"]))


def test_host_distance_equals_oracle_on_fuzzed_histograms():
    """the bitmask formulation (at most n_bins transfers) against the literal 2(u-1) x n_bins probe loop"""
    rng = np.random.Generator(np.random.PCG64(17))
    for _ in range(6000):
        n = int(rng.integers(1, 65))
        p = (rng.random(n) ** rng.integers(1, 7)).astype(np.float32)
        q = (rng.random(n) ** rng.integers(1, 7)).astype(np.float32)
        if rng.random() < 0.3:
            p[rng.random(n) < 0.5] = 0
        if rng.random() < 0.3:
            q[rng.random(n) < 0.5] = 0
        if rng.random() < 0.1:
            q = np.roll(p, int(rng.integers(0, n)))       # same mass, shifted: pure cross-bin work
        assert f32bits(ab.histogram_distance(p, q)) == f32bits(orc.emd_1d(p, q)), (n, p, q)
        assert f32bits(ab.histogram_distance(p, q, ab.DIST_L2)) == f32bits(orc.l2_dist(p, q))


def test_emd_edge_cases():
    z = np.zeros(8, dtype=np.float32)
    h = np.arange(8, dtype=np.float32)
    for f in (orc.emd_1d, ab.histogram_distance):
        assert f(z, h) == 0.0 and f(h, z) == 0.0 and f(z, z) == 0.0          # emd.rs:59-61
        assert f(np.float32([1]), np.float32([5])) == 0.0                      # one bin: all mass matches
    a = np.float32([1, 0, 0, 0]); b = np.float32([0, 0, 0, 1])
    assert orc.emd_1d(a, b) == ab.histogram_distance(a, b) == np.float32(3.0)  # u = 4: offset 3 is reachable, cost 1 * 3
    with pytest.raises(rs.RsError):
        ab.histogram_distance(np.zeros(65, np.float32), np.zeros(65, np.float32))
    with pytest.raises(ValueError):
        ab.histogram_distance(np.zeros(4, np.float32), np.zeros(5, np.float32))


def test_oracle_predict_takes_the_first_strict_minimum():
    """kmeans.rs:194-202: `if variance[k] < min_variance` -- ties keep the earlier center"""
    data = np.float32([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]])
    centers = np.float32([[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]])
    cl, md = orc.kmeans_predict(data, centers, orc.DIST_EMD)
    assert cl.tolist() == [1, 3, 0] and md.tolist() == [0.0, 1.0, 0.0]
    cl2, _ = orc.kmeans_predict(data, centers, orc.DIST_L2, threads=3)
    assert cl2.tolist() == [1, 0, 0]      # [0,0,0,1] and the empty histogram are equidistant from every center: the first one wins


# ---- the oracle's training loops (oracle/kmeans_fit.c): what they are pinned by, since the reference holds no test for them ---------------------

def _hist(rng, n, n_bins):
    return kei.histograms(rng, n, n_bins, "counts")


def test_oracle_hamerly_assignment_is_the_brute_force_assignment():
    """reassign_clusters only SKIPS distance evaluations (kmeans.rs:287-334): after every round of fit_regular the clusters must be Kmeans::predict's arg-min against
    the centers that round's reassign saw.  Exact for l2_dist (a metric).  emd_1d is a heuristic WITHOUT a triangle inequality, so with it the reference's own
    bounds skip evaluations they should not (about one datum in ten changes cluster here): for EMD the check is only that most assignments agree -- the
    disagreement is the reference's algorithm, reproduced, not an error of the restatement (the GPU path must match the oracle bit for bit either way)."""
    rng = np.random.Generator(np.random.PCG64(5))
    data = _hist(rng, 4000, 20)
    centers = data[rng.choice(len(data), size=25, replace=False)].copy()
    for kind, floor in ((orc.DIST_L2, 1.0), (orc.DIST_EMD, 0.8)):
        prev = centers
        for it in range(1, 6 if kind == orc.DIST_L2 else 3):   # EMD: a cluster that runs empty becomes the zero histogram, at emd distance 0 from everything
            cl, cent, bounds, inertia = orc.kmeans_fit_regular(data, centers, kind, it)
            want, _ = orc.kmeans_predict(data, prev, kind)
            assert (cl == want).mean() >= floor, (kind, it, (cl == want).mean())
            assert (bounds[:, 1] >= 0).all()
            prev = cent


def test_oracle_fit_regular_first_round_by_hand():
    """one round from scratch is plain k-means: every bound starts at (0, f32::MAX), so every datum scans all centers; means are sums in data order / counts,
    bins that sum to 0 stay 0 (kmeans.rs:537), and the centers come back as those means"""
    rng = np.random.Generator(np.random.PCG64(6))
    data = _hist(rng, 500, 8)
    centers = data[:5].copy()
    cl, cent, bounds, inertia = orc.kmeans_fit_regular(data, centers, orc.DIST_L2, 1)
    want_cl, want_d = orc.kmeans_predict(data, centers, orc.DIST_L2)
    assert (cl == want_cl).all()
    for j in range(5):
        acc = np.zeros(8, dtype=np.float32)
        cnt = np.float32(0)
        for i in np.nonzero(cl == j)[0]:                      # ascending data order, f32
            acc = (acc + data[i]).astype(np.float32)
            cnt = np.float32(cnt + np.float32(1))
        mean = np.where(acc > 0, (acc / cnt).astype(np.float32), acc)
        assert mean.view(np.uint32).tolist() == cent[j].view(np.uint32).tolist()
    mv = np.array([orc.l2_dist(cent[j], centers[j]) for j in range(5)], dtype=np.float32)
    assert (bounds[:, 1].view(np.uint32) == (want_d + mv[cl]).astype(np.float32).view(np.uint32)).all()   # upper = distance + own center's movement


def test_oracle_init_s_is_in_out_as_coded():
    """kmeans.rs:518 creates s once; init_s (:267-285) lowers and halves it, so a second call on unchanged centers halves it AGAIN"""
    rng = np.random.Generator(np.random.PCG64(7))
    centers = _hist(rng, 6, 10)
    s = np.full(6, np.finfo(np.float32).max, dtype=np.float32)
    orc.kmeans_init_s(centers, s, orc.DIST_L2)
    want = np.array([min(orc.l2_dist(centers[i], centers[j]) for j in range(6) if j != i) / np.float32(2) for i in range(6)], dtype=np.float32)
    assert s.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    orc.kmeans_init_s(centers, s, orc.DIST_L2)
    assert s.view(np.uint32).tolist() == (want / np.float32(2)).astype(np.float32).view(np.uint32).tolist()


def test_oracle_growbatch_is_one_pass_over_the_batch():
    rng = np.random.Generator(np.random.PCG64(8))
    data = _hist(rng, 3000, 12)
    centers = data[rng.choice(3000, size=9, replace=False)].copy()
    order = rng.permutation(3000).astype(np.uint32)
    cl, cent, bounds, stats = orc.kmeans_fit_growbatch(data, order, 700, centers, orc.DIST_L2)
    want, _ = orc.kmeans_predict(data[order[:700]], centers, orc.DIST_L2)
    assert (cl == want).all()                                  # first round: a datum keeps cluster 0 only if it is within s[0] of it, else it scans every center
    assert np.isfinite(stats).all() and stats[1] > 0
    for j in range(9):
        if (cl == j).sum() == 0:
            assert (cent[j] == 0).all()                        # empty cluster: the mean of nothing is the zero histogram (`count > 0.0`, kmeans.rs:412)


def test_oracle_pick_restart_by_hand():
    """three candidate sets of three centers on a line (l2_dist): the mean pairwise distance by hand, the arg-max, and the last-of-equal-maxima rule of max_by"""
    def line(xs):
        return np.array([[x, 0.0] for x in xs], dtype=np.float32)
    cands = np.stack([line([0, 1, 2]), line([0, 3, 6]), line([1, 4, 7])])     # mean pairwise distances 4/3, 4, 4
    best, cd = orc.kmeans_pick_restart(cands, orc.DIST_L2)
    assert np.allclose(cd, [8.0 / 6.0, 4.0, 4.0]) and best == 2


# ---- premises of tests/kmeans_edge_inputs.py: every edge case reaches its edge, shown with the oracle alone (test_gpu_kmeans_edges.py runs the device on the same arrays) ----

def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def last_reassign(data, centres, kind, rounds):
    """round `rounds`' reassign of orc.kmeans_fit_regular, replayed from the oracle's own state after rounds - 1 rounds (s is in/out: every round's init_s is replayed)
    -> (data whose upper bound that reassign left as it was, data whose lower bound it rewrote, n)"""
    s = np.full(len(centres), kei.FLT_MAX, dtype=np.float32)
    cl, cents, b = None, np.array(centres), None
    for r in range(rounds):
        if r:
            cl, cents, b, _ = orc.kmeans_fit_regular(data, centres, kind, r)
        orc.kmeans_init_s(cents, s, kind)
    before = b.copy()
    orc.kmeans_reassign(data, cents, s, cl, b, kind)
    if kind == orc.DIST_L2:                                                              # the replay is the fit's own last round (checked where the fit is cheap)
        assert (cl == orc.kmeans_fit_regular(data, centres, kind, rounds)[0]).all()
    return int((_bits(b[:, 1]) == _bits(before[:, 1])).sum()), int((_bits(b[:, 0]) != _bits(before[:, 0])).sum()), len(data)


def _multi_round_cases():
    """every fit of more than one round that test_gpu_kmeans_edges.py runs -> (name = case-...-kind, getter of the case, kind, rounds).  The one-round fits (the counter
    case, k = 16 384, every growbatch) have no last round to replay; the long fit runs under L2 only."""
    for nb in kei.WIDTHS:
        for kind in kei.DISTS:
            yield "width-%d-%d" % (nb, kind), (lambda nb=nb: kei.width_case(nb)), kind, kei.WIDTH_ROUNDS
    for k in (2, 256, 257, 4000):
        for kind in kei.DISTS:
            yield "count-%d-%d" % (k, kind), (lambda k=k: kei.count_case(k)), kind, kei.COUNT_CASES[k][2]
    yield "long-%d" % kei.DIST_L2, kei.long_case, kei.DIST_L2, 2
    for kind in kei.DISTS:
        yield "lists-%d" % kind, kei.lists_case, kind, kei.LIST_ROUNDS
        for n in kei.SIZES:
            for k in kei.SIZE_KS:
                yield "size-%d-%d-%d" % (n, k, kind), (lambda n=n, k=k: kei.size_case(n, k)), kind, kei.SIZE_ROUNDS
        for which in kei.VALUE_CASES:
            yield "value-%s-%d" % (which, kind), (lambda which=which: kei.value_case(which)), kind, kei.VALUE_ROUNDS
        for i in range(len(kei.REUSE)):
            yield "reuse-%d-%d" % (i, kind), (lambda i=i: kei.reuse_case(i)), kind, 3


# the multi-round fits in which NO input of the case's shape can make one round both skip and scan, each with its reason; every other case asserts the premise
_ONE_DATUM = "a single datum does one or the other"
_TWO_DATA = "both data hold an exact lower bound after round 1 and settle in round 2: the last round scans nothing (the oracle keeps 2 of 2)"
_CANNOT_SKIP_AND_SCAN = {
    "width-1-0": "one bin under EMD: every distance is 0, so from round 2 on every datum is skipped (the oracle keeps 2003 of 2003)",
    "value-zero_centre-0": "a supplied zero centre under EMD is at distance 0 from every datum: it takes all of them in round 1, every other cluster empties, and "
                           "from then on nothing scans (the oracle keeps 2996 of 3000 and rewrites no lower bound)",
}
_CANNOT_SKIP_AND_SCAN.update({"size-1-%d-%d" % (k, kind): _ONE_DATUM for k in kei.SIZE_KS for kind in kei.DISTS})
_CANNOT_SKIP_AND_SCAN.update({"size-2-%d-%d" % (k, kind): _TWO_DATA for k in kei.SIZE_KS for kind in kei.DISTS})
_ALL_MULTI = list(_multi_round_cases())
assert set(_CANNOT_SKIP_AND_SCAN) <= {c[0] for c in _ALL_MULTI}
_MULTI = [c for c in _ALL_MULTI if c[0] not in _CANNOT_SKIP_AND_SCAN]


@pytest.mark.parametrize("name", sorted(_CANNOT_SKIP_AND_SCAN))
def test_premise_exclusions_are_what_their_reasons_say(name):
    """a case on the exclusion table does not do both -- were one to, it belongs in the premise test below"""
    _, case, kind, rounds = next(c for c in _ALL_MULTI if c[0] == name)
    c = case()
    kept, scanned, n = last_reassign(c["data"], c["centres"], kind, rounds)
    assert not (0 < kept < n and scanned > 0), (name, kept, scanned, n)


@pytest.mark.parametrize("name,case,kind,rounds", _MULTI, ids=[c[0] for c in _MULTI])
def test_premise_last_round_skips_some_data_and_scans_some(name, case, kind, rounds):
    c = case()
    kept, scanned, n = last_reassign(c["data"], c["centres"], kind, rounds)
    assert 0 < kept < n and scanned > 0, (name, kept, scanned, n)


@pytest.mark.parametrize("kind", kei.DISTS)
def test_premise_list_lengths_and_row_alignments(kind):
    c = kei.lists_case()
    k, n_bins = c["centres"].shape
    want = {0, 1, 2, 3, 31, 32, 33}
    first = orc.kmeans_fit_regular(c["data"], c["centres"], kind, 1)[0]
    own = c["group"] != kei.NO_GROUP
    assert (first[own] == c["group"][own]).all() and (first[~own] >= k - 2).all()   # round 1 is the full scan: the lists are the groups, the bridge joins the last two
    for r in range(1, kei.LIST_ROUNDS + 1):
        lengths, residues = kei.list_facts(orc.kmeans_fit_regular(c["data"], c["centres"], kind, r)[0], k, n_bins)
        # L2: the lists keep their lengths in every round.  EMD: list 0 is empty after round 1 alone -- its centre is then the zero histogram, at distance 0 from every
        # datum that scans in round 2, which refills it -- so the later rounds hold the other six lengths
        assert (want if r == 1 or kind == orc.DIST_L2 else want - {0}) <= lengths, (r, sorted(lengths))
        assert residues == {0, 1, 2, 3}, (r, residues)
    cl = orc.kmeans_fit_growbatch(c["data"], c["order"], len(c["data"]), c["centres"], kind)[0]
    lengths, residues = kei.list_facts(cl, k, n_bins + 1)                         # growbatch stages one more row: the upper bounds
    assert want <= lengths and residues == {0, 1, 2, 3}


def test_premise_emptied_cluster_becomes_the_zero_centre():
    c = kei.value_case("emptied")
    cl, cent, _, _ = orc.kmeans_fit_regular(c["data"], c["centres"], orc.DIST_EMD, 1)
    assert not (cl == 5).any() and (cent[5] == 0).all() and kei.VALUE_ROUNDS > 1
    later = orc.kmeans_fit_regular(c["data"], c["centres"], orc.DIST_EMD, kei.VALUE_ROUNDS)[0]
    assert (later == 5).any()                                                     # at emd distance 0 from everything: it takes every datum that scans


def test_premise_f32_member_counter_sticks_at_two_to_the_24():
    c = kei.counter_case()
    data = c["data"]
    cl, cent, _, _ = orc.kmeans_fit_regular(data, c["centres"], orc.DIST_L2, 1)
    members = np.nonzero(cl == 0)[0]
    assert len(members) > 2 ** 24 + 32 and len(members) == kei.COUNTER_N - 3 and (np.nonzero(cl == 1)[0] == c["far"]).all()
    total = np.add.accumulate(data[members, 0], dtype=np.float32)[-1]             # f32, strictly in data order
    assert _bits(cent[0])[0] == _bits(total / np.float32(2 ** 24))[0]
    assert _bits(cent[0])[0] != _bits(total / np.float32(len(members)))[0]


def test_premise_long_case_needs_a_second_grid_trip():
    assert len(kei.long_case()["data"]) > 16384 * 256


@pytest.mark.parametrize("which", kei.VALUE_CASES)
def test_premise_value_edges_stay_finite_and_host_distance_agrees(which):
    c = kei.value_case(which)
    data, centres = c["data"], c["centres"]
    if which == "subnormal":
        tiny = np.finfo(np.float32).tiny
        assert ((data[::7] > 0) & (data[::7] < tiny)).any() and ((centres[0] > 0) & (centres[0] < tiny)).any()
    if which == "neg_zero":
        assert np.signbit(data[data == 0]).any() and np.signbit(centres[centres == 0]).any()
    if which == "centre_rows":
        assert sum((data == q).all(axis=1).sum() for q in centres) > len(centres)
    for kind in kei.DISTS:
        cl, cent, b, inertia = orc.kmeans_fit_regular(data, centres, kind, kei.VALUE_ROUNDS)
        assert np.isfinite(cent).all() and np.isfinite(b).all() and np.isfinite(inertia)
        cl, cent, b, stats = orc.kmeans_fit_growbatch(data, c["order"], c["batch"], centres, kind)
        assert np.isfinite(cent).all() and np.isfinite(b).all() and np.isfinite(stats).all()
        f = orc.emd_1d if kind == orc.DIST_EMD else orc.l2_dist
        rows = np.concatenate([data[:140], cent])                                 # the host distance on the value-edge rows, and on the means they make
        for p in rows:
            for q in centres:
                assert f32bits(ab.histogram_distance(p, q, kind)) == f32bits(f(p, q))
                assert f32bits(ab.histogram_distance(q, p, kind)) == f32bits(f(q, p))


@pytest.mark.parametrize("n_bins", kei.WIDTHS)
def test_premise_width_cases_hold_a_zero_centre_and_a_duplicate_for_init_s(n_bins):
    c = kei.width_case(n_bins)
    dup = c["zeroed"]
    assert (dup[11] == 0).all() and (dup[7] == dup[2]).all() and (dup[2] != 0).any() and (c["data"][::131] == 0).all()
    assert (c["dup"].sum(axis=1) > 0).all() and (c["dup"][7] == c["dup"][2]).all()
    s = orc.kmeans_init_s(dup, np.full(len(dup), kei.FLT_MAX, dtype=np.float32), orc.DIST_EMD)
    assert (s == 0).all()                                      # at emd distance 0 from the zero centre, every one of them; the zero centre from all
    s = orc.kmeans_init_s(dup, np.full(len(dup), kei.FLT_MAX, dtype=np.float32), orc.DIST_L2)
    assert s[7] == 0 and s[2] == 0 and ((s > 0).sum() == len(dup) - 2 or n_bins == 1)
