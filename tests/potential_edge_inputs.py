"""Inputs of the rank, size and value edge cases of the greedy-EMD assignment (rs_potential.hip), with what the numpy restatement tests/np_potential.py makes of them.
test_potential_cpu.py settles them (the premises hold, the host rs_pa_distance agrees), test_gpu_potential_edges.py runs the device on the same arrays.  Every case is
built once per process and handed out read-only.  Nothing here touches the library."""
import functools

import numpy as np

import np_potential as npp

F32 = np.float32
FLT_MAX = np.finfo(F32).max
HIGH_RANK_CASES = [(4099, "ties"), (4099, "duplicates"), (8192, "ties")]
HIGH_RANK_SEEDS = {(4099, "ties"): 4099, (4099, "duplicates"): 4100, (8192, "ties"): 8192}
FIVE_RANKS = {4099: (2040, 2500, 3000, 3500, 4098), 8192: (4090, 5600, 6600, 7600, 8191)}      # the low nine bits descend, so a later take stands at a lower `rank & 511`


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def rank_facts(trace):
    """what a trace of npp.distances says about high ranks -> (the pairs in which two different entries take at ranks r1 < r2 with r1 >= 512 and
    (r1 & 511) > (r2 & 511): only a bit at or above 9 puts r1 first; the highest rank of any take)"""
    by_pair, top = {}, -1
    for pair, rank, entry in trace:
        by_pair.setdefault(pair, []).append((rank, entry))
        top = max(top, rank)
    ordered_by_a_high_bit = []
    for pair, takes in by_pair.items():
        high = [(r, e) for r, e in takes if r >= 512]
        if any(r1 < r2 and e1 != e2 and (r1 & 511) > (r2 & 511) for r1, e1 in high for r2, e2 in high):
            ordered_by_a_high_bit.append(pair)
    return ordered_by_a_high_bit, top


@functools.lru_cache(maxsize=None)
def high_rank_case(n_next, which):
    """ranks above 511.  4099 next buckets (no multiple of 4 or 64): 40 rows -- 34 on the buckets below 1024, 6 anywhere; both lots hold rows of 1, 2 and 47 entries --
    and six means: a point, its copy (never to be chosen), the mean of two points, a point at mass 0.5 (targets stay unfinished), two points at mass 1.5, and five
    buckets of 0.2 that stand at the ranks FIVE_RANKS from row 0's only bucket.  8192 (RS_PA_MAX_NEXT): 8 rows of at most 4 entries, three means.
    -> ground, n_draws, rows, means, sel, want [rows][means] (the restatement's distance of every pair), pairs_ordered_by_a_high_bit, highest_take_rank,
    five_lowest_rank (under |i - j| the five buckets stand above rank 512 from every bucket of the 34 rows below 1024; under a random ground no bucket does from all)"""
    rng = np.random.Generator(np.random.PCG64(HIGH_RANK_SEEDS[(n_next, which)]))
    n_draws = 47
    ground = npp.tie_ground(n_next) if which == "ties" else npp.random_ground(rng, n_next, duplicates=3)
    order = npp.order_of(ground)
    if n_next == 8192:
        rows = np.stack([npp.random_row(rng, n_next, n_draws, s) for s in (1, 2, 3, 4, 4, 3, 2, 4)])
    else:
        rows = np.concatenate([npp.random_rows(rng, 34, 1024, n_draws), npp.random_rows(rng, 6, n_next, n_draws)])
    dense = npp.dense(rows, n_next, n_draws)
    a, b, c, d, e = (dense[i] for i in rng.choice(len(rows), size=5, replace=False))
    five = np.zeros(n_next, dtype=F32)
    five[order[int(rows[0, 0] >> 8), list(FIVE_RANKS[n_next])]] = F32(0.2)
    low = np.unique((rows[:34] >> 8)[rows[:34] != 0]).astype(np.int64)             # the buckets of the first lot of rows (8192: of every row)
    five_lowest_rank = int(np.argsort(order[low], axis=1)[:, five > 0].min())      # the lowest rank one of the five buckets has from one of them
    if n_next == 8192:
        means = np.stack([five, a * F32(0.5), ((b.astype(np.float64) + c) / 2).astype(F32)])
    else:
        means = np.stack([a, a, ((b.astype(np.float64) + c) / 2).astype(F32), d * F32(0.5), (c + e) * F32(0.75), five])
    sel = rng.integers(0, len(rows), size=len(rows) + 7).astype(np.uint32)      # with repeats
    trace = []
    k = len(means)
    want = npp.distances(np.repeat(rows, k, axis=0), np.tile(means, (len(rows), 1)), ground, n_draws, order=order, trace=trace).reshape(len(rows), k)
    pairs, top = rank_facts(trace)
    return frozen(ground=ground, n_draws=n_draws, rows=rows, means=means, sel=sel, want=want, pairs_ordered_by_a_high_bit=len(pairs), highest_take_rank=top,
                  five_lowest_rank=five_lowest_rank)


def choice_of(want):
    """the assignment rule on a matrix of distances -> (the first mean with the strictly smallest distance, that distance)"""
    c = np.argmin(want, axis=1)
    return c.astype(np.uint32), want[np.arange(len(want)), c]


# ---- values: small predicts at 65 next buckets --------------------------------------------------------------------------------------------------------------------------
VALUE_NEXT = 65
VALUE_CASES = ["a zero mean", "negative zeros and subnormals", "overflow", "overflow to every mean", "1 draw", "2 draws", "45 draws"]


def _value_means(rng, rows, n_draws):
    dense = npp.dense(rows, VALUE_NEXT, n_draws)
    a, b, c = (dense[i] for i in (5, 11, 23))
    return a, b, c


@functools.lru_cache(maxsize=None)
def value_case(name):
    """-> ground, n_draws, rows, means, want [rows][means]"""
    rng = np.random.Generator(np.random.PCG64(650 + VALUE_CASES.index("overflow" if name.startswith("overflow") else name)))      # both overflow cases: the same rows
    n_next = VALUE_NEXT
    n_draws = {"1 draw": 1, "2 draws": 2, "45 draws": 45}.get(name, 47)
    ground = npp.random_ground(rng, n_next, duplicates=2) if name != "a zero mean" else npp.tie_ground(n_next)
    rows = npp.random_rows(rng, 70, 40 if name.startswith("overflow") else n_next, n_draws)
    a, b, c = _value_means(rng, rows, n_draws)
    two = ((a.astype(np.float64) + b) / 2).astype(F32)
    zero = np.zeros(n_next, dtype=F32)
    if name == "a zero mean":                        # rows 5 and 11 are at +0.0 from means 0 and 1: the zero mean, 2, wins everywhere else; 3 never
        means = np.stack([a, b, zero, zero, two])
    elif name == "negative zeros and subnormals":
        tiny, least = F32(1e-40), F32(np.nextafter(F32(0), F32(1)))
        m0 = np.where(a > 0, a, F32(-0.0)).astype(F32)                       # -0.0 in every cell that is not positive
        m1 = two.copy()
        m1[m1 == 0] = np.where(np.arange((m1 == 0).sum()) % 2 == 0, tiny, least)      # subnormal in every cell that was empty
        m2 = zero.copy()
        m2[[3, 40]] = tiny, least                    # the only mass is subnormal
        m3 = np.where(c > 0, c, np.where(np.arange(n_next) % 3 == 0, F32(-0.0), np.where(np.arange(n_next) % 3 == 1, least, F32(0)))).astype(F32)
        m4 = zero.copy()
        m4[:] = F32(-0.0)                            # nothing positive at all
        m4[17] = least
        means = np.stack([m0, m1, m2, m3, m4])
    elif name.startswith("overflow"):
        # the rows live on the buckets below 40; from there every bucket from 40 on is FLT_MAX away.  The targets of a row add up to 1 within a few ulp, so a total
        # passes FLT_MAX only against a ground entry that is FLT_MAX itself, and then by the roundings of many part takes alone: some rows overflow, most do not
        # (a mean of one far bucket, which every entry takes from once, overflows for no row).  The three far means were picked among `cells` = 2 .. 25 and
        # mass 1, 1.2 and 2 for the rows they overflow for
        ground = ground.copy()
        ground[:40, 40:] = FLT_MAX
        far = []
        for cells, mass in ((21, 1.2), (25, 1.0), (17, 2.0)):
            far.append(zero.copy())
            far[-1][40:40 + cells] = F32(mass / cells)
        means = np.stack(far if name == "overflow to every mean" else [far[0], a, far[1], two, far[2]])
    else:
        means = np.stack([a, a, two, b * F32(0.5), (b + c) * F32(0.75)])
    with np.errstate(over="ignore"):                 # the overflow cases mean to
        want = npp.distance_matrix(rows, means, ground, n_draws)
    return frozen(ground=ground, n_draws=n_draws, rows=rows, means=means, want=want)


def value_premises(name, c):
    """what each value case is there for, from the restatement alone (the GPU file asserts the same)"""
    want = c["want"]
    choice, _ = choice_of(want)
    assert not np.isnan(want).any() and all(npp.well_formed(r, VALUE_NEXT, c["n_draws"]) for r in c["rows"])
    if name == "a zero mean":
        assert not c["means"][2].any() and (_bits(want[:, 2]) == 0).all()                      # +0.0 from every row
        first = (want[:, :2] == 0).any(axis=1)
        assert first.sum() == 2 and (choice[first] < 2).all() and (choice[~first] == 2).all()   # it wins exactly where no earlier mean is at 0 too; its copy never
    elif name == "negative zeros and subnormals":
        m = c["means"]
        tiny = np.finfo(F32).tiny
        assert all(np.signbit(x[x == 0]).any() for x in (m[0], m[3], m[4])) and all(((x > 0) & (x < tiny)).any() for x in m[1:])
        assert (m[2] < tiny).all() and (m[4] < tiny).all() and ((want > 0) & (want < tiny)).any() and len(set(choice.tolist())) >= 4
    elif name == "overflow":
        assert np.isinf(want).any(axis=0).tolist() == [True, False, True, False, True] and not np.isinf(want).all(axis=1).any()
    elif name == "overflow to every mean":
        every, first = np.isinf(want).all(axis=1), np.isinf(want[:, 0])
        assert every.sum() >= 2 and (choice[every] == 0).all() and (first & ~every).any() and (choice[first & ~every] > 0).all()
    else:
        counts = c["rows"] & 255
        assert c["n_draws"] == int(name.split()[0]) and (counts.sum(axis=1) == c["n_draws"]).all() and not (choice == 1).any()


# ---- past the grid caps ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_predict_case():
    """65 536 + 3 data at 2 next buckets: the 48 well-formed rows there are, drawn with replacement -> ground, n_draws, rows, means, want_c, want_d"""
    rng = np.random.Generator(np.random.PCG64(65539))
    n_draws = 47
    kinds = np.stack([npp.pack_row([0], [47]), npp.pack_row([1], [47])] + [npp.pack_row([0, 1], [c, 47 - c]) for c in range(1, 47)])
    ground = np.array([[0, 0.75], [1.5, 0]], dtype=F32)
    means = np.array([[0.25, 0.75], [0.625, 0.375]], dtype=F32)
    rows = kinds[rng.integers(0, len(kinds), size=(1 << 16) + 3)]
    c, d = npp.predict(rows, means, ground, n_draws)
    return frozen(ground=ground, n_draws=n_draws, rows=rows, means=means, want_c=c, want_d=d)


@functools.lru_cache(maxsize=None)
def long_fit_case():
    """262 144 + 5 data drawn with replacement from 2 000 random rows at 3 next buckets, 2 means, 3 iterations of npp.fit
    -> ground, n_draws, rows, means, want_c, want_m, want_d, want_changed"""
    rng = np.random.Generator(np.random.PCG64(262149))
    n_draws = 47
    ground = npp.random_ground(rng, 3)
    pool = npp.random_rows(rng, 2000, 3, n_draws)
    rows = pool[rng.integers(0, len(pool), size=(1 << 18) + 5)]
    means = npp.dense(pool[:2], 3, n_draws)
    c, m, d, changed = npp.fit(rows, means, ground, n_draws, 3)
    return frozen(ground=ground, n_draws=n_draws, rows=rows, means=means, want_c=c, want_m=m, want_d=d, want_changed=changed)
