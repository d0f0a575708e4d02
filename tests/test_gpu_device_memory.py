"""GPU (-m gpu): every device buffer of the library has one owner (rs_dev.hpp), charged to the process-wide count rs_device_held_bytes reads.  Each object gives
back exactly what it took when it is destroyed, and a creation that fails half way -- the n-th allocation refused by rs_debug_fail_alloc -- gives back
everything it had taken so far."""
import gc

import numpy as np
import pytest

import rustsolver_amd as rs
from oracle import orc
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from tests.test_gpu_cards import compare_trainer_tables, load_trainer_pair, oracle_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need a real MI355X (there is no CPU fallback)")


def held():
    gc.collect()   # objects of earlier tests that are only waiting for the collector would free their buffers in the middle of a measurement
    return int(L.load().rs_device_held_bytes())


def small_ranges(mask, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    allh = ab.random_range(mask)
    return [allh[rng.permutation(len(allh))[:12]], allh[rng.permutation(len(allh))[:15]]]


def small_trainer(dtype):
    """the three-street game from a flop, small ranges and a small batch, as the float-deal tests build it (with its oracle chain)"""
    mask = ab.card_mask("7h8hQc")
    if dtype == "i32":
        return load_trainer_pair(rs.three_street_options(), orc.options_three_street(), mask, small_ranges(mask, 3), 3, 256, seed=8, interval=2000, cap=10**9)
    return load_trainer_pair(rs.three_street_options(), orc.options_three_street(), mask, small_ranges(mask, 3), 3, 256, seed=8, interval=2000, cap=10**9,
                             odtype=orc.T_F16, scale=0.5, dtype=rs.F16)


def drop_trainer(ctx):
    ctx["tr"].destroy()
    for a in ctx["card_abs"]:
        a.destroy()


def test_every_object_gives_back_what_it_took():
    base = held()

    # a table with a lane solver
    rng = np.random.Generator(np.random.PCG64(1))
    sign = rng.integers(-1, 2, size=3 * 250).astype(np.float32)
    tr = rs.MCCFRTrainer.init(rs.default_flop(), [250], [3], leaf_sign=sign, scale=100.0, mode=rs.UPD_CLAMP_I64)
    tr.iterate(0)
    assert held() > base
    tr.destroy()
    tr.infosets.destroy()
    assert held() == base

    # one-GPU deal trainers on an i32 and on a binary16 table
    for dtype in ("i32", "f16"):
        ctx = small_trainer(dtype)
        ctx["tr"].train(1)
        assert held() > base
        drop_trainer(ctx)
        assert held() == base, dtype

    # a best response through a trainer, its workspace released
    ctx = small_trainer("i32")
    ctx["tr"].train(1)
    ctx["tr"].best_response(L.BR_MAX)
    with_ws = held()
    assert ctx["tr"].br_bytes() > 0
    ctx["tr"].br_release()
    assert held() < with_ws
    drop_trainer(ctx)
    assert held() == base

    # a k-means fit on a table of its own
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    table = rs.create_infosets(n_actions, tree, [4], [1])
    data = rng.random((3000, 20)).astype(np.float32)
    km = ab.Kmeans(table, data)
    km.fit_regular(data[:16].copy(), ab.DIST_L2, 3)
    del km
    table.destroy()
    assert held() == base

    # a solver whose table is destroyed first: it reports no workspace, and holds nothing
    tr = rs.MCCFRTrainer.init(rs.default_flop(), [250], [3], leaf_sign=sign, scale=100.0, mode=rs.UPD_CLAMP_I64)
    tr.iterate(1)
    assert L.load().rs_solver_workspace_bytes(tr._h) == tr.workspace_bytes > 0
    L.load().rs_table_destroy(tr.infosets._h)   # the C handle alone: the Python table would destroy its solvers first
    tr.infosets._h = None
    assert L.load().rs_solver_workspace_bytes(tr._h) == 0
    assert held() == base
    tr.destroy()
    assert held() == base


def test_every_failed_creation_gives_back_what_it_took():
    start = held()
    ctx = small_trainer("i32")
    kw = dict(seed=8, discount_interval=2000, discount_cap=10**9, prune_threshold=None, scale=100.0)
    ctx["tr"].destroy()   # its card abstractions (and whatever device mirrors they made) stay, as part of the baseline
    base = held()
    created = None
    try:
        for n in range(512):
            L.check(L.load().rs_debug_fail_alloc(n))
            try:
                created = rs.DealTrainer(ctx["tree"], ctx["card_abs"], ctx["ranges"], ctx["mask"], ctx["n_deals"], **kw)
            except rs.RsError as e:
                assert e.code in (L.ERR_OOM, L.ERR_HIP), (n, str(e))
                assert held() == base, "allocation %d refused: %d bytes left behind" % (n, held() - base)
                continue
            L.check(L.load().rs_debug_fail_alloc(-1))
            break
        assert created is not None, "creation still fails after 512 granted allocations"
        assert n > 10, "the creation made only %d allocations" % n
        print("a small deal trainer makes %d device allocations" % n)
    finally:
        L.load().rs_debug_fail_alloc(-1)
    ctx["tr"] = created
    created.train(1)
    assert (created.cards() == oracle_batch(ctx)).all()
    compare_trainer_tables(ctx)
    drop_trainer(ctx)
    assert held() == start
