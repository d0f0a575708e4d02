"""GPU (-m gpu): data-parallel deal training on float tables (binary32, binary16, RM+) in real processes.  W ranks x n deals must end bit-identical to ONE trainer with W * n
deals per batch: f32 sums do not associate, so the ranks exchange their per-deal delta vectors (items of the deals that touched a node) and every rank sums the union in global
deal order.  The ranks share GPU 0 and talk through tests/libstub_rccl.so, as in tests/test_gpu_multiproc.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from tests.test_gpu_multiproc import build_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_float_ranks(workdir, world, timeout=600):
    """start `world` fresh worker processes (they share GPU 0), wait, return their result files"""
    env = dict(os.environ, RS_RCCL_LIB=build_stub(), HSA_ENABLE_IPC_MODE_LEGACY="0")
    ident = ("/rs_stub_ftest_%d_%s" % (os.getpid(), os.urandom(6).hex())).encode().hex()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_multiproc_float_worker.py"), str(workdir), str(world), str(r), ident], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
    return [np.load(os.path.join(workdir, "rank%d.npz" % r)) for r in range(world)]


@pytest.mark.parametrize("world,dtype,rmplus,combos,n,batches", [(2, "f32", False, 35, 700, 3), (3, "f16", False, 35, 500, 3), (2, "f32", True, 35, 700, 3),
                                                                  (2, "f16", False, 200, 1500, 2)])
def test_float_data_parallel_trainer_equals_one_gpu_with_the_union_batch(world, dtype, rmplus, combos, n, batches, tmp_path):
    """three streets from 2c9dKh, bucket files on flop and turn, the ISOMORPHIC river (35 combos: about 40 K river clusters; 200 combos: more than 100 000), a discount
    tick inside the run.  Cards, iteration counts, every node's regrets and strategy sums: the same bits as one trainer with world * n deals."""
    rng = np.random.Generator(np.random.PCG64(4))
    mask = ab.card_mask("2c9dKh")
    allh = ab.random_range(mask)
    hands = allh[rng.permutation(len(allh))[:combos]]
    n_actions, tree = rs.build_game_tree(rs.three_street_options())
    files = [rng.integers(0, 23, size=1286792, dtype=np.uint32), rng.integers(0, 41, size=13960050, dtype=np.uint32), None]
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, files[r]) for r in range(3)]
    river = card_abs[2].get_size(0)
    assert river > 16384 and (combos < 200 or river >= 100_000), river
    dt = rs.F16 if dtype == "f16" else rs.F32
    mode = rs.UPD_CLAMP_I64 | (rs.UPD_RMPLUS if rmplus else 0)
    di = 2 * world * n - 100
    np.savez(os.path.join(tmp_path, "inputs.npz"), n=n, batches=batches, mask=mask, hands=hands, discount_interval=di, dtype=dt, mode=mode, file0=files[0], file1=files[1])
    single = rs.DealTrainer(tree, card_abs, [hands, hands], mask, world * n, seed=21, discount_interval=di, discount_cap=10**9, dtype=dt, mode=mode, prune_threshold=None)
    single.train(batches)
    ranks = run_float_ranks(tmp_path, world)
    assert (np.concatenate([r["cards"] for r in ranks], axis=1) == single.cards()).all()
    for g, got in enumerate(ranks):
        assert int(got["iterations"][0]) == single.iterations
        assert int(got["phase_rc"][0]) == L.ERR_UNSUPPORTED
        for nd in tree.action_nodes():
            want = single.infosets.download_node(nd.index)
            assert got["R%d" % nd.index].tobytes() == want[0].tobytes() and got["S%d" % nd.index].tobytes() == want[1].tobytes(), "node %d on rank %d" % (nd.index, g)
    single.status()
    # what a rank handed to the collectives per batch, against all-gathering the dense per-deal delta rows of both traversers' nodes
    per_batch = int(ranks[0]["exchange_bytes"][0]) / batches
    dense = world * sum(2 * nd.n_children * n * 4 for nd in tree.action_nodes())
    print("float data-parallel exchange (world %d, %s, %d river clusters): %.3f MB per batch and rank, dense rows %.3f MB" % (world, dtype, river, per_batch / 1e6, dense / 1e6))
    assert 0 < per_batch < dense


def test_float_deal_trainer_with_world_is_accepted_and_prune_still_refused():
    mask = ab.card_mask("4d5dAs3cKs")
    hands = ab.random_range(mask)[::3]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, ab.RIVER)]
    rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, world=2, rank=1, dtype=rs.F16, prune_threshold=None)
    with pytest.raises(rs.RsError):
        rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, world=2, rank=1, dtype=rs.F16, prune_threshold=10**7)
