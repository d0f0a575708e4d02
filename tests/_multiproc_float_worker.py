"""One rank of tests/test_gpu_float_deals_dp.py: a fresh process that shares GPU 0 with its peers and talks to them through tests/libstub_rccl.so (RS_RCCL_LIB).
    python tests/_multiproc_float_worker.py <workdir> <world> <rank> <id-hex>
Reads <workdir>/inputs.npz, trains a float-table DealTrainer data-parallel (rs_deal_trainer_attach_comm + rs_deal_trainer_train: the ranks' per-deal delta items exchanged
inside rs_iterate), checks that rs_iterate_phase refuses the solver, and writes what it ended up with to <workdir>/rank<rank>.npz."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

workdir, world, rank, id_hex = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
assert os.environ.get("RS_RCCL_LIB"), "the worker must run with RS_RCCL_LIB set"
import rustsolver_amd as rs  # noqa: E402
from rustsolver_amd import _lib as L  # noqa: E402
from rustsolver_amd import abstraction as ab  # noqa: E402

lib = L.load()
ident = (C.c_char * L.COMM_ID_BYTES).from_buffer_copy(bytes.fromhex(id_hex).ljust(L.COMM_ID_BYTES, b"\0"))
inp = np.load(os.path.join(workdir, "inputs.npz"))
n, batches, mask, hands = int(inp["n"]), int(inp["batches"]), int(inp["mask"]), inp["hands"]
dtype, mode = int(inp["dtype"]), int(inp["mode"])
n_actions, tree = rs.build_game_tree(rs.three_street_options())
files = [inp["file0"], inp["file1"], None]
card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, files[r]) for r in range(3)]
tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, n, world=world, rank=rank, seed=21, discount_interval=int(inp["discount_interval"]), discount_cap=10**9,
                    dtype=dtype, mode=mode, prune_threshold=None)
comm = C.c_void_p()
L.check(lib.rs_comm_create(tr.infosets._h, ident, rank, world, C.byref(comm)))
tr.attach_comm(comm)
tr.train(batches)
out = {"exchange_bytes": np.array([tr.exchange_bytes()], dtype=np.uint64), "cards": tr.cards(), "iterations": np.array([tr.iterations])}
for nd in tree.action_nodes():
    r, s2 = tr.infosets.download_node(nd.index)
    out["R%d" % nd.index], out["S%d" % nd.index] = r, s2
tr.status()
rc = lib.rs_iterate_phase(lib.rs_deal_trainer_solver(tr._h), 0, 0, None)   # a host driving the phases has nothing it could exchange
out["phase_rc"] = np.array([rc])
tr.attach_comm(None)
lib.rs_comm_destroy(comm)
np.savez(os.path.join(workdir, "rank%d.npz" % rank), **out)
print("rank %d done" % rank)
