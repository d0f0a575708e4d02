"""Node locks (rs_node_locks): a player's per-hand strategy fixed at chosen action nodes.

A lock of an action node with A actions, in round r, acted by player P is a float64 array [A][prefixes of round r][hands of P]: the probability of action a for hand h
under prefix f (the first r new board cards, in the node report's order) -- the shape of a node report's rows, so a lock can be built from a report.  Every column of a
(prefix, hand) pair that shares no card sums to 1; the entries of pairs that do share a card are never used.  InfosetTable.best_response_rounds, InfosetTable.node_report
and RangeCFR take locks={tree node id: lock}.  Pure numpy here apart from `arg`, which packs the C struct.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def from_clusters(sigma, cluster_table):
    """a per-cluster strategy sigma[A][n_clusters] expanded through the acting player's cluster table of the node's round, [n_prefix][n_hands] dense ids -> the lock
    [A][n_prefix][n_hands] that plays what a table whose node row gives sigma plays: the bridge from a table row to a lock"""
    sigma = np.asarray(sigma)
    ids = np.asarray(cluster_table).astype(np.int64)
    if sigma.ndim != 2 or ids.ndim != 2:
        raise ValueError("sigma is [A][n_clusters], the cluster table [n_prefix][n_hands]")
    return np.ascontiguousarray(sigma.astype(np.float64)[:, ids])


def pure(tree, node, action, n_prefix, n_hands):
    """the lock of `node` that always plays `action`"""
    A = tree.nodes[int(node)].n_children
    if not 0 <= int(action) < A:
        raise ValueError("node %d has %d actions" % (int(node), A))
    lock = np.zeros((A, int(n_prefix), int(n_hands)), dtype=np.float64)
    lock[int(action)] = 1.0
    return lock


def drop_columns(tree, locks, keep):
    """the locks without the columns of the hands drop_zero_weights took out of the acting player's range (keep[p]: the bool mask of player p's hands that stay, or None)"""
    if not locks:
        return locks
    out = {}
    for node, lock in locks.items():
        lock = np.asarray(lock, dtype=np.float64)
        nodes = tree.nodes
        if 0 <= int(node) < len(nodes) and nodes[int(node)].kind == L.NODE_ACTION and nodes[int(node)].player < 2:
            k = keep[nodes[int(node)].player]
            if k is not None and not k.all() and lock.ndim == 3 and lock.shape[-1] == len(k):
                lock = lock[:, :, k]
        out[int(node)] = lock
    return out


def arg(tree, n_board0, n_hands, locks):
    """locks -> (a pointer to rs_node_locks or None, what must stay alive for the call).  A lock of an action node must hold rs_node_lock_size doubles; everything else
    (a node that is no action node, an id twice, entries that are no strategy) is the library's to refuse."""
    if not locks:
        return None, None
    ids = np.ascontiguousarray([int(k) for k in locks], dtype=np.int32)
    rows = []
    for node, lock in locks.items():
        row = np.ascontiguousarray(lock, dtype=np.float64).reshape(-1)
        nodes = tree.nodes
        if 0 <= int(node) < len(nodes) and nodes[int(node)].kind == L.NODE_ACTION and nodes[int(node)].player < 2:
            want = int(L.load().rs_node_lock_size(tree._h, int(n_board0), int(n_hands[nodes[int(node)].player]), int(node)))
            if want and len(row) != want:
                raise ValueError("the lock of node %d holds %d values, not [A][n_prefix][n_hands] = %d" % (int(node), len(row), want))
        rows.append(row)
    ptrs = (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])
    st = L.NodeLocks()
    st.n, st.nodes, st.sigma = len(rows), ids.ctypes.data, C.cast(ptrs, C.c_void_p).value
    return C.byref(st), (st, ids, rows, ptrs)
