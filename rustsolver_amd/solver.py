"""Host-side mirror of the reference solver's surface (src/solver) on top of the C ABI.

Names follow the Rust items they stand for so that tests read like tests of the reference:

    Options / default_flop()          options.rs:10-28, :52-81
    build_game_tree(options)          tree_builder.rs:9   -> (n_actions, tree)
    create_infosets(n_actions, tree, card_abs)   infoset.rs:8   -> InfosetTable
    table[an.index][cluster_idx]      cfr.rs:375 (get-infoset) -> Infoset view
    Infoset.get_strategy() / .get_final_strategy()   infoset.rs:83 / :104
    MCCFRTrainer.init(options, ...) / .train(iterations)   cfr.rs:159 / :188

All compute runs in the HIP library; this file only marshals numpy arrays through ctypes.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib as L
from . import locks as node_locks
from . import rake as raked


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Options:
    """options.rs:10-28 (the fields build_game_tree reads)."""

    def __init__(self, stack_sizes=(500, 500), starting_pot=35, n_board_cards=5, bet_sizes=((0.5, 1.0),),
                 raise_sizes=((3.0,),)):
        self.stack_sizes = tuple(stack_sizes)
        self.starting_pot = starting_pot
        self.n_board_cards = n_board_cards  # board_mask.count_ones()
        self.bet_sizes = [list(b) for b in bet_sizes]
        self.raise_sizes = [list(r) for r in raise_sizes]

    def to_c(self):
        o = L.OptionsC()
        o.stack_sizes[0], o.stack_sizes[1] = self.stack_sizes
        o.starting_pot = self.starting_pot
        o.n_board_cards = self.n_board_cards
        o.n_rounds = len(self.bet_sizes)
        for r, (bs, rs) in enumerate(zip(self.bet_sizes, self.raise_sizes)):
            o.n_bet_sizes[r] = len(bs)
            for i, v in enumerate(bs):
                o.bet_sizes[r][i] = v
            o.n_raise_sizes[r] = len(rs)
            for i, v in enumerate(rs):
                o.raise_sizes[r][i] = v
        return o


def default_flop():
    """options::default_flop() (options.rs:52-81): despite the name, a 5-card (river) board."""
    o = L.OptionsC()
    L.check(L.load().rs_options_default(C.byref(o)))
    return Options((o.stack_sizes[0], o.stack_sizes[1]), o.starting_pot, o.n_board_cards,
                   [[o.bet_sizes[r][i] for i in range(o.n_bet_sizes[r])] for r in range(o.n_rounds)],
                   [[o.raise_sizes[r][i] for i in range(o.n_raise_sizes[r])] for r in range(o.n_rounds)])


def three_street_options():
    """options.rs:68-77 commented vectors (minus the 2.0 river bet) from a 3-card board."""
    return Options(n_board_cards=3, bet_sizes=((0.5, 1.0),) * 3, raise_sizes=((3.0,),) * 3)


class GameTree:
    """Tree<GameTreeNode> (tree.rs:14-17), host resident."""

    def __init__(self, handle):
        self._h = handle
        lib = L.load()
        self.n_nodes = lib.rs_tree_n_nodes(handle)
        self.n_action_nodes = lib.rs_tree_n_action_nodes(handle)
        self._nodes = None

    def get_node(self, idx):
        nd = L.TreeNode()
        L.check(L.load().rs_tree_get_node(self._h, idx, C.byref(nd)))
        return nd

    @property
    def nodes(self):
        if self._nodes is None:
            self._nodes = [self.get_node(i) for i in range(self.n_nodes)]
        return self._nodes

    def action_nodes(self):
        """ActionNodes ordered by .index"""
        out = [None] * self.n_action_nodes
        for nd in self.nodes:
            if nd.kind == L.NODE_ACTION:
                out[nd.index] = nd
        return out

    def subtree(self, node):
        """rs_tree_subtree: the subtree below action node `node` as a GameTree of its own (root 0, action indices renumbered in ascending trunk index, round_idx rebased)
        and node_map = int32 [its nodes]: the trunk node id of each of them"""
        h = C.c_void_p()
        node_map = np.full(max(self.n_nodes, 1), -1, dtype=np.int32)
        L.check(L.load().rs_tree_subtree(self._h, int(node), C.byref(h), node_map.ctypes.data_as(C.POINTER(C.c_int32))))
        sub = GameTree(h)
        return sub, node_map[: sub.n_nodes].copy()

    def __del__(self):
        try:
            L.load().rs_tree_destroy(self._h)
        except Exception:
            pass


def build_game_tree(options):
    """tree_builder.rs:9 -> (n_actions, tree)."""
    h = C.c_void_p()
    oc = options.to_c()
    L.check(L.load().rs_tree_build(C.byref(oc), C.byref(h)))
    t = GameTree(h)
    return t.n_action_nodes, t


def tree_from_nodes(nodes):
    arr = (L.TreeNode * len(nodes))(*nodes)
    h = C.c_void_p()
    L.check(L.load().rs_tree_from_nodes(arr, len(nodes), C.byref(h)))
    return GameTree(h)


def _report_request(tree, n_board0, n_hands, nodes):
    """a node report's request: the ids as int32, the blocks' offsets and the output buffer (rs_node_report_size); a bad request raises RsError before anything runs"""
    ids = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
    offsets = np.zeros(max(len(ids), 1), dtype=np.uint64)
    total = int(L.load().rs_node_report_size(tree._h, n_board0, n_hands, _vp(ids), len(ids), _vp(offsets)))
    if total == 0:
        raise L.RsError(L.ERR_INVALID, L.load().rs_last_error().decode("utf-8", "replace"))
    return ids, offsets, np.zeros(total, dtype=np.float64)


def _report_blocks(tree, n_hands, ids, offsets, out):
    """{node: dict(cfv=[A][F][H], value=[F][H], mass=[F][H], own=[F][H])} from a node report's output buffer"""
    res = {}
    ends = list(offsets[1:len(ids)]) + [len(out)]
    for k, node in enumerate(ids):
        A = tree.nodes[int(node)].n_children
        block = out[int(offsets[k]):int(ends[k])].reshape(A + 3, -1, n_hands)
        res[int(node)] = dict(cfv=block[:A], value=block[A], mass=block[A + 1], own=block[A + 2])
    return res


def _report_mode(current, sorted_showdowns):
    return L.BR_AVERAGE | (L.BR_CURRENT if current else 0) | (L.BR_SORTED if sorted_showdowns else 0)


DEALS = {"sequential": L.DEAL_SEQUENTIAL, "joint": L.DEAL_JOINT}


def drop_zero_weights(hands, clusters, weights):
    """A hand of weight exactly 0.0 is by definition a hand that is not in the range (the C ABI takes weights > 0 only): drops those hands, their weights and their
    columns of every cluster table.  hands = (hands0, hands1), clusters[r][p] = [prefixes of round r][n_hands_p], weights = None or (w0, w1), either None.
    -> hands, clusters, weights as contiguous arrays (weights float64, None where None was given) and keep = per player the bool mask of the hands that stay (None where
    no weights were given).  Pure: no device, no library; every other value of a weight (negative, NaN, ...) stays for the library to refuse."""
    hands = [np.ascontiguousarray(h, dtype=np.uint8).reshape(-1, 2) for h in hands]
    if weights is None:
        weights = (None, None)
    if len(weights) != 2:
        raise ValueError("weights is a pair (weights of player 0, of player 1); either may be None")
    w, keep = [None, None], [None, None]
    for p in (0, 1):
        if weights[p] is None:
            continue
        w[p] = np.ascontiguousarray(weights[p], dtype=np.float64).reshape(-1)
        if len(w[p]) != len(hands[p]):
            raise ValueError("one weight per hand: %d weights for the %d hands of player %d" % (len(w[p]), len(hands[p]), p))
        keep[p] = w[p] != 0.0
    cl = []
    for row in clusters:
        out = []
        for p in (0, 1):
            c = np.ascontiguousarray(row[p], dtype=np.uint32)
            if keep[p] is not None and not keep[p].all():
                c = np.ascontiguousarray(c.reshape(-1, len(keep[p]))[:, keep[p]])
            out.append(c)
        cl.append(out)
    for p in (0, 1):
        if keep[p] is not None and not keep[p].all():
            hands[p], w[p] = np.ascontiguousarray(hands[p][keep[p]]), np.ascontiguousarray(w[p][keep[p]])
    return hands, cl, w, keep


def _range_weights(w, deal):
    """rs_range_weights of drop_zero_weights' rows, or None for the call without weights; the rows must outlive the call"""
    deal = DEALS[deal] if isinstance(deal, str) else int(deal)
    if w[0] is None and w[1] is None and deal == L.DEAL_SEQUENTIAL:
        return None
    rw = L.RangeWeights()
    for p in (0, 1):
        rw.w[p] = None if w[p] is None else w[p].ctypes.data
    rw.deal, rw.reserved = deal, 0
    return C.byref(rw)


class _GameArgs:
    """The game as the rs_*_raked entry points take it, from the arguments of InfosetTable.best_response_rounds: normalised at construction (contiguous arrays, the hands
    of weight 0.0 dropped; kept[p] = the mask of player p's hands that stay, or None) and turned into the leading ctypes arguments, tree .. rake, by leading().  The
    object holds what those point at: it outlives the call."""

    def __init__(self, tree, board0, hands0, hands1, clusters, weights, deal, locks, rake):
        self.tree, self.deal, self.locks, self.rake = tree, deal, locks, rake
        self.b = np.ascontiguousarray(board0, dtype=np.uint8)
        self.hands, cl, self.w, self.kept = drop_zero_weights((hands0, hands1), clusters, weights)
        self.cl = [c for row in cl for c in row]
        self.n_hands = (len(self.hands[0]), len(self.hands[1]))

    def leading(self):
        arr = (C.c_void_p * len(self.cl))(*[k.ctypes.data for k in self.cl])
        lk, lk_alive = node_locks.arg(self.tree, len(self.b), self.n_hands, node_locks.drop_columns(self.tree, self.locks, self.kept))   # (the library copies the rows)
        rk, rk_alive = raked.arg(self.rake)
        self._alive = (arr, lk_alive, rk_alive)
        return (self.tree._h, _vp(self.b), len(self.b), _vp(self.hands[0]), self.n_hands[0], _vp(self.hands[1]), self.n_hands[1], arr, len(self.cl) // 2,
                _range_weights(self.w, self.deal), lk, rk)


def _restore_columns(res, keep):
    """a node report's rows with all-0.0 columns for the hands drop_zero_weights took out of the traverser's range"""
    if keep is None or keep.all():
        return res
    for blk in res.values():
        for key, x in blk.items():
            full = np.zeros(x.shape[:-1] + (len(keep),), dtype=x.dtype)
            full[..., keep] = x
            blk[key] = full
    return res


class DeviceBuffer:
    """A device allocation owned through the table's stream (rs_dmalloc / rs_dfree)."""

    def __init__(self, table, nbytes):
        self.table = table
        self.nbytes = nbytes
        p = C.c_void_p()
        L.check(L.load().rs_dmalloc(table._h, nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, table, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(table, arr.nbytes)
        b.upload(arr)
        return b

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        L.check(L.load().rs_h2d(self.table._h, self.ptr, _vp(arr), arr.nbytes))

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        L.check(L.load().rs_d2h(self.table._h, _vp(out), self.ptr, out.nbytes))
        return out

    def zero(self):
        L.check(L.load().rs_dmemset(self.table._h, self.ptr, 0, self.nbytes))

    def free(self):
        if self.ptr:
            L.load().rs_dfree(self.table._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Infoset:
    """View of one info set: `&self.infosets[an.index][cluster_idx]` (cfr.rs:375, infoset.rs:63-67)."""

    def __init__(self, table, node, board, cluster):
        self._t, self._n, self._b, self._c = table, node, board, cluster
        self._a = table.node_desc(node).n_actions
        self._np = np.int32 if table.dtype == L.I32 else np.float32

    def _get(self):
        r = np.empty(self._a, dtype=self._np)
        s = np.empty(self._a, dtype=self._np)
        rc = L.load().rs_get_infoset(self._t._h, self._n, self._b, self._c, _vp(r), _vp(s))
        if rc == L.ERR_OOB:
            raise IndexError(L.load().rs_last_error().decode())
        L.check(rc)
        return r, s

    @property
    def regrets(self):
        return self._get()[0]

    @property
    def strategy_sum(self):
        return self._get()[1]

    def set(self, regrets=None, strategy_sum=None):
        r = None if regrets is None else np.ascontiguousarray(regrets, dtype=self._np)
        s = None if strategy_sum is None else np.ascontiguousarray(strategy_sum, dtype=self._np)
        rc = L.load().rs_set_infoset(self._t._h, self._n, self._b, self._c, None if r is None else _vp(r),
                                     None if s is None else _vp(s))
        if rc == L.ERR_OOB:
            raise IndexError(L.load().rs_last_error().decode())
        L.check(rc)

    def _strategy(self, fn):
        out = np.empty(self._a, dtype=np.float32)
        rc = fn(self._t._h, self._n, self._b, self._c, out.ctypes.data_as(C.POINTER(C.c_float)))
        if rc == L.ERR_OOB:
            raise IndexError(L.load().rs_last_error().decode())
        L.check(rc)
        return out

    def get_strategy(self):
        """infoset.rs:83-102"""
        return self._strategy(L.load().rs_get_strategy)

    def get_final_strategy(self):
        """infoset.rs:104-123"""
        return self._strategy(L.load().rs_get_final_strategy)


class _Row:
    def __init__(self, table, node):
        self._t, self._n = table, node

    def __len__(self):
        d = self._t.node_desc(self._n)
        return d.n_boards * d.n_clusters

    def __getitem__(self, key):
        """row[cluster_idx] (board 0) or row[board, cluster_idx]"""
        d = self._t.node_desc(self._n)
        board, cluster = key if isinstance(key, tuple) else (0, key)
        if not (0 <= cluster < d.n_clusters and 0 <= board < d.n_boards):
            raise IndexError("index out of bounds: the len is %d but the index is %d" % (d.n_clusters, cluster))
        return Infoset(self._t, self._n, board, cluster)


class InfosetTable:
    """`InfosetTable = Vec<Vec<Infoset>>` (infoset.rs:6), resident in HBM."""

    def __init__(self, handle, owned=True):
        self._h = handle
        self._owned = owned   # False: a view of a table that a native object (rs_deal_trainer) owns
        lib = L.load()
        self.n_nodes = lib.rs_table_n_nodes(handle)
        self.dtype = lib.rs_table_dtype(handle)
        self.np_dtype = np.int32 if self.dtype == L.I32 else np.float32
        self._descs = {}
        self._solvers = weakref.WeakSet()   # solvers built on this table must be destroyed before it

    @classmethod
    def create(cls, descs, dtype=L.I32, device=0):
        """descs: list of (n_actions, n_clusters, n_boards, player, round_idx) in ActionNode.index order"""
        arr = (L.NodeDesc * len(descs))()
        for i, (a, c, b, p, r) in enumerate(descs):
            arr[i].n_actions, arr[i].n_clusters, arr[i].n_boards, arr[i].player, arr[i].round_idx = a, c, b, p, r
        h = C.c_void_p()
        L.check(L.load().rs_table_create(arr, len(descs), dtype, device, C.byref(h)))
        return cls(h)

    def __len__(self):
        return self.n_nodes

    def __getitem__(self, node):
        if not 0 <= node < self.n_nodes:
            raise IndexError("index out of bounds: the len is %d but the index is %d" % (self.n_nodes, node))
        return _Row(self, node)

    def node_desc(self, node):
        if node not in self._descs:
            d = L.NodeDesc()
            L.check(L.load().rs_table_node_desc(self._h, node, C.byref(d)))
            self._descs[node] = d
        return self._descs[node]

    def lanes(self, node):
        d = self.node_desc(node)
        return d.n_boards * d.n_clusters

    def pitch(self, node):
        return L.load().rs_table_lane_pitch(self._h, node)

    def tile_lanes(self, node):
        """lanes per tile of the node's block ([pitch / T][A][T]); == pitch(node): the plain [A][pitch] block"""
        return int(L.load().rs_table_tile_lanes(self._h, node))

    @property
    def cells(self):
        return L.load().rs_table_cells(self._h)

    def cell_offset(self, node):
        return L.load().rs_table_cell_offset(self._h, node)

    @property
    def nbytes(self):
        return L.load().rs_table_bytes(self._h)

    # ---- bulk host <-> device -------------------------------------------------------------------
    def upload_node(self, node, regrets=None, strategy_sum=None):
        """arrays [A][n_boards*n_clusters]"""
        r = None if regrets is None else np.ascontiguousarray(regrets, dtype=self.np_dtype)
        s = None if strategy_sum is None else np.ascontiguousarray(strategy_sum, dtype=self.np_dtype)
        L.check(L.load().rs_table_upload_node(self._h, node, None if r is None else _vp(r), None if s is None else _vp(s)))

    def download_node(self, node):
        a, n = self.node_desc(node).n_actions, self.lanes(node)
        r = np.empty((a, n), dtype=self.np_dtype)
        s = np.empty((a, n), dtype=self.np_dtype)
        L.check(L.load().rs_table_download_node(self._h, node, _vp(r), _vp(s)))
        return r, s

    def upload(self, node, board, regrets=None, strategy_sum=None):
        r = None if regrets is None else np.ascontiguousarray(regrets, dtype=self.np_dtype)
        s = None if strategy_sum is None else np.ascontiguousarray(strategy_sum, dtype=self.np_dtype)
        L.check(L.load().rs_table_upload(self._h, node, board, None if r is None else _vp(r), None if s is None else _vp(s)))

    def download(self, node, board):
        d = self.node_desc(node)
        r = np.empty((d.n_actions, d.n_clusters), dtype=self.np_dtype)
        s = np.empty((d.n_actions, d.n_clusters), dtype=self.np_dtype)
        L.check(L.load().rs_table_download(self._h, node, board, _vp(r), _vp(s)))
        return r, s

    def fill_random(self, seed, regret_range=(-10**6, 10**6), ssum_range=(0, 10**6)):
        L.check(L.load().rs_table_fill_random(self._h, seed, regret_range[0], regret_range[1], ssum_range[0], ssum_range[1]))

    # ---- device vectors ----------------------------------------------------------------------------
    def lane_buffer(self, node, rows=1, data=None):
        """float32 device buffer [rows][pitch]; `data` = numpy [rows][lanes] (padded on upload)"""
        pitch = self.pitch(node)
        buf = DeviceBuffer(self, rows * pitch * 4)
        if data is None:
            buf.zero()
        else:
            host = np.zeros((rows, pitch), dtype=np.float32)
            host[:, : self.lanes(node)] = np.asarray(data, dtype=np.float32).reshape(rows, -1)
            buf.upload(host)
        return buf

    def read_lane_buffer(self, buf, node, rows=1):
        pitch = self.pitch(node)
        return buf.download(np.float32, rows * pitch).reshape(rows, pitch)[:, : self.lanes(node)]

    # ---- bulk kernels ---------------------------------------------------------------------------------
    def regret_match_node(self, node):
        """bulk get_strategy (infoset.rs:83-102) -> [A][lanes]"""
        a = self.node_desc(node).n_actions
        out = self.lane_buffer(node, a)
        L.check(L.load().rs_regret_match_node(self._h, node, out.ptr))
        return self.read_lane_buffer(out, node, a)

    def final_strategy_node(self, node):
        a = self.node_desc(node).n_actions
        out = self.lane_buffer(node, a)
        L.check(L.load().rs_final_strategy_node(self._h, node, out.ptr))
        return self.read_lane_buffer(out, node, a)

    def final_strategy_all(self):
        out = DeviceBuffer(self, self.cells * 4)
        L.check(L.load().rs_final_strategy_all(self._h, out.ptr))
        flat = out.download(np.float32, self.cells)
        res = []
        for n in range(self.n_nodes):
            a, p = self.node_desc(n).n_actions, self.pitch(n)
            off = self.cell_offset(n)
            res.append(flat[off: off + a * p].reshape(a, p)[:, : self.lanes(n)])
        return res

    def calc_br(self, tree):
        """MCCFRTrainer::calc_br as coded (cfr.rs:629-638): the pair train() prints at a discount tick"""
        out = np.zeros(2, dtype=np.float32)
        L.check(L.load().rs_calc_br(self._h, tree._h, _vp(out)))
        return out

    def best_response(self, tree, board, hands0, cluster0, hands1, cluster1, mode=L.BR_MAX, current=False):
        """value per deal of each player against the other's average strategy: mode BR_MAX a best response inside the abstraction,
        BR_MAX | BR_REAL a best response in the real game (every hand decides for itself), BR_AVERAGE its own average strategy;
        exploitability = best_response(...).sum() / 2.  current: against (and, BR_AVERAGE, with) the CURRENT strategy, get_strategy of the regrets (BR_CURRENT)"""
        mode |= L.BR_CURRENT if current else 0
        b = np.ascontiguousarray(board, dtype=np.uint8)
        h0 = np.ascontiguousarray(hands0, dtype=np.uint8).reshape(-1, 2)
        h1 = np.ascontiguousarray(hands1, dtype=np.uint8).reshape(-1, 2)
        c0, c1 = np.ascontiguousarray(cluster0, dtype=np.uint32), np.ascontiguousarray(cluster1, dtype=np.uint32)
        if len(b) != 5 or len(c0) != len(h0) or len(c1) != len(h1):
            raise ValueError("board[5], one cluster id per hand")
        out = np.zeros(2, dtype=np.float64)
        L.check(L.load().rs_best_response(self._h, tree._h, _vp(b), _vp(h0), len(h0), _vp(c0), _vp(h1), len(h1), _vp(c1), mode, _vp(out)))
        return out

    def best_response_rounds(self, tree, board0, hands0, hands1, clusters, mode=L.BR_MAX, current=False, weights=None, deal="sequential", locks=None,
                             rake=None):
        """multi-round best response (rs_best_response_rounds): clusters[r][p] = uint32 [prefixes of round r][n_hands_p] dense ids; current: BR_CURRENT.
        weights = (w0, w1), either None: per-hand range weights (rs_best_response_weighted), a weight of 0.0 takes the hand out of the range; deal: "sequential"
        (generate_hand with weighted draws) or "joint" (the product of the two ranges with card removal).
        locks = {tree node id: float64 [A][prefixes of the node's round][hands of the acting player]}: node locks (rs_best_response_locked, rustsolver_amd.locks); the
        columns of hands of weight 0.0 are dropped with the hands.
        rake = (rate, cap): raked pots (rs_best_response_raked, rustsolver_amd.rake, which states the units); the game is then general-sum -- under BR_AVERAGE
        -(out[0] + out[1]) is the rake paid per deal, and a profile's exploitability is rake.exploitability(max_values, avg_values)"""
        mode |= L.BR_CURRENT if current else 0
        g = _GameArgs(tree, board0, hands0, hands1, clusters, weights, deal, locks, rake)
        out = np.zeros(2, dtype=np.float64)
        L.check(L.load().rs_best_response_raked(self._h, *g.leading(), mode, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def node_report(self, tree, board0, hands0, hands1, clusters, traverser, nodes, current=False, sorted_showdowns=True, weights=None, deal="sequential", locks=None,
                    rake=None):
        """per-hand values, reach and mass at the action nodes `nodes` (tree node ids) for one traverser, both players playing the average strategy (current: the current
        one) in the game best_response_rounds measures (rs_node_report).  -> {node: dict(cfv=[A][F][H], value=[F][H], mass=[F][H], own=[F][H])}, float64, F the prefixes of
        the node's round, H the traverser's hands: cfv[a] the action's counterfactual value, value the node's, mass the opponent range the hand faces (cfv / mass = chips
        given that the hand is there), own the traverser's own probability of getting there.  weights, deal: as best_response_rounds (rs_node_report_weighted); a hand of
        weight 0.0 has 0.0 in every row.  locks: as best_response_rounds (rs_node_report_locked); a locked node reports its value by the lock.
        rake: as best_response_rounds (rs_node_report_raked); the tree's terminals are raked, the mass rows are not"""
        g = _GameArgs(tree, board0, hands0, hands1, clusters, weights, deal, locks, rake)
        if traverser not in (0, 1):
            raise L.RsError(L.ERR_INVALID, "rs_node_report: traverser is 0 or 1")
        n_hands = g.n_hands[traverser]
        ids, offsets, out = _report_request(tree, len(g.b), n_hands, nodes)
        L.check(L.load().rs_node_report_raked(self._h, *g.leading(), _report_mode(current, sorted_showdowns), int(traverser), _vp(ids), len(ids), _vp(out), len(out)))
        return _restore_columns(_report_blocks(tree, n_hands, ids, offsets, out), g.kept[traverser])

    def best_response_hands(self, tree, board0, hands0, hands1, clusters, traverser, mode=L.BR_MAX | L.BR_REAL, current=False, weights=None, deal="sequential", locks=None,
                            rake=None):
        """per-hand root values of one traverser's best-response walk (rs_best_response_hands) -> (value, mass), float64 [hands of the traverser]: the root's value row
        and the root's mass row (the opponent range the hand faces) summed over the run-outs.  Every mode of best_response_rounds; value.sum() is its result for the
        traverser, value / mass under BR_MAX the hand's counterfactual best-response value.  weights, deal, locks, rake: as best_response_rounds; a hand of weight 0.0
        has 0.0 in both arrays."""
        mode |= L.BR_CURRENT if current else 0
        g = _GameArgs(tree, board0, hands0, hands1, clusters, weights, deal, locks, rake)
        if traverser not in (0, 1):
            raise L.RsError(L.ERR_INVALID, "rs_best_response_hands: traverser is 0 or 1")
        out = np.zeros((2, g.n_hands[traverser]), dtype=np.float64)
        L.check(L.load().rs_best_response_hands(self._h, *g.leading(), mode, int(traverser), _vp(out[0]), _vp(out[1])))
        kept = g.kept[traverser]
        if kept is None:
            return out[0].copy(), out[1].copy()
        full = np.zeros((2, len(kept)), dtype=np.float64)
        full[:, kept] = out
        return full[0], full[1]

    def update_node(self, node, action_utils, reach=None, scale=100.0, mode=L.UPD_CLAMP_I64):
        """One traverser visit of every lane (cfr.rs:370-466 / :571-623).  Returns node util [lanes]."""
        a = self.node_desc(node).n_actions
        u = self.lane_buffer(node, a, action_utils)
        r = None if reach is None else self.lane_buffer(node, 1, reach)
        out = self.lane_buffer(node, 1)
        L.check(L.load().rs_update_node(self._h, node, u.ptr, None if r is None else r.ptr, scale, mode, out.ptr))
        return self.read_lane_buffer(out, node)[0]

    def node_util(self, node, action_utils):
        a = self.node_desc(node).n_actions
        u = self.lane_buffer(node, a, action_utils)
        out = self.lane_buffer(node, 1)
        L.check(L.load().rs_node_util(self._h, node, u.ptr, out.ptr))
        return self.read_lane_buffer(out, node)[0]

    def child_reach(self, node, reach=None):
        a = self.node_desc(node).n_actions
        r = None if reach is None else self.lane_buffer(node, 1, reach)
        out = self.lane_buffer(node, a)
        L.check(L.load().rs_child_reach(self._h, node, None if r is None else r.ptr, out.ptr))
        return self.read_lane_buffer(out, node, a)

    def get_infosets(self, node, lanes):
        """batched get-infoset: (regrets[A][n], strategy_sum[A][n]) of lanes (= board * n_clusters + cluster) of one node"""
        lanes = np.ascontiguousarray(lanes, dtype=np.uint32)
        a = self.node_desc(node).n_actions
        dt = np.int32 if self.dtype == L.I32 else np.float32
        r, s = np.zeros((a, len(lanes)), dtype=dt), np.zeros((a, len(lanes)), dtype=dt)
        L.check(L.load().rs_get_infosets(self._h, node, lanes.ctypes.data_as(C.c_void_p), len(lanes), r.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))
        return r, s

    def checksum(self):
        """(regrets, strategy_sum) order-independent 64-bit checksums of the whole device arrays (diagnostics)"""
        out = (C.c_uint64 * 2)()
        L.check(L.load().rs_table_checksum(self._h, out))
        return int(out[0]), int(out[1])

    def save(self, path):
        """checkpoint ("RSTB" v1)"""
        L.check(L.load().rs_table_save(self._h, path.encode()))

    @classmethod
    def load(cls, path, device=0):
        h = C.c_void_p()
        L.check(L.load().rs_table_load(path.encode(), device, C.byref(h)))
        return cls(h)

    def discount(self, d):
        """cfr.rs:250-261"""
        L.check(L.load().rs_discount(self._h, float(d)))

    def discount_dcfr(self, d_pos, d_neg, d_sum):
        """rs_discount_dcfr: regrets > 0 times d_pos, the other regrets times d_neg, strategy sums times d_sum (three equal factors = discount(d))"""
        L.check(L.load().rs_discount_dcfr(self._h, float(d_pos), float(d_neg), float(d_sum)))

    def sync(self):
        L.check(L.load().rs_sync(self._h))

    # ---- profiling ------------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        L.check(L.load().rs_profile_enable(self._h, int(on)))

    def profile_mark(self):
        L.check(L.load().rs_profile_mark(self._h))

    def profile_marks(self, cap=65536):
        """durations (ms) between consecutive profile_mark() events on the table's stream; synchronises and forgets the marks"""
        buf, n = (C.c_float * cap)(), C.c_size_t()
        L.check(L.load().rs_profile_marks(self._h, buf, cap, C.byref(n)))
        return [float(buf[i]) for i in range(min(cap, n.value))]

    def profile_reset(self):
        L.check(L.load().rs_profile_reset(self._h))

    def profile_read(self):
        p = L.Profile()
        L.check(L.load().rs_profile_read(self._h, C.byref(p)))
        names = ["update", "node_util", "reach", "chance", "discount", "strategy", "tree"]
        return {n: dict(launches=int(p.launches[i]), ms=float(p.ms[i]), algo_bytes=float(p.algo_bytes[i]))
                for i, n in enumerate(names)}

    def destroy(self):
        if self._h:
            for sv in list(self._solvers):
                sv.destroy()
            if self._owned:
                L.load().rs_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def create_infosets(n_actions, tree, card_abs, n_boards=(1, 1, 1), dtype=L.I32, device=0):
    """infoset.rs:8.  `card_abs[round_idx]` stands for CardAbstraction::get_size: either an int (same for
    both players) or a (size_p0, size_p1) pair.  n_boards[round_idx] is the README's [board] axis."""
    if n_actions != tree.n_action_nodes:
        raise ValueError("n_actions does not match the tree")
    nc = ((C.c_uint32 * L.MAX_PLAYERS) * L.MAX_ROUNDS)()
    nb = (C.c_uint32 * L.MAX_ROUNDS)()
    for r in range(L.MAX_ROUNDS):
        sz = card_abs[r] if r < len(card_abs) else card_abs[-1]
        sz = (sz, sz) if isinstance(sz, int) else tuple(sz)
        nc[r][0], nc[r][1] = sz
        nb[r] = n_boards[r] if r < len(n_boards) else n_boards[-1]
    h = C.c_void_p()
    L.check(L.load().rs_create_infosets(tree._h, C.byref(nc), C.byref(nb), dtype, device, C.byref(h)))
    return InfosetTable(h)


DEFAULT_FORMS = {}   # rs_kernel_forms fields every MCCFRTrainer of this process starts from (the test-suite's fixtures set it; a caller passes forms=)


class MCCFRTrainer:
    """cfr.rs:146-297 for the batched lane model."""

    DISCOUNT_INTERVAL = 100_000   # cfr.rs:193
    DISCOUNT_CAP = 20_000_000     # cfr.rs:194

    def __init__(self, tree, infosets, leaves, scale=10000.0, mode=L.UPD_WRAP_I32, chance_mode=L.CHANCE_ENUM,
                 use_graph=False, leaves_p1=None, fuse_subtrees=None, opp_mode=L.OPP_FULL, sample_seed=0, deals=None, shard=None, prune_deal=None, forms=None, rake=None):
        """leaves: dict tree-node-id -> (LEAF_* kind, DeviceBuffer) for every showdown / all-in terminal.
        deals: None (lane model) or dict (round_idx, player) -> uint32 array of dense cluster ids, one per deal
        (what get_cluster() returned, cfr.rs:361-365): batch-synchronous deal sweeps on the reference-shaped table.
        rake = (rate, cap): raked pots in a deal solver's LEAF_SIGN and uncontested leaves (rs_solver_create_deals_raked, rustsolver_amd.rake); lane solvers take none."""
        if rake is not None and deals is None:
            raise L.RsError(L.ERR_UNSUPPORTED, "MCCFRTrainer: rake goes with deals= (rs_solver_create_deals_raked); lane solvers are unraked")
        self.game_tree, self.infosets = tree, infosets
        self._keep = [leaves, leaves_p1]
        if fuse_subtrees is None:   # tree-specialised kernels need hipRTC at run time; the level plan does not
            fuse_subtrees = bool(L.load().rs_jit_available())
        self.fused = bool(fuse_subtrees)
        self.n_deals = None
        batch = None
        if deals is not None:
            self.n_deals = len(next(iter(deals.values())))
            batch = L.DealBatch()
            batch.n_deals = self.n_deals
            pitch = deal_pitch(self.n_deals)
            for (r, pl), arr in deals.items():
                host = np.zeros(pitch, dtype=np.uint32)
                host[: self.n_deals] = np.asarray(arr, dtype=np.uint32)
                buf = DeviceBuffer.from_numpy(infosets, host)
                self._keep.append(buf)
                batch.d_cluster[r][pl] = buf.ptr
            if prune_deal is not None:   # UPD_PRUNE per deal (cfr.rs:213-221): uint8 flags, one per deal
                host = np.zeros(pitch, dtype=np.uint8)
                host[: self.n_deals] = np.asarray(prune_deal, dtype=np.uint8)
                buf = DeviceBuffer.from_numpy(infosets, host)
                self._keep.append(buf)
                batch.d_prune = buf.ptr
            chance_mode = L.CHANCE_PASS
        arrs = []
        for lv in (leaves, leaves if leaves_p1 is None else leaves_p1):
            arr = (L.LeafDesc * tree.n_nodes)()
            for nid, (kind, buf) in lv.items():
                arr[nid].kind = kind
                arr[nid].d_buf = buf.ptr
            arrs.append(arr)
        sw, sr, srd, sg = shard if shard else (0, 0, 0, 0)   # (world, rank, round, global boards of that round)
        p = L.SolverParams(scale, mode, chance_mode, int(use_graph), int(fuse_subtrees), opp_mode, sample_seed, sw, sr, srd, sg)
        for k, v in dict(DEFAULT_FORMS, **(forms or {})).items():   # rs_kernel_forms by field name: lane_fan, deals_per_thread, shadow, deal_order, delta_rows, direct_rows (0 = the engine's choice)
            setattr(p.forms, k, int(v))
        h = C.c_void_p()
        if batch is None:
            L.check(L.load().rs_solver_create(infosets._h, tree._h, arrs[0], arrs[1], C.byref(p), C.byref(h)))
        elif rake is None:
            L.check(L.load().rs_solver_create_deals(infosets._h, tree._h, C.byref(batch), arrs[0], arrs[1], C.byref(p), C.byref(h)))
        else:
            rk, _alive = raked.arg(rake)
            L.check(L.load().rs_solver_create_deals_raked(infosets._h, tree._h, C.byref(batch), arrs[0], arrs[1], C.byref(p), rk, C.byref(h)))
        self._h = h
        infosets._solvers.add(self)
        self.workspace_bytes = L.load().rs_solver_workspace_bytes(h)

    @classmethod
    def init(cls, options, card_abs, n_boards=(1, 1, 1), leaf_sign=None, dtype=L.I32, device=0, **kw):
        """MCCFRTrainer::init (cfr.rs:159-184): tree, table, plan.  leaf_sign: numpy [lanes of the last round]
        = sign(score0 - score1) per lane, shared by every showdown / all-in terminal of that round."""
        n_actions, tree = build_game_tree(options)
        infosets = create_infosets(n_actions, tree, card_abs, n_boards, dtype, device)
        leaves = {}
        bufs = {}
        for i, nd in enumerate(tree.nodes):
            if nd.kind == L.NODE_TERMINAL and nd.ttype != L.TERM_UNCONTESTED:
                parent = tree.nodes[nd.parent]
                r = parent.round_idx
                if r not in bufs:
                    sign = leaf_sign[r] if isinstance(leaf_sign, dict) else leaf_sign
                    bufs[r] = infosets.lane_buffer(parent.index, 1, sign)
                leaves[i] = (L.LEAF_SIGN, bufs[r])
        return cls(tree, infosets, leaves, **kw)

    def n_launches(self, player):
        return L.load().rs_solver_n_launches(self._h, player)

    def walk_counts(self, player):
        """(deal, round subtree) walks of the last sweep of `player`, per betting round (rs_solver_walk_counts)"""
        return walk_counts(self._h, player)

    @property
    def ordered(self):
        """deal sweeps walk the batch in the order of the traverser's last-round cluster (rs_kernel_forms.deal_order)"""
        return bool(L.load().rs_solver_forms(self._h) & 1)

    @property
    def paired(self):
        """both traversers' sweeps run as one pair launch per iteration (rs_kernel_forms.pair_sweeps)"""
        return bool(L.load().rs_solver_forms(self._h) & 4)

    @property
    def split_pair(self):
        """the pair launch is the split form: two threads of a workgroup share a lane's subtree, cut below its root (rs_solver_forms bit 3)"""
        return bool(L.load().rs_solver_forms(self._h) & 8)

    @property
    def delta_rows(self):
        """deal sweeps store their deltas by list position and sum them in one pass per sweep (rs_kernel_forms.delta_rows)"""
        return bool(L.load().rs_solver_forms(self._h) & 2)

    def iterate(self, player, want_root_util=False):
        """`self.cfr(0, player, hand, 1f32, ..)` for every lane (cfr.rs:217)"""
        root = self.game_tree.nodes[self.game_tree.nodes[0].children[0]]
        if not want_root_util:
            L.check(L.load().rs_iterate(self._h, player, None))
            return None
        if self.n_deals is not None:
            out = deal_buffer(self.infosets, self.n_deals)
            L.check(L.load().rs_iterate(self._h, player, out.ptr))
            return out.download(np.float32, deal_pitch(self.n_deals))[: self.n_deals]
        out = self.infosets.lane_buffer(root.index, 1)
        L.check(L.load().rs_iterate(self._h, player, out.ptr))
        return self.infosets.read_lane_buffer(out, root.index)[0]

    def iterate_phase(self, player, phase, want_root_util=False):
        """sharded sweeps driven by the host: phase 0, <exchange the slots>, phase 1"""
        root = self.game_tree.nodes[self.game_tree.nodes[0].children[0]]
        out = self.infosets.lane_buffer(root.index, 1) if (want_root_util and phase == 1) else None
        L.check(L.load().rs_iterate_phase(self._h, player, phase, None if out is None else out.ptr))
        return None if out is None else self.infosets.read_lane_buffer(out, root.index)[0]

    def exchange_info(self, player):
        """(device pointer, bytes per rank) of the exchange buffer [world][bytes per rank]"""
        buf, n = C.c_void_p(), C.c_size_t()
        L.check(L.load().rs_solver_exchange_info(self._h, player, C.byref(buf), C.byref(n)))
        return buf.value, n.value

    def attach_comm(self, comm_handle):
        L.check(L.load().rs_solver_attach_comm(self._h, comm_handle))

    def training_loop(self, on):
        """rs_solver_training_loop: bracket a hand-written loop of iterate() / table.discount() calls (nothing else may touch the table in between)"""
        L.check(L.load().rs_solver_training_loop(self._h, int(bool(on))))

    def train(self, iterations, discount_interval=None, discount_cap=None):
        """cfr.rs:188"""
        L.check(L.load().rs_train(self._h, iterations, discount_interval or self.DISCOUNT_INTERVAL,
                                  discount_cap or self.DISCOUNT_CAP))
        self.infosets.sync()

    def train_dcfr(self, iterations, alpha=1.5, beta=0.0, gamma=2.0, interval=1, cap=None, t0=0, fused=None):
        """rs_train_dcfr: Discounted CFR over full sweeps -- a tick with dcfr_factors(alpha, beta, gamma, t / interval) after every iteration t <= cap with t % interval == 0,
        t counted from t0.  fused: None = the engine's choice, True / False = apply a pending tick inside the next sweeps' row loads where the solver can / sweep every tick"""
        p = dcfr_params(alpha, beta, gamma, interval, cap, t0, fused)
        L.check(L.load().rs_train_dcfr(self._h, iterations, C.byref(p)))
        self.infosets.sync()

    @property
    def dcfr_fused(self):
        """the last train_dcfr applied its ticks inside the sweeps (rs_solver_dcfr_fused)"""
        return bool(L.load().rs_solver_dcfr_fused(self._h))

    def destroy(self):
        if self._h:
            L.load().rs_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def walk_counts(solver_handle, player):
    import ctypes as C
    out = (C.c_uint64 * 3)()
    L.check(L.load().rs_solver_walk_counts(solver_handle, player, out))
    return [int(x) for x in out]


class DealTrainer:
    """MCCFRTrainer::init + train (cfr.rs:159-297) with the whole deal pipeline on the GPU (rs_deal_trainer): generate_hand,
    get_cluster for every round and player, the showdown comparison and the sampled mccfr sweep, batch after batch."""

    def __init__(self, tree, card_abs, hand_ranges, board_mask, deals_per_batch, seed=0, scale=100.0, mode=L.UPD_CLAMP_I64,
                 opp_mode=L.OPP_SAMPLE, discount_interval=MCCFRTrainer.DISCOUNT_INTERVAL, discount_cap=MCCFRTrainer.DISCOUNT_CAP,
                 use_graph=False, fuse_subtrees=None, device=0, world=1, rank=0, prune_threshold=10_000_000, forms=None, prefetch=None, dtype=L.I32,
                 weights=None, deal="sequential", rake=None):
        """rake = (rate, cap): raked pots (rs_deal_trainer_set_rake, rustsolver_amd.rake): the sweeps train the raked, general-sum game, and best_response(), node_report(),
        train_full_width() and exploitability() measure it.
        weights = (w0, w1), either None: per-hand range weights the deals are drawn with (rs_deal_trainer_set_weights; deal: "sequential" or "joint", as
        InfosetTable.best_response_rounds); best_response(), node_report() and train_full_width() then work on the weighted game.  A weight of exactly 0.0 raises ValueError: drop
        the hand from the range before the card abstractions are built, they are made from the same lists.
        prune_threshold: cfr.rs:190 PRUNE_THRESHOLD (None = never prune).  forms: rs_kernel_forms fields by name, as for MCCFRTrainer.  world / rank: data-parallel training on replicated tables (one process per GPU): this rank deals its share of every global
        batch; attach_comm() makes every rank apply the deltas of the union batch."""
        if fuse_subtrees is None:
            fuse_subtrees = bool(L.load().rs_jit_available())
        self.game_tree, self.card_abs = tree, list(card_abs)
        p = L.DealTrainerParams()
        p.board_mask, p.deals_per_batch, p.seed = board_mask, deals_per_batch, seed
        p.world, p.rank = world, rank
        p.prune_threshold = 2**64 - 1 if prune_threshold is None else prune_threshold
        p.discount_interval, p.discount_cap = discount_interval, discount_cap
        p.table_dtype = dtype   # rs_deal_trainer_params.table_dtype: RS_I32 (the reference), or RS_F32 / RS_F16 (float deal sweeps: prune_threshold=None)
        p.prefetch = L.FORM_DEFAULT if prefetch is None else (L.FORM_ON if prefetch else L.FORM_OFF)   # rs_deal_trainer_params.prefetch: deal the next batch beside this one's sweeps
        p.solver.scale, p.solver.mode, p.solver.chance_mode = scale, mode, L.CHANCE_PASS
        p.solver.use_graph, p.solver.fuse_subtrees = int(use_graph), int(bool(fuse_subtrees))
        p.solver.opp_mode, p.solver.sample_seed = opp_mode, seed
        for k, v in dict(DEFAULT_FORMS, **(forms or {})).items():
            setattr(p.solver.forms, k, int(v))
        h0 = np.ascontiguousarray(hand_ranges[0], dtype=np.uint8).reshape(-1, 2)
        h1 = np.ascontiguousarray(hand_ranges[1], dtype=np.uint8).reshape(-1, 2)
        abs_arr = (C.c_void_p * len(self.card_abs))(*[a._h for a in self.card_abs])
        h = C.c_void_p()
        L.check(L.load().rs_deal_trainer_create(tree._h, abs_arr, len(self.card_abs), _vp(h0), len(h0), _vp(h1), len(h1), C.byref(p), device,
                                                C.byref(h)))
        self._h = h
        self.n_deals = deals_per_batch
        self._n_hands, self._n_board0 = (len(h0), len(h1)), bin(board_mask).count("1")
        self.infosets = InfosetTable(C.c_void_p(L.load().rs_deal_trainer_table(h)), owned=False)
        if weights is not None or deal != "sequential":
            self.set_weights(weights, deal)
        self._rake = None
        if rake is not None:
            self.set_rake(rake)

    def set_rake(self, rake):
        """rs_deal_trainer_set_rake: only before the first batch.  rake = (rate, cap), or None: unraked"""
        rk, _alive = raked.arg(rake)
        L.check(L.load().rs_deal_trainer_set_rake(self._h, rk))
        self._rake = rake if rake is not None and float(rake[0]) > 0.0 and float(rake[1]) > 0.0 else None

    def set_weights(self, weights, deal="sequential"):
        """rs_deal_trainer_set_weights: only before the first batch.  weights=None with deal="sequential": back to unweighted dealing"""
        w = [None, None]
        for p, row in enumerate(weights if weights is not None else (None, None)):
            if row is not None:
                w[p] = np.ascontiguousarray(row, dtype=np.float64).reshape(-1)
                if len(w[p]) != self._n_hands[p]:
                    raise ValueError("one weight per hand: %d weights for the %d hands of player %d" % (len(w[p]), self._n_hands[p], p))
                if (w[p] == 0.0).any():
                    raise ValueError("a hand of weight 0.0 is not in the range: drop it from the hand list (and build the card abstractions from that list)")
        L.check(L.load().rs_deal_trainer_set_weights(self._h, _range_weights(w, deal)))

    def train(self, n_batches):
        L.check(L.load().rs_deal_trainer_train(self._h, n_batches))

    def deal(self):
        L.check(L.load().rs_deal_trainer_deal(self._h))

    def attach_comm(self, comm_handle):
        L.check(L.load().rs_deal_trainer_attach_comm(self._h, comm_handle))

    def iterate_phase(self, player, phase):
        """phase 0: the sweep (deltas accumulated), phase 1: table += delta; between them the ranks' deltas are summed"""
        L.check(L.load().rs_iterate_phase(L.load().rs_deal_trainer_solver(self._h), player, phase, None))

    def walk_counts(self, player):
        """(deal, round subtree) walks of the last batch's sweep of `player`, per betting round"""
        return walk_counts(L.load().rs_deal_trainer_solver(self._h), player)

    def finish_batch(self):
        L.check(L.load().rs_deal_trainer_finish_batch(self._h))

    def exchange_bytes(self):
        """bytes this rank has handed to the collectives of its data-parallel sweeps so far (rs_solver_exchange_bytes)"""
        b, n = C.c_uint64(), C.c_uint64()
        L.check(L.load().rs_solver_exchange_bytes(L.load().rs_deal_trainer_solver(self._h), C.byref(b), C.byref(n)))
        return b.value

    def deltas(self):
        """(regret deltas, strategy_sum deltas) as int32 arrays of rs_table_cells() elements"""
        a, b = C.c_void_p(), C.c_void_p()
        L.check(L.load().rs_table_deltas(self.infosets._h, C.byref(a), C.byref(b)))
        n = self.infosets.cells
        return self._download(a.value, np.int32, n), self._download(b.value, np.int32, n)

    def set_deltas(self, dreg, dssm):
        a, b = C.c_void_p(), C.c_void_p()
        L.check(L.load().rs_table_deltas(self.infosets._h, C.byref(a), C.byref(b)))
        for ptr, arr in ((a.value, dreg), (b.value, dssm)):
            arr = np.ascontiguousarray(arr, dtype=np.int32)
            L.check(L.load().rs_h2d(self.infosets._h, ptr, _vp(arr), arr.nbytes))

    def status(self):
        L.check(L.load().rs_deal_trainer_status(self._h))

    @property
    def iterations(self):
        return int(L.load().rs_deal_trainer_iterations(self._h))

    def set_dcfr(self, alpha=1.5, beta=0.0, gamma=2.0, enable=True):
        """rs_deal_trainer_set_dcfr: the trainer's discount ticks sweep with Discounted CFR's three factors at p = t / discount_interval; enable=False: back to cfr.rs:248-261"""
        if not enable:
            L.check(L.load().rs_deal_trainer_set_dcfr(self._h, None))
            return
        p = dcfr_params(alpha, beta, gamma)
        L.check(L.load().rs_deal_trainer_set_dcfr(self._h, C.byref(p)))

    def set_tick_br(self, enable=True):
        """calc_br at every discount tick, as train() does (cfr.rs:244-246)"""
        L.check(L.load().rs_deal_trainer_set_tick_br(self._h, int(enable)))

    def last_br(self):
        """(pair of the latest tick, iteration count it was taken at)"""
        out, t = np.zeros(2, dtype=np.float32), C.c_uint64()
        L.check(L.load().rs_deal_trainer_last_br(self._h, _vp(out), C.byref(t)))
        return out, int(t.value)

    def calc_br(self):
        out = np.zeros(2, dtype=np.float32)
        L.check(L.load().rs_deal_trainer_calc_br(self._h, _vp(out)))
        return out

    def best_response(self, mode=L.BR_MAX, current=False):
        out = np.zeros(2, dtype=np.float64)
        L.check(L.load().rs_deal_trainer_best_response(self._h, mode | (L.BR_CURRENT if current else 0), _vp(out)))
        return out

    def node_report(self, traverser, nodes, current=False, sorted_showdowns=True):
        """InfosetTable.node_report on the trainer's own tree, ranges, board and cluster tables (rs_deal_trainer_node_report), on the prepared game best_response() keeps"""
        if traverser not in (0, 1):
            raise L.RsError(L.ERR_INVALID, "rs_deal_trainer_node_report: traverser is 0 or 1")
        n_hands = self._n_hands[traverser]
        ids, offsets, out = _report_request(self.game_tree, self._n_board0, n_hands, nodes)
        L.check(L.load().rs_deal_trainer_node_report(self._h, _report_mode(current, sorted_showdowns), int(traverser), _vp(ids), len(ids), _vp(out), len(out)))
        return _report_blocks(self.game_tree, n_hands, ids, offsets, out)

    def train_full_width(self, iterations, rmplus=False, dcfr=None, sorted_showdowns=True):
        """rs_deal_trainer_range_cfr: `iterations` iterations of full-width, chance-enumerated CFR over both ranges on the trainer's own game and table (F32 trainers).
        dcfr: None, True (the paper's 1.5, 0, 2, a tick per iteration) or an rs_dcfr_params from dcfr_params(...).  Returns the two players' values per deal under the
        current profile at the last iteration.  Does not advance iterations()."""
        out = np.zeros(2, dtype=np.float64)
        L.check(L.load().rs_deal_trainer_range_cfr(self._h, int(iterations), C.byref(_range_cfr_params(rmplus, sorted_showdowns)), _dcfr_arg(dcfr),
                                                   out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def br_bytes(self):
        """device bytes held by the best-response objects the trainer keeps between calls"""
        return int(L.load().rs_deal_trainer_br_bytes(self._h))

    def br_release(self):
        L.check(L.load().rs_deal_trainer_br_release(self._h))

    def br_launches(self, sorted_showdowns=True):
        return int(L.load().rs_deal_trainer_br_launches(self._h, int(sorted_showdowns)))

    def exploitability(self, sorted_showdowns=True, real=False, current=False):
        """(BR value of player 0 + BR value of player 1) / 2 against the current average strategies, per deal, in pot units of the leaves.  sorted_showdowns: the leaves by
        rank order (RS_BR_SORTED: O(n log n) per run-out, equal to the pair loop of cfr.rs:323-347 within f64 rounding).  real: the responder plays the real game
        (RS_BR_REAL: an info set is the board seen so far and its own two cards) instead of the abstraction -- never the smaller number, and the one to compare abstractions by.
        A raked trainer's game is general-sum: rake.exploitability(max, avg), from two calls"""
        if self._rake is not None:
            srt = L.BR_SORTED if sorted_showdowns else 0
            return raked.exploitability(self.best_response(L.BR_MAX | srt | (L.BR_REAL if real else 0), current=current), self.best_response(L.BR_AVERAGE | srt, current=current))
        return float(self.best_response(L.BR_MAX | (L.BR_SORTED if sorted_showdowns else 0) | (L.BR_REAL if real else 0), current=current).sum() / 2.0)

    def _download(self, ptr, dtype, count):
        out = np.empty(count, dtype=dtype)
        L.check(L.load().rs_d2h(self.infosets._h, _vp(out), ptr, out.nbytes))
        return out

    def cards(self):
        """the current batch: uint8 [9][n_deals]"""
        pitch = deal_pitch(self.n_deals)
        return self._download(L.load().rs_deal_trainer_cards(self._h), np.uint8, 9 * pitch).reshape(9, pitch)[:, : self.n_deals]

    def signs(self):
        return self._download(L.load().rs_deal_trainer_signs(self._h), np.float32, deal_pitch(self.n_deals))[: self.n_deals]

    def prune_flags(self):
        """uint8 [n_deals]: the live batch's per-deal prune decision (cfr.rs:213-221); all zero before the threshold"""
        ptr = L.load().rs_deal_trainer_prune_flags(self._h)
        return self._download(ptr, np.uint8, deal_pitch(self.n_deals))[: self.n_deals]

    def clusters(self, round_idx, player):
        return self._download(L.load().rs_deal_trainer_clusters(self._h, round_idx, player), np.uint32, deal_pitch(self.n_deals))[: self.n_deals]

    def destroy(self):
        if self._h:
            self.infosets._h = None
            L.load().rs_deal_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _range_cfr_params(rmplus, sorted_showdowns):
    p = L.RangeCfrParams()
    p.mode = L.UPD_RMPLUS if rmplus else 0
    p.sorted = L.FORM_ON if sorted_showdowns else L.FORM_OFF
    return p


def _dcfr_arg(dcfr):
    if dcfr is None or dcfr is False:
        return None
    return C.byref(dcfr_params() if dcfr is True else dcfr)


class RangeCFR:
    """Full-width CFR over hand ranges (rs_range_cfr): chance-enumerated, vector-form sweeps of the game best_response_rounds measures, on an F32 table -- the same
    arguments: board0 (3, 4 or 5 cards), the two ranges, clusters[r][p] = uint32 [prefixes of round r][n_hands_p].  The table and the tree must outlive the object.
    The update rule (plain or regret matching+) is a property of the C object: one is created at construction (`rmplus`), the other on the first call that asks for it.
    locks = {tree node id: float64 [A][prefixes of the node's round][hands of the acting player]}: node locks (rs_range_cfr_create_locked, rustsolver_amd.locks) -- the
    sweeps solve everything around them and leave the locked nodes' table rows alone; set_gadget is refused on such an object.
    rake = (rate, cap): raked pots (rs_range_cfr_create_raked, rustsolver_amd.rake): the sweeps solve the raked, general-sum game; set_gadget is refused on such an object."""

    def __init__(self, table, tree, board0, hands0, hands1, clusters, rmplus=False, sorted_showdowns=True, weights=None, deal="sequential", locks=None, rake=None):
        self.table, self.tree = table, tree
        self._game = _GameArgs(tree, board0, hands0, hands1, clusters, weights, deal, locks, rake)   # weights, deal: as InfosetTable.best_response_rounds
        (self._h0, self._h1), self._keep = self._game.hands, self._game.kept
        self._sorted, self._rmplus, self._hs = bool(sorted_showdowns), bool(rmplus), {}
        self._handle(self._rmplus)

    def _handle(self, rmplus):
        rmplus = self._rmplus if rmplus is None else bool(rmplus)
        if rmplus not in self._hs:
            h = C.c_void_p()
            L.check(L.load().rs_range_cfr_create_raked(self.table._h, *self._game.leading(), C.byref(_range_cfr_params(rmplus, self._sorted)), C.byref(h)))
            self._hs[rmplus] = h
            if getattr(self, "_gadget", None) is not None:      # a handle created after set_gadget starts armed, from zero rows
                self._arm(h, *self._gadget)
        self._last = self._hs[rmplus]
        return self._last

    def iterate(self, traverser, rmplus=None):
        """one traverser's sweep; returns its value per deal under the current profile"""
        v = C.c_double(0.0)
        L.check(L.load().rs_range_cfr_iterate(self._handle(rmplus), int(traverser), C.byref(v)))
        return v.value

    def train(self, iterations, rmplus=None, dcfr=None):
        """`iterations` iterations (traverser 0, then 1); dcfr: None, True (1.5, 0, 2, a tick per iteration) or dcfr_params(...).  Returns the last iteration's two values."""
        out = np.zeros(2, dtype=np.float64)
        L.check(L.load().rs_range_cfr_train(self._handle(rmplus), int(iterations), _dcfr_arg(dcfr), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    GADGET_KINDS = {"resolve": L.GADGET_RESOLVE, "maxmargin": L.GADGET_MAXMARGIN}

    @staticmethod
    def _arm(h, resolver, alt, kind):
        if kind == L.GADGET_RESOLVE:
            L.check(L.load().rs_range_cfr_set_gadget(h, resolver, _vp(alt)))
        else:
            L.check(L.load().rs_range_cfr_set_gadget_kind(h, kind, resolver, _vp(alt)))

    def set_gadget(self, resolver, alt, kind="resolve"):
        """rs_range_cfr_set_gadget: arms the re-solving gadget above the root -- player 1 - resolver chooses per hand between alt[h] (TERMINATE) and the tree (FOLLOW);
        alt = one float64 per hand of that player as handed to the constructor (hands of weight 0 dropped with the range).  Zeroes the gadget rows of every update rule.
        kind="maxmargin" (rs_range_cfr_set_gadget_kind, RS_GADGET_MAXMARGIN): player 1 - resolver picks the HAND on which the resolver improved least instead; row 0 of
        the gadget rows is then the hand-choice row and gadget_margins() returns alt - value / mass per hand after that player's sweep."""
        if kind not in self.GADGET_KINDS:
            raise ValueError("kind is one of %s" % sorted(self.GADGET_KINDS))
        keep = self._keep[1 - int(resolver)] if int(resolver) in (0, 1) else None
        alt = np.ascontiguousarray(alt, dtype=np.float64).reshape(-1)
        if keep is not None and len(alt) == len(keep):
            alt = np.ascontiguousarray(alt[keep])
        n = len((self._h0, self._h1)[1 - int(resolver)]) if int(resolver) in (0, 1) else len(alt)
        if len(alt) != n:
            raise ValueError("one alt per hand of the opponent: %d for %d hands" % (len(alt), n))
        for h in self._hs.values():
            self._arm(h, int(resolver), alt, self.GADGET_KINDS[kind])
        self._gadget = (int(resolver), alt, self.GADGET_KINDS[kind])

    def gadget_margins(self, rmplus=None):
        """rs_range_cfr_gadget_margins -> float64 [n]: alt[h] - F[h] / M[h] of the opponent's last sweep under the max-margin gadget, NaN for a hand that is never dealt
        or faces no mass"""
        h = self._handle(rmplus)
        n = len((self._h0, self._h1)[1 - self._gadget[0]]) if getattr(self, "_gadget", None) is not None else 0
        out = np.zeros(n, dtype=np.float64)
        L.check(L.load().rs_range_cfr_gadget_margins(h, _vp(out)))
        return out

    def gadget(self, rmplus=None):
        """rs_range_cfr_gadget_get -> (regrets, ssum), float32 [2][n]: row 0 TERMINATE, row 1 FOLLOW"""
        h = self._handle(rmplus)
        n = len((self._h0, self._h1)[1 - self._gadget[0]]) if getattr(self, "_gadget", None) is not None else 0
        r, s = np.zeros((2, n), dtype=np.float32), np.zeros((2, n), dtype=np.float32)
        L.check(L.load().rs_range_cfr_gadget_get(h, _vp(r), _vp(s)))
        return r, s

    def set_gadget_rows(self, regrets=None, ssum=None, rmplus=None):
        """rs_range_cfr_gadget_set: float32 [2][n] each, None = leave that array"""
        h = self._handle(rmplus)
        n = len((self._h0, self._h1)[1 - self._gadget[0]]) if getattr(self, "_gadget", None) is not None else 0
        rows = []
        for x in (regrets, ssum):
            if x is not None:
                x = np.ascontiguousarray(x, dtype=np.float32)
                if x.shape != (2, n):
                    raise ValueError("gadget rows are float32 [2][%d]" % n)
            rows.append(x)
        L.check(L.load().rs_range_cfr_gadget_set(h, None if rows[0] is None else _vp(rows[0]), None if rows[1] is None else _vp(rows[1])))

    @property
    def nbytes(self):
        """device bytes held: the prepared game and, from the first sweep on, the workspace"""
        return sum(int(L.load().rs_range_cfr_bytes(h)) for h in self._hs.values())

    def launches(self):
        """kernel launches of the last sweep under the level plan, -1 after a depth-first one"""
        return int(L.load().rs_range_cfr_launches(self._last))

    def destroy(self):
        for h in getattr(self, "_hs", {}).values():
            L.load().rs_range_cfr_destroy(h)
        self._hs = {}

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def deal_pitch(n_deals):
    """per-deal device vectors are padded to a multiple of 64 lanes"""
    return (n_deals + 63) // 64 * 64


def deal_buffer(table, n_deals, data=None):
    """float32 device vector with one value per deal"""
    host = np.zeros(deal_pitch(n_deals), dtype=np.float32)
    if data is not None:
        host[:n_deals] = np.asarray(data, dtype=np.float32)
    return DeviceBuffer.from_numpy(table, host)


def showdown_sign(table, cards):
    """cards: uint8 [9][n_deals] (board x5, P0 hole x2, P1 hole x2) -> (DeviceBuffer of signs, numpy copy)"""
    cards = np.asarray(cards, dtype=np.uint8)
    n = cards.shape[1]
    pitch = deal_pitch(n)
    host = np.zeros((9, pitch), dtype=np.uint8)
    host[:, :n] = cards
    dc = DeviceBuffer.from_numpy(table, host)
    out = deal_buffer(table, n)
    L.check(L.load().rs_showdown_sign(table._h, dc.ptr, n, out.ptr))
    return out, out.download(np.float32, pitch)[:n]


def jit_check_tree(tree, dtype=L.I32, mode=L.UPD_CLAMP_I64, opp_mode=L.OPP_FULL):
    """compile (no GPU needed) every tree-specialised kernel of `tree`; returns the number of distinct kernels"""
    n = C.c_int()
    L.check(L.load().rs_jit_check_tree(tree._h, dtype, mode, opp_mode, C.byref(n)))
    return n.value


def jit_check_pair(tree, dtype=L.I32, mode=L.UPD_CLAMP_I64, opp_mode=L.OPP_FULL):
    """compile (no GPU needed) the pair kernel (both traversers in one walk per lane) of every topmost chance-free subtree of `tree`; returns the number of distinct kernels"""
    n = C.c_int()
    L.check(L.load().rs_jit_check_pair(tree._h, dtype, mode, opp_mode, C.byref(n)))
    return n.value


def jit_check_dcfr(tree, dtype=L.I32, mode=L.UPD_CLAMP_I64):
    """compile (no GPU needed) the discounted variants (train_dcfr, fused) of both traversers' lane kernels of every topmost chance-free subtree of `tree`; returns the number
    of distinct kernels"""
    n = C.c_int()
    L.check(L.load().rs_jit_check_dcfr(tree._h, dtype, mode, C.byref(n)))
    return n.value


def dcfr_params(alpha=1.5, beta=0.0, gamma=2.0, interval=1, cap=None, t0=0, fused=None):
    """an rs_dcfr_params: rs_dcfr_params_default with the given fields"""
    p = L.DcfrParams()
    L.check(L.load().rs_dcfr_params_default(C.byref(p)))
    p.alpha, p.beta, p.gamma, p.interval, p.t0 = float(alpha), float(beta), float(gamma), int(interval), int(t0)
    if cap is not None:
        p.cap = int(cap)
    p.fused = L.FORM_DEFAULT if fused is None else (L.FORM_ON if fused else L.FORM_OFF)
    return p


def dcfr_factors(alpha, beta, gamma, p):
    """rs_dcfr_factors: (pos, neg, sum) of tick number p > 0 as float32"""
    out = (C.c_float * 3)()
    L.check(L.load().rs_dcfr_factors(float(alpha), float(beta), float(gamma), int(p), out))
    return np.array(out[:], dtype=np.float32)


def jit_check_tree_deals(tree, mode=L.UPD_CLAMP_I64, opp_mode=L.OPP_SAMPLE, rake=None):
    """compile (no GPU needed) every deal-batch kernel of `tree`: round subtrees, reach-down and walk, dense / listed, LDS / direct.  rake = (rate, cap): their raked forms
    (rs_jit_check_tree_deals_raked), with the library's check that the unraked sources stay what they are"""
    n = C.c_int()
    if rake is not None:
        rk, _alive = raked.arg(rake)
        L.check(L.load().rs_jit_check_tree_deals_raked(tree._h, mode, opp_mode, rk, C.byref(n)))
        return n.value
    L.check(L.load().rs_jit_check_tree_deals(tree._h, mode, opp_mode, C.byref(n)))
    return n.value


def discount_factor(tc, interval=MCCFRTrainer.DISCOUNT_INTERVAL):
    """cfr.rs:248-249"""
    return np.float32(L.load().rs_discount_factor(tc, interval))


def device_count():
    n = C.c_int()
    rc = L.load().rs_device_count(C.byref(n))
    return n.value if rc == L.OK else 0
