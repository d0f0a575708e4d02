"""Host mirror of the card-abstraction plumbing (card_abstraction.rs) on top of the C ABI: bucket files, index_to_cluster,
deterministic dense-id maps, the canonical hand index (rust_poker hand_indexer_s) and the per-round card abstractions."""
import ctypes as C

import numpy as np

from . import _lib as L


def read_cluster_file(path):
    """flat LE u32 per canonical hand index (card_abstraction.rs:227-229)"""
    out, n = C.POINTER(C.c_uint32)(), C.c_size_t()
    L.check(L.load().rs_cluster_file_read(path.encode(), C.byref(out), C.byref(n)))
    try:
        return np.ctypeslib.as_array(out, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.uint32)
    finally:
        L.load().rs_free_u32(out)


def write_cluster_file(path, clusters):
    """gen_abstraction/main.rs:372-380; refuses to overwrite (create_new)"""
    a = np.ascontiguousarray(clusters, dtype=np.uint32)
    L.check(L.load().rs_cluster_file_write(path.encode(), a.ctypes.data_as(C.POINTER(C.c_uint32)), len(a)))


def index_to_cluster(indices, cluster_arr=None):
    """card_abstraction.rs:20-29"""
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    out = np.empty(len(idx), dtype=np.uint64)
    if cluster_arr is None:
        rc = L.load().rs_index_to_cluster(None, 0, idx.ctypes.data_as(C.POINTER(C.c_uint64)), len(idx), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    else:
        arr = np.ascontiguousarray(cluster_arr, dtype=np.uint32)
        rc = L.load().rs_index_to_cluster(arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(arr), idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          len(idx), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc == L.ERR_OOB:
        raise IndexError(L.load().rs_last_error().decode())
    L.check(rc)
    return out


class DenseMap:
    """cluster_map[player] + size[player] of generate_maps (card_abstraction.rs:75-184), first-appearance order"""

    def __init__(self, buckets):
        b = np.ascontiguousarray(buckets, dtype=np.uint64)
        h = C.c_void_p()
        L.check(L.load().rs_dense_map_create(b.ctypes.data_as(C.POINTER(C.c_uint64)), len(b), C.byref(h)))
        self._h = h

    def __len__(self):          # get_size
        return L.load().rs_dense_map_size(self._h)

    def lookup(self, buckets):  # get_cluster's map step; KeyError where Rust would unwrap() a None
        b = np.ascontiguousarray(buckets, dtype=np.uint64)
        out = np.empty(len(b), dtype=np.uint32)
        rc = L.load().rs_dense_map_lookup(self._h, b.ctypes.data_as(C.POINTER(C.c_uint64)), len(b), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc == L.ERR_OOB:
            raise KeyError(L.load().rs_last_error().decode())
        L.check(rc)
        return out

    def keys(self):
        out = np.empty(len(self), dtype=np.uint64)
        L.check(L.load().rs_dense_map_keys(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def __del__(self):
        try:
            L.load().rs_dense_map_destroy(self._h)
        except Exception:
            pass


# ---- cards -------------------------------------------------------------------------------------------------------------------
RANKS = "23456789TJQKA"
SUITS = "shdc"   # only the NUMBER of distinct suits matters to anything in this package (suit isomorphism)


def card(text):
    """'As' -> 4*rank + suit (cfr.rs:592, gen_abstraction/ehs.rs:109: 48, 49 is AA)"""
    return 4 * RANKS.index(text[0].upper()) + SUITS.index(text[1].lower())


def card_mask(text):
    """rust_poker::hand_range::get_card_mask("4d5dAs3cKs") (options.rs:57)"""
    m = 0
    for i in range(0, len(text), 2):
        m |= 1 << card(text[i:i + 2])
    return m


def random_range(board_mask=0):
    """HandRange::from_string("random") after remove_invalid_combos(board_mask) (options.rs:63-64, cfr.rs:161-163):
    every two-card combo that avoids the board, as a uint8 [n][2] array"""
    return np.array([(a, b) for a in range(52) for b in range(a) if not ((board_mask >> a) & 1 or (board_mask >> b) & 1)], dtype=np.uint8)


class HandIndexer:
    """rust_poker::hand_indexer_s: init(rounds, cards_per_round) / size / get_index / get_hand"""

    def __init__(self, cards_per_round):
        cpr = (C.c_uint8 * len(cards_per_round))(*cards_per_round)
        h = C.c_void_p()
        L.check(L.load().rs_hand_indexer_create(len(cards_per_round), cpr, C.byref(h)))
        self._h = h
        self.cards_per_round = tuple(cards_per_round)
        self.rounds = len(cards_per_round)

    def size(self, round_):
        return int(L.load().rs_hand_indexer_size(self._h, round_))

    def n_cards(self, round_):
        return sum(self.cards_per_round[: round_ + 1])

    def get_index(self, cards, round_=None):
        """cards: uint8 [n][n_cards(round)] (or one hand) -> uint64 [n]; round_ defaults to the last, like get_index"""
        r = self.rounds - 1 if round_ is None else round_
        c = np.ascontiguousarray(cards, dtype=np.uint8)
        one = c.ndim == 1
        c = c.reshape(-1, c.shape[-1])
        if c.shape[1] < self.n_cards(r):
            raise ValueError("a hand of round %d has %d cards" % (r, self.n_cards(r)))
        c = np.ascontiguousarray(c[:, : self.n_cards(r)])   # like the reference, extra cards are ignored (card_abstraction.rs:319)
        out = np.empty(len(c), dtype=np.uint64)
        L.check(L.load().rs_hand_index(self._h, r, c.ctypes.data, len(c), out.ctypes.data))
        return int(out[0]) if one else out

    def get_hand(self, round_, indices):
        idx = np.ascontiguousarray(np.atleast_1d(indices), dtype=np.uint64)
        out = np.empty((len(idx), self.n_cards(round_)), dtype=np.uint8)
        rc = L.load().rs_hand_unindex(self._h, round_, idx.ctypes.data, len(idx), out.ctypes.data)
        if rc == L.ERR_OOB:
            raise IndexError(L.load().rs_last_error().decode())
        L.check(rc)
        return out

    def verify(self, cards, expect, round_=None):
        """rs_hand_index_verify: `expect` = the indices ANOTHER indexer (rust_poker's) gave for `cards`; returns (first_bad, got) -- (n, None) when all agree"""
        r = self.rounds - 1 if round_ is None else round_
        c = np.ascontiguousarray(cards, dtype=np.uint8)
        c = np.ascontiguousarray(c.reshape(-1, c.shape[-1])[:, : self.n_cards(r)])
        e = np.ascontiguousarray(expect, dtype=np.uint64)
        if len(e) != len(c):
            raise ValueError("one expected index per hand")
        bad, got = C.c_size_t(), C.c_uint64()
        rc = L.load().rs_hand_index_verify(self._h, r, c.ctypes.data, len(c), e.ctypes.data, C.byref(bad), C.byref(got))
        if rc == L.ERR_MISMATCH:
            return int(bad.value), int(got.value)
        L.check(rc)
        return len(c), None

    def get_index_device(self, table, cards, round_=None):
        """same on the GPU: cards uint8 [n][n_cards] -> uint64 [n] (uploads SoA rows, downloads the indices)"""
        from .solver import DeviceBuffer, deal_pitch
        r = self.rounds - 1 if round_ is None else round_
        c = np.ascontiguousarray(cards, dtype=np.uint8)
        n, nc = c.shape[0], self.n_cards(r)
        pitch = deal_pitch(n)
        host = np.zeros((nc, pitch), dtype=np.uint8)
        host[:, :n] = c[:, :nc].T
        dc = DeviceBuffer.from_numpy(table, host)
        do = DeviceBuffer(table, max(pitch, 1) * 8)
        L.check(L.load().rs_hand_index_device(table._h, self._h, r, dc.ptr, n, do.ptr))
        return do.download(np.uint64, pitch)[:n]

    def __del__(self):
        try:
            L.load().rs_hand_indexer_destroy(self._h)
        except Exception:
            pass


FLOP, TURN, RIVER = 0, 1, 2   # BettingRound (state.rs)


class CardAbstraction:
    """One round's ICardAbstraction (card_abstraction.rs:31-298): `ISOMORPHIC.init` / `EMD.init` / `OCHS.init` are
    `CardAbstraction.init(..., cluster_arr=None | the bucket file)`; get_cluster / get_size as in the reference."""

    def __init__(self, hand_ranges, initial_board_mask, round_, cluster_arr=None):
        h0 = np.ascontiguousarray(hand_ranges[0], dtype=np.uint8).reshape(-1, 2)
        h1 = np.ascontiguousarray(hand_ranges[1], dtype=np.uint8).reshape(-1, 2)
        arr = None if cluster_arr is None else np.ascontiguousarray(cluster_arr, dtype=np.uint32)
        h = C.c_void_p()
        rc = L.load().rs_card_abs_create(round_, h0.ctypes.data, len(h0), h1.ctypes.data, len(h1), initial_board_mask,
                                         None if arr is None else arr.ctypes.data, 0 if arr is None else len(arr), C.byref(h))
        if rc == L.ERR_OOB:
            raise IndexError(L.load().rs_last_error().decode())
        L.check(rc)
        self._h = h
        self.round = round_
        self.n_cards = 5 + round_

    init = classmethod(lambda cls, hand_ranges, board_mask, round_, cluster_arr=None: cls(hand_ranges, board_mask, round_, cluster_arr))

    def get_size(self, player):
        return int(L.load().rs_card_abs_size(self._h, player))

    def index_size(self):
        return int(L.load().rs_card_abs_index_size(self._h))

    def keys(self, player):
        out = np.empty(self.get_size(player), dtype=np.uint64)
        L.check(L.load().rs_card_abs_keys(self._h, player, out.ctypes.data))
        return out

    def get_cluster(self, cards, player):
        """cards: the player's two hole cards then the board (cfr.rs:357-365), one hand or [n][>= 5 + round]"""
        c = np.ascontiguousarray(cards, dtype=np.uint8)
        one = c.ndim == 1
        c = np.ascontiguousarray(c.reshape(-1, c.shape[-1])[:, : self.n_cards])
        out = np.empty(len(c), dtype=np.uint32)
        rc = L.load().rs_card_abs_get_cluster(self._h, c.ctypes.data, len(c), player, out.ctypes.data)
        if rc == L.ERR_OOB:
            raise KeyError(L.load().rs_last_error().decode())
        L.check(rc)
        return int(out[0]) if one else out

    def get_clusters_device(self, table, cards9):
        """cards9: uint8 [9][n] deal matrix (board x5, P0 x2, P1 x2) -> (ids of player 0, ids of player 1), computed on the GPU"""
        from .solver import DeviceBuffer, deal_pitch
        c = np.ascontiguousarray(cards9, dtype=np.uint8)
        n = c.shape[1]
        pitch = deal_pitch(n)
        host = np.zeros((9, pitch), dtype=np.uint8)
        host[:, :n] = c
        dc = DeviceBuffer.from_numpy(table, host)
        d0, d1 = DeviceBuffer(table, max(pitch, 1) * 4), DeviceBuffer(table, max(pitch, 1) * 4)
        L.check(L.load().rs_card_abs_clusters_device(self._h, table._h, dc.ptr, n, d0.ptr, d1.ptr))
        rc = L.load().rs_card_abs_status(self._h, table._h)
        if rc == L.ERR_OOB:
            raise KeyError(L.load().rs_last_error().decode())
        L.check(rc)
        return d0.download(np.uint32, pitch)[:n], d1.download(np.uint32, pitch)[:n]

    def destroy(self):
        if self._h:
            L.load().rs_card_abs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DealWeights:
    """rs_deal_weights: the integer quanta of a pair of weighted ranges (and, with a table, their prefix sums on its device).  weights = (w0, w1), either None = 1.0 for
    every hand; n_hands = (n0, n1)"""

    def __init__(self, table, weights, n_hands, deal="sequential"):
        from .solver import DEALS
        w = [None if row is None else np.ascontiguousarray(row, dtype=np.float64).reshape(-1) for row in weights]
        for p in (0, 1):
            if w[p] is not None and len(w[p]) != n_hands[p]:
                raise ValueError("one weight per hand: %d weights for the %d hands of player %d" % (len(w[p]), n_hands[p], p))
        h = C.c_void_p()
        L.check(L.load().rs_deal_weights_create(None if table is None else table._h, None if w[0] is None else w[0].ctypes.data, n_hands[0],
                                                None if w[1] is None else w[1].ctypes.data, n_hands[1], DEALS[deal] if isinstance(deal, str) else int(deal), C.byref(h)))
        self._h, self.n_hands = h, tuple(int(n) for n in n_hands)

    def quanta(self, player):
        q = np.zeros(self.n_hands[player], dtype=np.uint64)
        L.check(L.load().rs_deal_weights_quanta(self._h, player, q.ctypes.data))
        return q

    def destroy(self):
        if self._h:
            L.load().rs_deal_weights_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def deal_quanta(weights):
    """the host quantisation of one row of range weights -> uint64 [n]: q[i] = floor(w[i] / max(w) * 2^32 + 0.5) (rs_deal_weights_create states the refusals)"""
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    dw = DealWeights(None, (w, None), (len(w), 1))
    try:
        return dw.quanta(0)
    finally:
        dw.destroy()


def sample_deals(table, seed, first_deal, board_mask, hand_ranges, n_deals, weights=None, deal="sequential"):
    """generate_hand (cfr.rs:100-143) for n_deals deals on the GPU -> uint8 [9][n_deals].  weights = (w0, w1), either None: rs_deals_sample_weighted under `deal`
    ("sequential" or "joint"); weights=None with deal="sequential" is rs_deals_sample"""
    from .solver import DeviceBuffer, deal_pitch
    h0 = np.ascontiguousarray(hand_ranges[0], dtype=np.uint8).reshape(-1, 2)
    h1 = np.ascontiguousarray(hand_ranges[1], dtype=np.uint8).reshape(-1, 2)
    d0, d1 = DeviceBuffer.from_numpy(table, h0), DeviceBuffer.from_numpy(table, h1)
    pitch = deal_pitch(n_deals)
    dc = DeviceBuffer(table, 9 * max(pitch, 1))
    dc.zero()
    de = DeviceBuffer(table, 4)
    de.zero()
    if weights is None and deal == "sequential":
        L.check(L.load().rs_deals_sample(table._h, seed, first_deal, board_mask, d0.ptr, len(h0), d1.ptr, len(h1), n_deals, dc.ptr, de.ptr))
    else:
        dw = weights if isinstance(weights, DealWeights) else DealWeights(table, weights if weights is not None else (None, None), (len(h0), len(h1)), deal)
        try:
            L.check(L.load().rs_deals_sample_weighted(table._h, seed, first_deal, board_mask, d0.ptr, len(h0), d1.ptr, len(h1), dw._h, n_deals, dc.ptr, de.ptr))
            table.sync()   # the launch reads dw's rows
        finally:
            if dw is not weights:
                dw.destroy()
    err = int(de.download(np.uint32, 1)[0])
    if err:
        raise RuntimeError("generate_hand: no valid combo for some deal (error word %d)" % err)
    return dc.download(np.uint8, 9 * pitch).reshape(9, pitch)[:, :n_deals]


# ---- abstraction generator's distance sweep (gen_abstraction/kmeans.rs, emd.rs) -----------------------------------------------------
DIST_EMD, DIST_L2 = L.DIST_EMD, L.DIST_L2


def histogram_distance(p, q, dist=DIST_EMD):
    """emd::emd_1d (emd.rs:53-113) or kmeans::l2_dist (kmeans.rs:622-630) of two histograms, on the host"""
    a, b = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("two histograms of the same length")
    out = C.c_float()
    L.check(L.load().rs_histogram_distance(dist, a.ctypes.data, b.ctypes.data, len(a), C.byref(out)))
    return np.float32(out.value)


# ---- exact EHS and the round histograms the k-means clusters (rs_ehs.hip; semantics in include/rustsolver_amd.h) -----------------------------------
EHS_MAX_BINS = L.EHS_MAX_BINS


def ehs_bin(value, n_bins):
    """get_bin (gen_abstraction/main.rs:58-70) literally, on the host"""
    return L.check_nonneg(L.load().rs_ehs_bin(float(np.float32(value)), n_bins))


def _card_rows(table, cards, n_cards):
    """uint8 [n][n_cards] -> the SoA rows [n_cards][pitch] on the device"""
    from .solver import DeviceBuffer, deal_pitch
    c = np.ascontiguousarray(cards, dtype=np.uint8).reshape(-1, n_cards)
    pitch = deal_pitch(len(c))
    host = np.zeros((n_cards, max(pitch, 1)), dtype=np.uint8)
    host[:, :len(c)] = c.T
    return DeviceBuffer.from_numpy(table, host), len(c)


def ehs(table, cards):
    """Exact expected hand strength against a random hand (EHS::get_ehs by enumeration): cards uint8 [n][5, 6 or 7] = two hole cards then the
    board (or one hand) -> float32 [n].  A hand with a repeated card or a byte that is no card raises RsError (ERR_INVALID)."""
    from .solver import DeviceBuffer
    c = np.ascontiguousarray(cards, dtype=np.uint8)
    one = c.ndim == 1
    c = c.reshape(-1, c.shape[-1])
    dc, n = _card_rows(table, c, c.shape[1])
    do = DeviceBuffer(table, max(n, 1) * 4)
    L.check(L.load().rs_ehs(table._h, dc.ptr, c.shape[1], n, do.ptr))
    out = do.download(np.float32, n)
    return out[0] if one else out


class RoundHistograms:
    """The device buffer `round_histograms` fills: float32 [rows][n_bins], one row per canonical hand index of the round"""

    def __init__(self, table, rows, n_bins, buffer):
        self.table, self.rows, self.n_bins, self.buffer = table, rows, n_bins, buffer

    @property
    def ptr(self):
        return self.buffer.ptr

    @property
    def nbytes(self):
        return self.buffer.nbytes

    def download(self, first=0, count=None):
        """rows first .. first + count (default: all) as float32 [count][n_bins] on the host -- small cases, or in slices: the turn round at 30 bins is 1.7 GB"""
        count = self.rows - first if count is None else count
        if first < 0 or count < 0 or first + count > self.rows:
            raise IndexError("rows %d .. %d of %d" % (first, first + count, self.rows))
        out = np.empty((count, self.n_bins), dtype=np.float32)
        if out.size:
            L.check(L.load().rs_d2h(self.table._h, out.ctypes.data, self.ptr + first * self.n_bins * 4, out.nbytes))
        return out

    def gather(self, indices):
        """the rows `indices` (a few: candidate centers), one copy each"""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        return np.concatenate([self.download(int(i), 1) for i in idx]) if len(idx) else np.zeros((0, self.n_bins), dtype=np.float32)


def round_histograms(table, indexer, n_bins, boards=None, out=None):
    """The EHS histograms of a flop (indexer [2, 3]) or turn (indexer [2, 4]) round on the device.  boards: uint8 [n][3 or 4], or None = every board of the
    round.  Rows whose hands lie on no listed board are left as they were (a buffer made here starts at zero).  -> RoundHistograms"""
    from .solver import DeviceBuffer
    if out is None:
        rows = indexer.size(indexer.rounds - 1)
        out = RoundHistograms(table, rows, n_bins, DeviceBuffer(table, max(rows * max(n_bins, 0), 1) * 4))
        out.buffer.zero()
    db, n = None, 0
    if boards is not None:
        b = np.ascontiguousarray(boards, dtype=np.uint8)
        if b.size == 0:
            return out
        b = b.reshape(-1, b.shape[-1])
        if b.shape[1] != indexer.n_cards(indexer.rounds - 1) - 2:
            raise ValueError("a board of this round has %d cards" % (indexer.n_cards(indexer.rounds - 1) - 2))
        db, n = _card_rows(table, b, b.shape[1])
    L.check(L.load().rs_ehs_round_histograms(table._h, indexer._h, n_bins, db.ptr if db else None, n, out.ptr))
    return out


# ---- exact OCHS features and the opponent ranges they are measured against (rs_ochs.hip; semantics in include/rustsolver_amd.h) -----------------------------
OCHS_MAX_CLUSTERS, OCHS_NO_CLUSTER = L.OCHS_MAX_CLUSTERS, L.OCHS_NO_CLUSTER
PREFLOP_ROW_SUM = 21187600   # C(50, 5) boards of a hole pair, each met on C(5, 3) flops


def hole_pair_index(c0, c1):
    """the row of a hole pair in pair_cluster and in the preflop counts: c1 (c1 - 1) / 2 + c0 for c0 < c1 (either order given)"""
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    return hi * (hi - 1) // 2 + lo


def _hole_pairs():
    """uint8 [1326][2]: the cards of every hole pair in hole_pair_index order"""
    return np.array([(c0, c1) for c1 in range(52) for c0 in range(c1)], dtype=np.uint8)


def _board_rows(table, boards, n_cards):
    b = np.ascontiguousarray(boards, dtype=np.uint8)
    b = b.reshape(-1, b.shape[-1])
    if b.shape[1] != n_cards:
        raise ValueError("a board of this round has %d cards" % n_cards)
    return _card_rows(table, b, n_cards)


def ochs_features(table, indexer, pair_cluster, n_clusters, normalize=True, boards=None, out=None):
    """The OCHS feature vectors of a flop ([2, 3]), turn ([2, 4]) or river ([2, 5]) round on the device: one row of n_clusters equities per canonical hand index.
    pair_cluster: uint8 [1326] by hole_pair_index, a cluster id or OCHS_NO_CLUSTER.  boards: uint8 [n][3, 4 or 5], or None = the whole round (every row is
    written).  Rows whose hands lie on no listed board are left as they were (a buffer made here starts at zero).  -> RoundHistograms (rows x n_clusters), which
    Kmeans.from_device takes as it is"""
    from .solver import DeviceBuffer
    pc = np.ascontiguousarray(pair_cluster, dtype=np.uint8).reshape(-1)
    if len(pc) != 1326:
        raise ValueError("pair_cluster has one entry per hole pair: 1326")
    if out is None:
        rows = indexer.size(indexer.rounds - 1)
        out = RoundHistograms(table, rows, n_clusters, DeviceBuffer(table, max(rows * max(n_clusters, 0), 1) * 4))
        out.buffer.zero()
    db, n = None, 0
    if boards is not None:
        if np.asarray(boards).size == 0:
            return out
        db, n = _board_rows(table, boards, indexer.n_cards(indexer.rounds - 1) - 2)
    L.check(L.load().rs_ochs_round_features(table._h, indexer._h, pc.ctypes.data, n_clusters, int(bool(normalize)), db.ptr if db else None, n, out.ptr))
    return out


def preflop_counts(table, n_bins, boards=None):
    """For every hole pair (hole_pair_index order) the river-EHS bin counts of its completions, summed over the listed flops (uint8 [n][3]) or over all 22 100:
    -> uint32 [1326][n_bins].  Over all flops every row sums to PREFLOP_ROW_SUM"""
    from .solver import DeviceBuffer
    do = DeviceBuffer(table, 1326 * max(n_bins, 1) * 4)
    db, n = None, 0
    if boards is not None:
        if np.asarray(boards).size == 0:
            return np.zeros((1326, n_bins), dtype=np.uint32)
        db, n = _board_rows(table, boards, 3)
    L.check(L.load().rs_ehs_preflop_counts(table._h, n_bins, db.ptr if db else None, n, do.ptr))
    return do.download(np.uint32, 1326 * n_bins).reshape(1326, n_bins)


def _preflop_classes():
    """-> (HandIndexer([2]) row of every hole pair [1326], pairs per row [169])"""
    rows = HandIndexer([2]).get_index(_hole_pairs()).astype(np.int64)
    return rows, np.bincount(rows, minlength=169)


def _class_histograms(counts):
    rows, n_pairs = _preflop_classes()
    sums = np.zeros((169, counts.shape[1]), dtype=np.int64)
    np.add.at(sums, rows, counts.astype(np.int64))
    return (sums.astype(np.float64) / (n_pairs * PREFLOP_ROW_SUM).astype(np.float64)[:, None]).astype(np.float32)


def preflop_histograms(table, n_bins):
    """The EHS histograms of the 169 preflop classes (generate_histograms(.., 0, n_bins) by enumeration): float32 [169][n_bins]; row r of HandIndexer([2]) is
    f32(f64(sum of its pairs' counts) / f64(n_pairs x PREFLOP_ROW_SUM))"""
    return _class_histograms(preflop_counts(table, n_bins))


def opponent_clusters(table, n_clusters, n_bins=35, seed=1):
    """generate_opponent_clusters (gen_abstraction/main.rs:161-236): the 169 preflop classes clustered into n_clusters opponent ranges by their EHS histograms --
    kmeans++ (init_pp: a uniform first center, then draws weighted by update_min_dists) with EMD, fit_regular, predict -- and expanded to pair_cluster uint8 [1326].
    The draws come from numpy's Generator(PCG64(seed)) where the reference uses thread_rng.
    A deviation: the reference orders the ranges by an all-in equity it samples (calc_equity(range vs random, 10000)); here range 0 .. n_clusters - 1 ascend by the
    combo-weighted mean bin of their members' summed counts (f64 from integers), ties to the range with the lowest member row; a range without members sorts last."""
    if not 1 <= n_clusters <= OCHS_MAX_CLUSTERS:
        raise ValueError("n_clusters must be 1..OCHS_MAX_CLUSTERS")
    counts = preflop_counts(table, n_bins).astype(np.int64)
    hist = _class_histograms(counts)
    rng = np.random.Generator(np.random.PCG64(seed))
    km = Kmeans(table, hist)
    centers = [hist[int(rng.integers(0, len(hist)))]]
    min_dists = np.full(len(hist), np.finfo(np.float32).max, dtype=np.float32)
    for _ in range(1, n_clusters):
        min_dists = km.update_min_dists(min_dists, centers[-1])
        w = min_dists.astype(np.float64)
        if not w.sum() > 0:
            raise ValueError("fewer distinct preflop histograms than opponent clusters")
        centers.append(hist[int(rng.choice(len(hist), p=w / w.sum()))])
    _, centers, _, _ = km.fit_regular(np.stack(centers))
    clusters, _ = km.predict(centers)
    rows, _ = _preflop_classes()
    of_pair = clusters.astype(np.int64)[rows]
    keys = []
    for c in range(n_clusters):
        total = counts[of_pair == c].sum(axis=0)
        members = np.nonzero(clusters == c)[0]
        mean = float(np.dot(np.arange(n_bins, dtype=np.float64), total.astype(np.float64)) / np.float64(total.sum())) if len(members) else np.inf
        keys.append((mean, int(members[0]) if len(members) else 169 + c, c))
    rank = np.empty(n_clusters, dtype=np.uint8)
    for new, (_, _, c) in enumerate(sorted(keys)):
        rank[c] = new
    return rank[of_pair]


class Kmeans:
    """The distance sweeps of gen_abstraction/kmeans.rs on the GPU: `predict` (kmeans.rs:173-211) and the kmeans++ `update_min_dists`
    (kmeans.rs:603-619).  The dataset stays resident on the device between calls."""

    def __init__(self, table, dataset):
        from .solver import DeviceBuffer
        d = np.ascontiguousarray(dataset, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError("dataset is [n][n_bins]")
        self.table, self.n, self.n_bins = table, d.shape[0], d.shape[1]
        self._data = DeviceBuffer.from_numpy(table, d) if d.size else None
        self._DeviceBuffer = DeviceBuffer

    @classmethod
    def from_device(cls, table, buffer, n, n_bins):
        """the same over a dataset that is on the device already: `buffer` (a DeviceBuffer or RoundHistograms, kept alive by this object) holds float32 [n][n_bins]"""
        from .solver import DeviceBuffer
        if n < 0 or n_bins < 1 or n * n_bins * 4 > buffer.nbytes:
            raise ValueError("the buffer holds fewer than n x n_bins floats")
        self = cls.__new__(cls)
        self.table, self.n, self.n_bins = table, n, n_bins
        self._data = buffer if n else None
        self._DeviceBuffer = DeviceBuffer
        return self

    def predict(self, centers, dist=DIST_EMD):
        """-> (clusters uint32 [n], distance to the chosen center float32 [n])"""
        c = np.ascontiguousarray(centers, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] != self.n_bins:
            raise ValueError("centers are [k][n_bins]")
        dc = self._DeviceBuffer(self.table, max(self.n, 1) * 4)
        dm = self._DeviceBuffer(self.table, max(self.n, 1) * 4)
        L.check(L.load().rs_kmeans_predict(self.table._h, dist, self._data.ptr if self._data else None, self.n, c.ctypes.data, len(c), self.n_bins,
                                           dc.ptr, dm.ptr))
        return dc.download(np.uint32, self.n), dm.download(np.float32, self.n)

    def update_min_dists(self, min_dists, new_center, dist=DIST_EMD):
        m = np.ascontiguousarray(min_dists, dtype=np.float32)
        c = np.ascontiguousarray(new_center, dtype=np.float32)
        dm = self._DeviceBuffer.from_numpy(self.table, m) if self.n else None
        L.check(L.load().rs_update_min_dists(self.table._h, dist, dm.ptr if dm else None, self._data.ptr if self._data else None, self.n, c.ctypes.data,
                                             self.n_bins))
        return dm.download(np.float32, self.n) if self.n else m

    # ---- the training loops (kmeans.rs:213-601) ------------------------------------------------------------------------------------------
    def init_s(self, centers, s, dist=DIST_EMD):
        """Kmeans::init_s (kmeans.rs:267-285): returns the updated s (float32 [k]); s is in/out in the reference"""
        c = np.ascontiguousarray(centers, dtype=np.float32)
        out = np.array(s, dtype=np.float32, order="C")
        L.check(L.load().rs_kmeans_init_s(self.table._h, dist, c.ctypes.data, len(c), self.n_bins, out.ctypes.data))
        return out

    def pick_restart(self, candidates, dist=DIST_EMD):
        """Kmeans::init_random's scoring (kmeans.rs:124-156): candidates [n_restarts][k][n_bins] -> (index of the most spread set, mean pairwise distances)"""
        import ctypes as C
        c = np.ascontiguousarray(candidates, dtype=np.float32)
        cd = np.zeros(c.shape[0], dtype=np.float32)
        best = C.c_int()
        L.check(L.load().rs_kmeans_pick_restart(self.table._h, dist, c.ctypes.data, c.shape[0], c.shape[1], c.shape[2], cd.ctypes.data, C.byref(best)))
        return best.value, cd

    def reassign(self, centers, s, clusters, bounds, dist=DIST_EMD, order=None):
        """Kmeans::reassign_clusters (kmeans.rs:287-334) -> (clusters uint32 [m], bounds float32 [m][2]); m = len(clusters) items, item i = dataset[order[i]]"""
        c = np.ascontiguousarray(centers, dtype=np.float32)
        s_ = np.ascontiguousarray(s, dtype=np.float32)
        dc = self._DeviceBuffer.from_numpy(self.table, np.ascontiguousarray(clusters, dtype=np.uint32))
        db = self._DeviceBuffer.from_numpy(self.table, np.ascontiguousarray(bounds, dtype=np.float32))
        do = None if order is None else self._DeviceBuffer.from_numpy(self.table, np.ascontiguousarray(order, dtype=np.uint32))
        m = len(clusters)
        L.check(L.load().rs_kmeans_reassign(self.table._h, dist, self._data.ptr, do.ptr if do else None, m, c.ctypes.data, len(c), self.n_bins, s_.ctypes.data,
                                            dc.ptr, db.ptr))
        return dc.download(np.uint32, m), db.download(np.float32, 2 * m).reshape(m, 2)

    def fit_regular(self, centers, dist=DIST_EMD, iterations=10):
        """Kmeans::fit_regular (kmeans.rs:497-600) -> (clusters uint32 [n], new centers [k][n_bins], bounds [n][2], inertia)"""
        import ctypes as C
        c = np.array(centers, dtype=np.float32, order="C")
        dc = self._DeviceBuffer(self.table, self.n * 4)
        db = self._DeviceBuffer(self.table, self.n * 8)
        inertia = C.c_float()
        L.check(L.load().rs_kmeans_fit_regular(self.table._h, dist, self._data.ptr, self.n, c.ctypes.data, len(c), self.n_bins, iterations, dc.ptr, db.ptr,
                                               C.byref(inertia)))
        return dc.download(np.uint32, self.n), c, db.download(np.float32, 2 * self.n).reshape(self.n, 2), np.float32(inertia.value)

    def fit_growbatch(self, order, batch, centers, dist=DIST_EMD):
        """Kmeans::fit_growbatch as coded (kmeans.rs:336-495) -> (clusters [batch], new centers, bounds [batch][2], stats = (p, inertia))"""
        c = np.array(centers, dtype=np.float32, order="C")
        do = self._DeviceBuffer.from_numpy(self.table, np.ascontiguousarray(order, dtype=np.uint32))
        dc = self._DeviceBuffer(self.table, batch * 4)
        db = self._DeviceBuffer(self.table, batch * 8)
        stats = np.zeros(2, dtype=np.float32)
        L.check(L.load().rs_kmeans_fit_growbatch(self.table._h, dist, self._data.ptr, self.n, do.ptr, batch, c.ctypes.data, len(c), self.n_bins, dc.ptr, db.ptr,
                                                 stats.ctypes.data))
        return dc.download(np.uint32, batch), c, db.download(np.float32, 2 * batch).reshape(batch, 2), stats


# ---- potential-aware abstraction: next-round histograms and a k-means under the greedy EMD (rs_potential.hip; semantics in include/rustsolver_amd.h) -------------
PA_ROW_WORDS, PA_MAX_NEXT = L.PA_ROW_WORDS, L.PA_MAX_NEXT


class SparseRows:
    """The device buffer `next_round_histograms` fills: uint32 [rows][PA_ROW_WORDS], entries `bucket << 8 | count` ascending by bucket, then zeros"""

    def __init__(self, table, rows, n_draws, buffer):
        self.table, self.rows, self.n_draws, self.buffer = table, rows, n_draws, buffer

    @property
    def ptr(self):
        return self.buffer.ptr

    @property
    def nbytes(self):
        return self.buffer.nbytes

    def download(self, first=0, count=None):
        """rows first .. first + count (default: all) as uint32 [count][PA_ROW_WORDS] on the host: the turn round is 2.7 GB, so in slices"""
        count = self.rows - first if count is None else count
        if first < 0 or count < 0 or first + count > self.rows:
            raise IndexError("rows %d .. %d of %d" % (first, first + count, self.rows))
        out = np.empty((count, PA_ROW_WORDS), dtype=np.uint32)
        if out.size:
            L.check(L.load().rs_d2h(self.table._h, out.ctypes.data, self.ptr + first * PA_ROW_WORDS * 4, out.nbytes))
        return out

    def gather(self, indices):
        """the rows `indices` (a few: initial means), one copy each"""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        return np.concatenate([self.download(int(i), 1) for i in idx]) if len(idx) else np.zeros((0, PA_ROW_WORDS), dtype=np.uint32)

    def dense(self, words, n_next):
        """rows as they are stored (uint32 [n][PA_ROW_WORDS] or one row) -> float32 [n][n_next] of count / n_draws"""
        return dense_rows(words, n_next, self.n_draws)


def dense_rows(words, n_next, n_draws):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    one = w.ndim == 1
    w = w.reshape(-1, PA_ROW_WORDS)
    out = np.zeros((len(w), n_next), dtype=np.float32)
    at, j = np.nonzero(w)
    out[at, (w[at, j] >> 8).astype(np.int64)] = (w[at, j] & 255).astype(np.float32) / np.float32(n_draws)
    return out[0] if one else out


def next_round_histograms(table, indexer, next_indexer, next_buckets, n_next, boards=None, out=None):
    """A flop ([2, 3], next [2, 4]) or turn ([2, 4], next [2, 5]) hand as the multiset of the next round's buckets over its 47 / 46 next cards.  next_buckets: the next
    round's bucket file (uint32 [next_indexer.size(1)], values below n_next) as a numpy array or a DeviceBuffer that holds it.  boards: uint8 [n][3 or 4], or None = the
    whole round.  Rows whose hands lie on no listed board are left as they were (a buffer made here starts at zero).  -> SparseRows"""
    from .solver import DeviceBuffer
    nb = indexer.n_cards(indexer.rounds - 1) - 2
    if out is None:
        rows = indexer.size(indexer.rounds - 1)
        out = SparseRows(table, rows, 50 - nb, DeviceBuffer(table, max(rows, 1) * PA_ROW_WORDS * 4))
        out.buffer.zero()
    if isinstance(next_buckets, DeviceBuffer):
        dn = next_buckets
    else:
        nbk = np.ascontiguousarray(next_buckets, dtype=np.uint32).reshape(-1)
        if len(nbk) != next_indexer.size(next_indexer.rounds - 1):
            raise ValueError("the next round's bucket file has %d entries" % next_indexer.size(next_indexer.rounds - 1))
        dn = DeviceBuffer.from_numpy(table, nbk)
    db, n = None, 0
    if boards is not None:
        if np.asarray(boards).size == 0:
            return out
        db, n = _board_rows(table, boards, nb)
    L.check(L.load().rs_next_round_histograms(table._h, indexer._h, next_indexer._h, dn.ptr, n_next, db.ptr if db else None, n, out.ptr))
    return out


def ground_distances(table, centers, dist=DIST_EMD):
    """[K][K] float32 with g[i][j] = the distance of centre i to centre j as rs_kmeans_predict computes it: its d_min_dist with the centres as data and centre j alone"""
    c = np.ascontiguousarray(centers, dtype=np.float32)
    if c.ndim != 2:
        raise ValueError("centers are [k][n_bins]")
    km = Kmeans(table, c)
    return np.stack([km.predict(c[j:j + 1], dist)[1] for j in range(len(c))], axis=1) if len(c) else np.zeros((0, 0), dtype=np.float32)


class PotentialKmeans:
    """k-means over SparseRows under the greedy earth mover's distance whose ground distance is `ground` [n_next][n_next] (distances between the next round's centres).
    table=None gives a host-only object: `distance` works, the device calls do not."""

    def __init__(self, table, rows, ground):
        g = np.ascontiguousarray(ground, dtype=np.float32)
        if g.ndim != 2 or g.shape[0] != g.shape[1]:
            raise ValueError("ground is [n_next][n_next]")
        h = C.c_void_p()
        L.check(L.load().rs_pa_metric_create(table._h if table is not None else None, g.ctypes.data, g.shape[0], C.byref(h)))
        self._h, self.table, self.rows, self.n_next = h, table, rows, g.shape[0]

    def _means(self, means):
        m = np.array(means, dtype=np.float32, order="C")
        if m.ndim != 2 or m.shape[1] != self.n_next:
            raise ValueError("means are [k][n_next]")
        return m

    def _sel(self, sel):
        from .solver import DeviceBuffer
        if sel is None:
            return None, self.rows.rows
        s = np.ascontiguousarray(sel, dtype=np.uint32).reshape(-1)
        return (DeviceBuffer.from_numpy(self.table, s) if len(s) else None), len(s)

    def distance(self, row, mean, n_draws=None):
        """one distance on the host: row uint32 [PA_ROW_WORDS], mean float32 [n_next]"""
        r = np.ascontiguousarray(row, dtype=np.uint32).reshape(-1)
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        if len(r) != PA_ROW_WORDS or len(m) != self.n_next:
            raise ValueError("a row of PA_ROW_WORDS words and a mean of n_next values")
        out = C.c_float()
        L.check(L.load().rs_pa_distance(self._h, r.ctypes.data, self.rows.n_draws if n_draws is None else n_draws, m.ctypes.data, C.byref(out)))
        return np.float32(out.value)

    def predict(self, means, sel=None):
        """-> (clusters uint32 [n], distance to the chosen mean float32 [n]); datum i is row sel[i] (None: every row)"""
        from .solver import DeviceBuffer
        m = self._means(means)
        ds, n = self._sel(sel)
        dc, dm = DeviceBuffer(self.table, max(n, 1) * 4), DeviceBuffer(self.table, max(n, 1) * 4)
        L.check(L.load().rs_pa_predict(self.table._h, self._h, self.rows.ptr, ds.ptr if ds else None, n, self.rows.n_draws, m.ctypes.data, len(m), dc.ptr, dm.ptr))
        return dc.download(np.uint32, n), dm.download(np.float32, n)

    def fit(self, means, iterations=10, sel=None):
        """the Lloyd loop -> (clusters uint32 [n], new means [k][n_next], distances float32 [n], changed uint32 [iterations run])"""
        from .solver import DeviceBuffer
        m = self._means(means)
        ds, n = self._sel(sel)
        dc, dm = DeviceBuffer(self.table, max(n, 1) * 4), DeviceBuffer(self.table, max(n, 1) * 4)
        changed, ran = np.zeros(max(iterations, 1), dtype=np.uint32), C.c_int()
        L.check(L.load().rs_pa_fit(self.table._h, self._h, self.rows.ptr, ds.ptr if ds else None, n, self.rows.n_draws, m.ctypes.data, len(m), iterations, dc.ptr, dm.ptr,
                                   changed.ctypes.data, C.byref(ran)))
        return dc.download(np.uint32, n), m, dm.download(np.float32, n), changed[:ran.value]

    def __del__(self):
        try:
            L.load().rs_pa_metric_destroy(self._h)
        except Exception:
            pass
