"""GPU (-m gpu): the member lists of the float deal apply (rs_member_lists), a stable sort of the deal indices by cluster, against numpy: members[start[c] ..
start[c + 1]) = the indices whose key is c, ascending; keys >= k count as k - 1.  Up to 16 384 clusters and 2^22 entries of its [tile][cluster] histogram the counting sort
with one LDS counter per cluster builds them, otherwise the radix sort (tiles of 2048 data, at most 8 key bits per pass; 4 M keys at 16 384 clusters take it too); both
must give the one permutation a stable sort defines."""
import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd.solver import DeviceBuffer

pytestmark = pytest.mark.gpu

LDS_TILE, RADIX_TILE = 512, 2048


@pytest.fixture(scope="module")
def table():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need a real MI355X (there is no CPU fallback)")
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    return rs.create_infosets(n_actions, tree, [4], [1])


def make_keys(kind, n, k, rng):
    if kind == "uniform":
        return rng.integers(0, k, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "equal":
        return np.full(n, k // 2, dtype=np.uint32)
    if kind == "clamped":   # a third of the keys at or above k, some at the top of the range
        keys = rng.integers(0, k, size=n, dtype=np.uint64).astype(np.uint32)
        over = rng.random(n) < 0.33
        keys[over] = rng.integers(k, 2**32, size=int(over.sum()), dtype=np.uint64).astype(np.uint32)
        keys[:: 7] = 0xFFFFFFFF
        return keys
    assert kind == "heavy"   # most of the data in three clusters, the rest spread
    keys = rng.integers(0, k, size=n, dtype=np.uint64).astype(np.uint32)
    heavy = np.array([0, k - 1, k // 3], dtype=np.uint32)
    pick = rng.random(n) < 0.9
    keys[pick] = heavy[rng.integers(0, 3, size=int(pick.sum()))]
    return keys


def member_lists(table, keys, k):
    n = len(keys)
    d_keys = DeviceBuffer.from_numpy(table, keys) if n else DeviceBuffer(table, 4)
    d_start = DeviceBuffer(table, (k + 1) * 4)
    d_members = DeviceBuffer(table, max(n, 1) * 4)
    L.check(L.load().rs_member_lists(table._h, d_keys.ptr, n, k, d_start.ptr, d_members.ptr))
    out = d_start.download(np.uint32, k + 1), d_members.download(np.uint32, n)
    for b in (d_keys, d_start, d_members):
        b.free()
    return out


def check(table, keys, k):
    clamped = np.minimum(keys, np.uint32(k - 1))
    want_members = np.argsort(clamped, kind="stable").astype(np.uint32)
    want_start = np.zeros(k + 1, dtype=np.uint32)
    np.cumsum(np.bincount(clamped, minlength=k), out=want_start[1:])
    start, members = member_lists(table, keys, k)
    assert start.tobytes() == want_start.tobytes(), "start differs (n=%d, k=%d)" % (len(keys), k)
    assert members.tobytes() == want_members.tobytes(), "members differ (n=%d, k=%d)" % (len(keys), k)


SMALL_N = sorted({1, LDS_TILE - 1, LDS_TILE, LDS_TILE + 1, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 3 * RADIX_TILE + 17})


@pytest.mark.parametrize("k", [1, 2, 16384, 16385, 55000, 1 << 20, 1 << 24])
@pytest.mark.parametrize("kind", ["uniform", "equal", "clamped", "heavy"])
def test_member_lists_equal_a_stable_argsort(table, k, kind):
    rng = np.random.Generator(np.random.PCG64(k * 7 + len(kind)))
    for n in SMALL_N:
        check(table, make_keys(kind, n, k, rng), k)


@pytest.mark.parametrize("k", [16384, 55000, 1 << 20, 1 << 24])
@pytest.mark.parametrize("kind", ["uniform", "heavy"])
def test_member_lists_at_four_million_deals(table, k, kind):
    rng = np.random.Generator(np.random.PCG64(k + 3))
    check(table, make_keys(kind, 1 << 22, k, rng), k)


def test_member_lists_edge_cases(table):
    check(table, np.zeros(0, dtype=np.uint32), 1)          # no data: every list empty
    check(table, np.zeros(0, dtype=np.uint32), 70000)
    check(table, np.array([5], dtype=np.uint32), 70000)
    with pytest.raises(rs.RsError):
        member_lists(table, np.zeros(4, dtype=np.uint32), 0)
