"""numpy restatement of the potential-aware abstraction (include/rustsolver_amd.h): the sparse next-round row of a hand, the greedy earth mover's
distance of Ganzfried and Sandholm's Algorithm 2 in f32 without FMA, the assignment and the Lloyd loop.  Written from the definition, not from the kernels: the
distance is vectorised over (row, mean) pairs and walks the (rank, entry) lockstep in Python; nothing here runs ahead, skips or takes tickets."""
import numpy as np

F32 = np.float32
ROW_WORDS = 48
NO_CLUSTER = 0xFFFFFFFF


# ---- synthetic inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def synthetic_buckets(size, n_next):
    """a bucket file nobody trained: (index * 2654435761 mod 2^32) % n_next"""
    return (((np.arange(size, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) % np.uint64(n_next)).astype(np.uint32)


def synthetic_bucket_at(indices, n_next):
    return (((np.asarray(indices, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) % np.uint64(n_next)).astype(np.uint32)


def tie_ground(n):
    """|i - j|: integer valued, full of equal distances"""
    i = np.arange(n)
    return np.abs(i[:, None] - i[None, :]).astype(F32)


def random_ground(rng, n, duplicates=0):
    """asymmetric f32 distances with a zero diagonal; `duplicates` pairs of centres are made one point (zero off the diagonal, equal rows and columns)"""
    g = rng.random((n, n)).astype(F32) + F32(0.125)
    np.fill_diagonal(g, 0)
    for _ in range(duplicates):
        if n < 2:
            break
        a, b = rng.choice(n, size=2, replace=False)
        g[b, :] = g[a, :]
        g[:, b] = g[:, a]
        g[a, a] = g[a, b] = g[b, a] = g[b, b] = 0
    return np.ascontiguousarray(g, dtype=F32)


def pack_row(buckets, counts):
    """ascending buckets and their counts -> uint32 [ROW_WORDS]"""
    row = np.zeros(ROW_WORDS, dtype=np.uint32)
    row[:len(buckets)] = (np.asarray(buckets, dtype=np.uint32) << 8) | np.asarray(counts, dtype=np.uint32)
    return row


def random_row(rng, n_next, n_draws, entries):
    """a well-formed row of `entries` entries (at most min(n_next, n_draws))"""
    m = min(entries, n_next, n_draws)
    buckets = np.sort(rng.choice(n_next, size=m, replace=False))
    cuts = np.sort(rng.choice(np.arange(1, n_draws), size=m - 1, replace=False)) if m > 1 else np.zeros(0, dtype=np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [n_draws]]))
    return pack_row(buckets, counts)


def random_rows(rng, n, n_next, n_draws):
    """rows of 1, 2, 47 (or as many as fit) and of random numbers of entries"""
    sizes = [1, 2, 47] + rng.integers(1, 48, size=max(n - 3, 0)).tolist()
    return np.stack([random_row(rng, n_next, n_draws, s) for s in sizes[:n]])


def dense(rows, n_next, n_draws):
    """uint32 [n][ROW_WORDS] -> float32 [n][n_next] of count / n_draws"""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, ROW_WORDS)
    out = np.zeros((len(rows), n_next), dtype=F32)
    for j in range(ROW_WORDS):
        used = rows[:, j] != 0
        out[np.nonzero(used)[0], (rows[used, j] >> 8).astype(np.int64)] = (rows[used, j] & 255).astype(F32) / F32(n_draws)
    return out


def counts_of(rows, n_next):
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, ROW_WORDS)
    out = np.zeros((len(rows), n_next), dtype=np.int64)
    for j in range(ROW_WORDS):
        used = rows[:, j] != 0
        out[np.nonzero(used)[0], (rows[used, j] >> 8).astype(np.int64)] = (rows[used, j] & 255).astype(np.int64)
    return out


def well_formed(row, n_next, n_draws):
    row = np.asarray(row, dtype=np.uint32)
    m = int((row != 0).sum())
    if m < 1 or (row[m:] != 0).any() or (row[:m] == 0).any():
        return False
    b, c = (row[:m] >> 8).astype(np.int64), (row[:m] & 255).astype(np.int64)
    return bool((c >= 1).all() and (b < n_next).all() and (np.diff(b) > 0).all() and c.sum() == n_draws)


# ---- the row of a hand --------------------------------------------------------------------------------------------------------------------------------------------
def hand_rows(next_indexer, hands, bucket_of, n_next):
    """hands: uint8 [n][2 + nb] (hole pair, board) -> uint32 [n][ROW_WORDS]; bucket_of(indices) gives the next round's buckets of canonical hand indices"""
    hands = np.asarray(hands, dtype=np.uint8).reshape(len(hands), -1)
    n, nc = hands.shape
    out = np.zeros((n, ROW_WORDS), dtype=np.uint32)
    x = np.arange(52, dtype=np.uint8)
    free = ~(hands[:, :, None] == x[None, None, :]).any(axis=1)                       # [n][52]
    at, card = np.nonzero(free)
    full = np.concatenate([hands[at], card[:, None].astype(np.uint8)], axis=1)
    b = np.asarray(bucket_of(next_indexer.get_index(full)), dtype=np.int64)
    assert (b < n_next).all()
    counts = np.zeros((n, n_next), dtype=np.int64)
    np.add.at(counts, (at, b), 1)
    assert (counts.sum(axis=1) == 52 - nc).all()
    for i in range(n):
        bk = np.nonzero(counts[i])[0]
        out[i, :len(bk)] = (bk.astype(np.uint32) << 8) | counts[i, bk].astype(np.uint32)
    return out


# ---- the distance -------------------------------------------------------------------------------------------------------------------------------------------------
def order_of(ground):
    """order[b][.]: the ids sorted stably by ascending ground[b][.]"""
    return np.argsort(np.asarray(ground, dtype=F32), axis=1, kind="stable")


def distances(rows, means, ground, n_draws, exits=True, order=None, ranks=None, trace=None):
    """rows uint32 [P][ROW_WORDS], means float32 [P][n_next], pair by pair -> float32 [P].  exits: stop once, in every pair, every entry is done or no bucket is
    positive.  ranks (a list): gets the number of ranks walked.  trace (a list): gets (pair, rank, entry) for every take, in the order of the definition; it only
    listens.  A value is positive if it is above 0 in IEEE f32: a subnormal is, -0.0 is not"""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, ROW_WORDS)
    ground = np.asarray(ground, dtype=F32)
    n = ground.shape[0]
    order = order_of(ground) if order is None else order
    rem = np.array(means, dtype=F32).reshape(len(rows), n)
    P = len(rows)
    used = rows != 0
    bk = (rows >> 8).astype(np.int64)
    target = (rows & 255).astype(F32) / F32(n_draws)
    tot = np.zeros((P, ROW_WORDS), dtype=F32)
    done = ~used
    m_max = int(used.sum(axis=1).max()) if P else 0
    walked = 0
    for i in range(n):
        if exits and (done.all(axis=1) | ~(rem > 0).any(axis=1)).all():
            break
        walked += 1
        for j in range(m_max):                       # entry j of every pair at once: a pair stands in `at` once, so the writes below never meet
            at = np.nonzero(~done[:, j])[0]
            b = bk[at, j]
            t = order[b, i]
            a = rem[at, t]
            pos = a > 0
            at, b, t, a = at[pos], b[pos], t[pos], a[pos]
            if not len(at):
                continue
            if trace is not None:
                trace.extend((int(p), i, j) for p in at)
            d = ground[b, t]
            tj = target[at, j]
            part = a < tj
            whole = ~part
            tot[at[part], j] = tot[at[part], j] + a[part] * d[part]
            target[at[part], j] = tj[part] - a[part]
            rem[at[part], t[part]] = F32(0)
            tot[at[whole], j] = tot[at[whole], j] + tj[whole] * d[whole]
            rem[at[whole], t[whole]] = a[whole] - tj[whole]
            target[at[whole], j] = F32(0)
            done[at[whole], j] = True
    if ranks is not None:
        ranks.append(walked)
    dist = np.zeros(P, dtype=F32)
    for j in range(ROW_WORDS):
        dist = dist + np.where(used[:, j], tot[:, j], F32(0))
    assert dist.dtype == F32 and tot.dtype == F32 and rem.dtype == F32
    return dist


def distance_matrix(rows, means, ground, n_draws, order=None):
    """every row against every mean -> float32 [n][K]"""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, ROW_WORDS)
    means = np.asarray(means, dtype=F32)
    n, k = len(rows), len(means)
    d = distances(np.repeat(rows, k, axis=0), np.tile(means, (n, 1)), ground, n_draws, order=order)
    return d.reshape(n, k)


def predict(rows, means, ground, n_draws, order=None):
    """-> (the first mean with the strictly smallest distance uint32 [n], that distance float32 [n])"""
    d = distance_matrix(rows, means, ground, n_draws, order)
    c = np.argmin(d, axis=1)                      # the first of equal minima
    return c.astype(np.uint32), d[np.arange(len(d)), c]


def fit(rows, means, ground, n_draws, iterations):
    """the Lloyd loop -> (clusters, means, distances, changed [iterations run])"""
    ground = np.asarray(ground, dtype=F32)
    n_next = ground.shape[0]
    order = order_of(ground)
    means = np.array(means, dtype=F32)
    counts = counts_of(rows, n_next)
    clusters = np.full(len(rows), NO_CLUSTER, dtype=np.uint32)
    changed, dist = [], None
    for _ in range(iterations):
        new, dist = predict(rows, means, ground, n_draws, order)
        changed.append(int((new != clusters).sum()))
        clusters = new
        for k in range(len(means)):
            members = int((clusters == k).sum())
            if members:
                total = counts[clusters == k].sum(axis=0)
                means[k] = (total.astype(np.float64) / (np.float64(members) * np.float64(n_draws))).astype(F32)
        if changed[-1] == 0:
            break
    return clusters, means, dist, np.asarray(changed, dtype=np.uint32)
