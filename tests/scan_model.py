"""The numpy model of osp_csr_scan and osp_csr_draw (include/outerspace_spgemm_scan.h) and of the two graph functions built on
them (graph.weighted_random_walks, graph.weighted_sample_neighbors).  A helper, not a test file.

The scan's order is the header's: blocks of 32 entries, a sequential scan inside a block from the identity, a sequential scan
of the blocks' totals across the row, S = C (+) L.  ``np.add.accumulate`` on a 1-D array is sequential, one IEEE addition a
step; MIN and MAX are written as the header writes them (``b < a ? b : a``: a NaN is never taken)."""
import numpy as np

BLOCK = 32          # OSP_SCAN_BLOCK
CHAIN_LANE = 16     # kScanChainLane: rows of more blocks are chained by a whole wave
LOCAL_TILE = 128    # kScanLocalThreads: blocks of one workgroup of the local pass
OPS = ("plus", "min", "max")
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """Equal to the bit, NaNs at the same places: which NaN (sign, payload) an addition returns the header leaves open."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def identity(op, dt):
    return dt(0.0) if op == "plus" else dt(np.inf) if op == "min" else dt(-np.inf)


def _accumulate(op, seq):
    """The sequential scan of a 1-D array whose first element is the carry in; returns all but that element."""
    if op == "plus":
        with np.errstate(all="ignore"):
            return np.add.accumulate(seq)[1:]
    # the leader is the first entry that no later one beats: b replaces a only when b < a (b > a), never a NaN, never a tie
    w = seq.copy() if op == "min" else -seq
    w[np.isnan(w)] = np.inf
    run = np.minimum.accumulate(w)
    improve = np.zeros(len(w), bool)
    improve[1:] = w[1:] < run[:-1]
    leader = np.maximum.accumulate(np.where(improve, np.arange(len(w)), 0))
    return seq[leader][1:]


def _combine(op, a, b):
    """a (+) b with a a scalar and b an array."""
    with np.errstate(all="ignore"):
        if op == "plus":
            return (a + b).astype(b.dtype)
        return np.where(b < a, b, a).astype(b.dtype) if op == "min" else np.where(b > a, b, a).astype(b.dtype)


def scan_row(v, op):
    """S of one row's values (a 1-D array of the dtype)."""
    dt = v.dtype.type
    ident = identity(op, dt)
    out = np.empty_like(v)
    carry = ident
    for b0 in range(0, len(v), BLOCK):
        local = _accumulate(op, np.concatenate([[ident], v[b0:b0 + BLOCK]]).astype(v.dtype))
        out[b0:b0 + BLOCK] = local if b0 == 0 else _combine(op, carry, local)
        carry = _combine(op, carry, local[-1:])[0]
    return out


def scan(csr, op):
    """(rowptr, col, S): the pattern is the operand's."""
    rowptr, col, val = csr
    out = np.empty_like(val)
    for i in range(len(rowptr) - 1):
        out[rowptr[i]:rowptr[i + 1]] = scan_row(val[rowptr[i]:rowptr[i + 1]], op)
    return rowptr, col, out


def scan_launches(n):
    """Kernels of the library's exclusive scan over n items (osp_prims.h)."""
    return 1 if n <= 16 * 2048 else 3


def scan_stats(csr, ncol):
    """The counters of osp_scan_stats_t by the header's cost paragraph."""
    M, nnz = len(csr[0]) - 1, len(csr[1])
    launches = 0
    if M and nnz:
        launches = scan_launches(M) + 1 + (2 if min(ncol, nnz) > BLOCK else 0)
    return {"nnz_in": nnz, "nnz_out": nnz, "blocks": nnz // BLOCK + M, "launches": launches, "readbacks": 0}


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
def mix(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix_array(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def weights(v):
    with np.errstate(invalid="ignore"):
        return np.where((v > 0) & (v < np.inf), v, v.dtype.type(0.0)).astype(v.dtype)


def uniform(h, dt):
    """u of the hashes h (uint64 array) in the dtype: exact."""
    if dt == np.float64:
        return (h >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def pick(S, t):
    """The first q with S_q > t || S_q == total (total = S[-1]); S non-decreasing."""
    total = S[-1]
    ok = (S > t) | (S == total)
    return int(np.argmax(ok))


def draw(csr, draws, seed):
    """(cols, pos, rows_without): M x draws int64 arrays."""
    rowptr, col, val = csr
    dt = val.dtype.type
    M = len(rowptr) - 1
    cols = np.full((M, draws), -1, np.int64)
    pos = np.full((M, draws), -1, np.int64)
    s0 = np.uint64(mix(seed + GOLDEN))
    without = 0
    d = np.arange(draws, dtype=np.uint64)
    for i in range(M):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        S = scan_row(weights(val[b:e]), "plus") if e > b else None
        if S is None or not (0 < S[-1] < np.inf):
            without += 1
            continue
        h = mix_array(s0 ^ ((np.uint64(i) << np.uint64(32)) | d))
        with np.errstate(all="ignore"):
            t = (uniform(h, dt) * S[-1]).astype(dt)
        total = S[-1]
        # the first q with S_q > t || S_q == total: S is non-decreasing
        q = np.minimum(np.searchsorted(S, t, side="right"), np.searchsorted(S, total, side="left"))
        pos[i] = b + q
        cols[i] = col[b + q]
    return cols, pos, without


def draw_stats(csr, ncol, draws):
    M, nnz = len(csr[0]) - 1, len(csr[1])
    ran = M and nnz
    return {"nnz_in": nnz, "nnz_out": M * draws, "launches": scan_stats(csr, ncol)["launches"] + 3 if ran else 0, "readbacks": 1 if ran else 0}


# ---- the graph functions -----------------------------------------------------------------------------------------------------------
def adjacency(rows, cols, n, w, directed, dt):
    """The weighted adjacency as graph.adjacency_matrix(dup="plus") builds it: self loops dropped unless directed, the list
    followed by its mirrored copy unless directed, parallel edges added in list order."""
    r, c, w = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(w, dt)
    if not directed:
        keep = r != c
        r, c, w = r[keep], c[keep], w[keep]
        r, c, w = np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([w, w])
    order = np.lexsort((np.arange(len(r)), c, r))   # stable: list order inside a coordinate
    r, c, w = r[order], c[order], w[order]
    head = np.ones(len(r), bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(head)
    val = np.empty(len(starts), dt)
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(r)
        acc = w[s]
        for x in w[s + 1:e]:
            acc = dt(acc + x)
        val[k] = acc
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r[head], minlength=n))]).astype(np.int64)
    return rowptr, c[head].astype(np.uint32), val


def extract_rows(csr, rows):
    rowptr, col, val = csr
    lens = (rowptr[1:] - rowptr[:-1])[rows]
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col[idx], val[idx]


def weighted_random_walks(rows, cols, n, w, starts, length, seed=0, directed=False, dt=np.float64):
    A = adjacency(rows, cols, n, w, directed, dt)
    current = np.asarray(starts, np.int64).copy()
    walks = np.full((len(current), length + 1), -1, np.int64)
    walks[:, 0] = current
    alive = np.ones(len(current), bool)
    for step in range(length):
        picked = draw(extract_rows(A, current), 1, (seed + step) & MASK)[0][:, 0]
        moved = picked >= 0
        alive &= moved
        current = np.where(moved, picked, current)
        walks[:, step + 1] = np.where(alive, current, -1)
    return walks


def weighted_sample_neighbors(rows, cols, n, w, seeds, fanouts, seed=0, directed=False, dt=np.float64):
    """(blocks, frontiers): blocks[h] = (rowptr, col, multiplicities)."""
    A = adjacency(rows, cols, n, w, directed, dt)
    frontier = np.asarray(seeds, np.int64)
    frontiers, blocks = [frontier], []
    seen = np.zeros(n, bool)
    seen[frontier] = True
    for h, fanout in enumerate(fanouts):
        picked = draw(extract_rows(A, frontier), fanout, (seed + h) & MASK)[0]
        rowptr, col, val = [0], [], []
        for i in range(len(frontier)):
            c, m = np.unique(picked[i][picked[i] >= 0], return_counts=True)
            col.append(c)
            val.append(m)
            rowptr.append(rowptr[-1] + len(c))
        col = np.concatenate(col + [np.zeros(0, np.int64)])
        blocks.append((np.asarray(rowptr, np.int64), col.astype(np.uint32), np.concatenate(val + [np.zeros(0, np.int64)]).astype(dt)))
        new = np.unique(col[~seen[col]]) if len(col) else np.zeros(0, np.int64)
        seen[new] = True
        frontier = np.concatenate([frontier, new]).astype(np.int64)
        frontiers.append(frontier)
    return blocks, frontiers
