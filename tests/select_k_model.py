"""The numpy model of osp_csr_select_k (include/outerspace_spgemm_select_k.h) and of the graph functions built on it.  A
helper module, not a test file; tests/test_select_k_cpu.py holds it to constructions that share nothing with it.

Per row: a stable argsort on (order key, column), the first k, put back in column order.  The value orders sort the VALUES
(numpy comparisons, NaNs pushed behind by a flag of their own) -- the library's sign-flipped integer keys do not occur here --
and the RANDOM key is the header's hash in ``uint64`` with wrapping arithmetic."""
import numpy as np

ORDERS = ("largest", "smallest", "random")
LONG_MIN = 2048            # kSelectKLongMin: capped rows longer than this are selected by a workgroup
SCAN_TILE, SCAN_SMALL_TILES = 2048, 16
_GOLDEN = 0x9E3779B97F4A7C15
_MASK = (1 << 64) - 1


def mix(z):
    """The header's mix() on a uint64 array (arithmetic mod 2^64)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def random_keys(seed, row, cols):
    """The 64-bit keys of the entries of row ``row`` at columns ``cols`` under ``seed``."""
    s = mix(np.uint64((int(seed) + _GOLDEN) & _MASK))
    coord = (np.uint64(int(row)) << np.uint64(32)) | np.asarray(cols).astype(np.uint64)
    return mix(s ^ coord)


def row_choice(vals, cols, k, order, seed=0, row=0):
    """The positions (ascending) of the entries a row keeps."""
    m = len(cols)
    if m <= k:
        return np.arange(m)
    cols = np.asarray(cols)
    if order == "random":
        rank = np.lexsort((cols, random_keys(seed, row, cols)))
    else:
        v = np.asarray(vals).astype(np.float64)   # (exact for float32; comparisons only)
        nan = np.isnan(v)
        v = np.where(nan, 0.0, v)                  # all NaNs equal, behind every number by the flag
        rank = np.lexsort((cols, -v if order == "largest" else v, nan))   # (-0.0 == 0.0 under the comparison)
    return np.sort(rank[:k])


def scan_launches(n):
    return 1 if n == 0 or -(-n // SCAN_TILE) <= SCAN_SMALL_TILES else 3


def select_k(csr, ncol, k, order, seed=0, long_min=LONG_MIN):
    """``osp_csr_select_k``: returns ((rowptr int64, col uint32, val), stats) with stats nnz_in, nnz_out, rows_capped,
    rows_long, launches, readbacks."""
    assert order in ORDERS and 1 <= k <= 0xffffffff
    rowptr, col, val = csr
    M, nnz = len(rowptr) - 1, len(col)
    lengths = np.diff(rowptr)
    keep = [row_choice(val[rowptr[i]:rowptr[i + 1]], col[rowptr[i]:rowptr[i + 1]], k, order, seed, i) + rowptr[i]
            for i in np.flatnonzero(lengths)]
    pos = np.concatenate(keep + [np.zeros(0, np.int64)]).astype(np.int64)
    out_ptr = np.concatenate([[0], np.cumsum(np.minimum(lengths, k))]).astype(np.int64)
    capped, long_ = int((lengths > k).sum()), int((lengths > max(k, long_min)).sum())
    stats = {"nnz_in": nnz, "nnz_out": len(pos), "rows_capped": 0, "rows_long": 0, "launches": 0, "readbacks": 0}
    if nnz and k < min(ncol, nnz):      # otherwise the host sees that no row can be capped
        stats["launches"], stats["readbacks"] = 1, 1                     # classify, the classes' sizes
        stats["rows_capped"], stats["rows_long"] = capped, long_
        if capped:
            stats["launches"] += (capped > long_) + (long_ > 0) + 1 + scan_launches(-(-nnz // 64)) + 2   # select, flag, scan, rowptr, write
            stats["readbacks"] += 1
    else:
        assert capped == 0
    return (out_ptr, col[pos], val[pos]), stats


# ---- the graphs the device functions build (graph.adjacency_matrix) ------------------------------------------------------------
def adjacency(rows, cols, n, directed=False, weights=None, dup="max"):
    """(rowptr, col, val float64) of the adjacency: undirected = both directions, self loops dropped; directed = as listed,
    self loops kept.  Parallel edges: one entry, the max / min of the weights (1 without weights)."""
    r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    w = np.ones(len(r)) if weights is None else np.asarray(weights, np.float64)
    if not directed:
        keep = r != c
        r, c, w = r[keep], c[keep], w[keep]
        r, c, w = np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([w, w])
    key = r * n + c
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    val = (np.maximum if dup == "max" else np.minimum).reduceat(w, first) if len(key) else w
    key = key[first]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int64)
    return rowptr, (key % n).astype(np.uint32), val


def extract_rows(csr, vertices):
    rowptr, col, val = csr
    pos = np.concatenate([np.arange(rowptr[v], rowptr[v + 1]) for v in vertices] + [np.zeros(0, np.int64)]).astype(np.int64)
    out_ptr = np.concatenate([[0], np.cumsum([rowptr[v + 1] - rowptr[v] for v in vertices])]).astype(np.int64)
    return out_ptr, col[pos], val[pos]


def sample_neighbors(rows, cols, n, seeds, fanouts, seed=0, directed=False):
    """``graph.sample_neighbors``: (blocks as (rowptr, col), frontiers, info with nnz and launches)."""
    A = adjacency(rows, cols, n, directed)
    frontier = np.asarray(seeds, np.int64)
    blocks, frontiers, info = [], [frontier], {"nnz": [], "launches": 0, "rows_capped": []}
    for h, fanout in enumerate(fanouts):
        (bp, bc, _), st = select_k(extract_rows(A, frontier), n, fanout, "random", (seed + h) & _MASK)
        blocks.append((bp, bc))
        info["nnz"].append(len(bc))
        info["rows_capped"].append(st["rows_capped"])
        info["launches"] += st["launches"]
        new = np.setdiff1d(np.unique(bc.astype(np.int64)), frontier)
        frontier = np.concatenate([frontier, new])
        frontiers.append(frontier)
    return blocks, frontiers, info


def _entries(csr, n):
    rowptr, col, val = csr
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr)), col.astype(np.int64), val


def knn_graph(rows, cols, n, weights, k, largest=True, symmetric="union"):
    """``graph.knn_graph``: ((rowptr, col, val), the k-select's stats)."""
    W = adjacency(rows, cols, n, False, weights, "max" if largest else "min")
    S, st = select_k(W, n, k, "largest" if largest else "smallest")
    if symmetric is None:
        return S, st
    r, c, v = _entries(S, n)
    if symmetric == "union":
        key, val = np.concatenate([r * n + c, c * n + r]), np.concatenate([v, v])
        order = np.argsort(key, kind="stable")
        key, val = key[order], val[order]
        first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
        val = (np.maximum if largest else np.minimum).reduceat(val, first) if len(key) else val
        key = key[first]
    else:
        both = np.isin(r * n + c, c * n + r)
        key, val = (r * n + c)[both], v[both]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int64)
    return (rowptr, (key % n).astype(np.uint32), val), st


def random_walks(rows, cols, n, starts, length, seed=0, directed=False):
    """``graph.random_walks``: the int64 array (len(starts), length + 1)."""
    rowptr, col, _ = adjacency(rows, cols, n, directed)
    current = np.asarray(starts, np.int64).copy()
    walks = np.full((len(current), length + 1), -1, np.int64)
    walks[:, 0] = current
    alive = np.ones(len(current), bool)
    for step in range(length):
        for w, v in enumerate(current):
            nb = col[rowptr[v]:rowptr[v + 1]]
            if len(nb) == 0:
                alive[w] = False
                continue
            current[w] = int(nb[np.argmin(random_keys((seed + step) & _MASK, w, nb))])
        walks[alive, step + 1] = current[alive]
    return walks
