"""numpy / scipy models that judge the GPU's mask filter and traversals (tests/test_gpu_apply_mask.py, tests/test_gpu_bfs.py):
``apply_mask`` (osp_csr_apply_mask), ``symmetric_adjacency``, ``bfs_levels`` and ``brandes`` (graph.py).  Written for
clarity, not speed, and on purpose NOT in the GPU's formulation: the search walks one source at a time over adjacency
lists, and the dependencies are accumulated in dense arrays.  tests/test_apply_mask_cpu.py checks the models themselves
against scipy's shortest paths and networkx's betweenness."""
import numpy as np
import scipy.sparse as sp


def apply_mask(rowptr, col, val, m_rowptr, m_col, ncol, complement=False):
    """The entries of the CSR (rowptr, col, val) whose coordinate is (complement: is not) in the CSR pattern
    (m_rowptr, m_col); values are passed through untouched.  Returns (rowptr, col, val)."""
    rowptr, m_rowptr = np.asarray(rowptr, np.int64), np.asarray(m_rowptr, np.int64)
    nrow = len(rowptr) - 1
    row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(rowptr))
    m_row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(m_rowptr))
    key = row * int(ncol) + np.asarray(col, np.int64)
    m_key = m_row * int(ncol) + np.asarray(m_col, np.int64)
    keep = np.isin(key, m_key)
    if complement:
        keep = ~keep
    out_ptr = np.zeros(nrow + 1, np.int64)
    np.add.at(out_ptr, row[keep] + 1, 1)
    return np.cumsum(out_ptr), np.asarray(col)[keep], np.asarray(val)[keep]


def symmetric_adjacency(rows, cols, n):
    """scipy CSR of the undirected simple graph: A + A.T, the diagonal removed, every value 1, columns ascending."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    A = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    S = (A + A.T).tocoo()
    off = S.row != S.col
    S = sp.csr_matrix((np.ones(int(off.sum())), (S.row[off], S.col[off])), shape=(n, n))
    S.sort_indices()
    return S


def bfs_levels(adj, sources, max_levels=None):
    """Breadth-first search of the scipy CSR `adj` from every source on its own.  Returns (level int32 [S, n] with -1 where
    unreached, sigma float64 [S, n], the exact shortest-path counts, info): info = levels (the deepest
    level reached by any source) and per level d = 1, 2, ... of the BATCHED search the lists nnz_product (the entries of
    frontier @ adj: for every source, the distinct neighbours of its level d - 1) and nnz_new (of those, the unvisited)."""
    n = adj.shape[0]
    ptr, idx = adj.indptr.astype(np.int64), adj.indices.astype(np.int64)
    sources = np.atleast_1d(np.asarray(sources, np.int64))
    S = len(sources)
    level = np.full((S, n), -1, np.int32)
    sigma = np.zeros((S, n), np.float64)   # sums of non-negative integers: exact, and never back below 2^53 once above it
    nnz_product, nnz_new = [], []
    for i, s in enumerate(sources):
        lv, sg = level[i], sigma[i]
        lv[s] = 0
        sg[s] = 1.0
        frontier, d = np.array([s], np.int64), 0
        while frontier.size and (max_levels is None or d < max_levels):
            d += 1
            # every edge u -> v out of the frontier
            cnt = ptr[frontier + 1] - ptr[frontier]
            u = np.repeat(frontier, cnt)
            v = idx[np.repeat(ptr[frontier], cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)]
            fresh = lv[v] < 0
            new = np.unique(v[fresh])
            lv[new] = d
            np.add.at(sg, v[fresh], sg[u[fresh]])
            while len(nnz_product) < d:
                nnz_product.append(0)
                nnz_new.append(0)
            nnz_product[d - 1] += len(np.unique(v))
            nnz_new[d - 1] += len(new)
            frontier = new
    assert not sigma.size or sigma.max() < 2.0 ** 53
    return level, sigma, {"levels": int(level.max()) if level.size else 0, "nnz_product": nnz_product, "nnz_new": nnz_new}


def brandes(adj, sources=None):
    """sum over the sources s (default: all vertices) of Brandes' dependency delta_s(v), v != s, as float64 [n]:
    unnormalised and not halved (all sources of an undirected graph: twice networkx's unnormalised betweenness).  Per
    source: vertices in order of non-increasing distance, delta[u] += sigma[u] / sigma[v] * (1 + delta[v]) over the
    predecessors u of v."""
    n = adj.shape[0]
    ptr, idx = adj.indptr, adj.indices
    sources = np.arange(n) if sources is None else np.atleast_1d(np.asarray(sources, np.int64))
    level, sigma, _ = bfs_levels(adj, sources)
    bc = np.zeros(n)
    deg = np.diff(ptr)
    src_of = np.repeat(np.arange(n), deg)
    for i, s in enumerate(sources):
        lv, sg = level[i], sigma[i]
        delta = np.zeros(n)
        for d in range(int(lv.max()), 0, -1):
            # the edges u -> v with level[v] == d and level[u] == d - 1, all at once (one vertex's terms in adjacency order)
            e = np.nonzero((lv[src_of] == d - 1) & (lv[idx] == d))[0]
            u, v = src_of[e], idx[e]
            np.add.at(delta, u, sg[u] / sg[v] * (1.0 + delta[v]))
        delta[s] = 0.0
        bc += delta
    return bc


def grid_edges(w, h):
    """Edge list of the w x h grid graph, vertex y * w + x."""
    v = np.arange(w * h).reshape(h, w)
    rows = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    cols = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return w * h, rows, cols
