"""numpy / scipy models that judge the GPU's entry filter and truss functions (tests/test_gpu_select.py,
tests/test_gpu_truss.py): ``select`` (osp_csr_select), ``edge_support``, ``k_truss`` and ``truss_decomposition`` (graph.py).
Written for clarity, not speed.  The truss models follow the round rule of DESIGN.md section 12 so that their ``info``
lists can be compared with the GPU's round for round; tests/test_select_cpu.py checks their edge lists against
``networkx.k_truss``, which peels edges one vertex at a time and shares nothing with them."""
import numpy as np
import scipy.sparse as sp

VALUE_OPS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}
POSITION_OPS = {"tril": np.less_equal, "triu": np.greater_equal, "diag": np.equal, "offdiag": np.not_equal}
OPS = list(VALUE_OPS) + list(POSITION_OPS)


def select(rowptr, col, val, op, threshold=0.0, diag=0, fill=None):
    """The entries of the CSR (rowptr, col, val) that pass ``op``: value ``op`` threshold, compared as float64 (numpy's
    comparisons are IEEE's: false with a NaN on either side, except !=), or column ``op`` row + diag, compared as Python
    integers (no overflow whatever ``diag`` is).  Kept values are passed through untouched, or are all ``fill`` in val's
    dtype.  Returns (rowptr, col, val)."""
    rowptr = np.asarray(rowptr, np.int64)
    col, val = np.asarray(col), np.asarray(val)
    nrow = len(rowptr) - 1
    row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(rowptr))
    if op in VALUE_OPS:
        with np.errstate(invalid="ignore"):
            keep = VALUE_OPS[op](val.astype(np.float64), np.float64(threshold))
    else:
        # |col - row| < 2^32: a diagonal beyond that selects what the nearest diagonal inside selects
        d = max(-(1 << 40), min(1 << 40, int(diag)))
        keep = POSITION_OPS[op](col.astype(np.int64), row + np.int64(d))
    out_ptr = np.zeros(nrow + 1, np.int64)
    np.add.at(out_ptr, row[keep] + 1, 1)
    out_val = val[keep] if fill is None else np.full(int(keep.sum()), fill, val.dtype)
    return np.cumsum(out_ptr), col[keep], out_val


def _supports(adj):
    """(adj @ adj) at adj's pattern, zeros dropped: the masked product's result, as scipy CSR with float64 counts."""
    S = (adj @ adj).multiply(adj).tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return S


def _upper(M):
    U = sp.triu(M, k=1).tocsr()
    U.sort_indices()
    U = U.tocoo()
    return U.row.astype(np.int64), U.col.astype(np.int64), U.data


def edge_support(adj):
    """(u, v, support) of the symmetric 0/1 scipy CSR ``adj``: every edge once, u < v, ascending by (u, v); support int64 =
    the triangles through the edge, counted as common neighbours of its two ends (0 included)."""
    u, v, _ = _upper(adj)
    ptr, idx = adj.indptr, adj.indices
    support = np.array([len(np.intersect1d(idx[ptr[a]:ptr[a + 1]], idx[ptr[b]:ptr[b + 1]], assume_unique=True)) for a, b in zip(u, v)],
                       np.int64).reshape(len(u))
    return u, v, support


def _info():
    return {"rounds": 0, "nnz_graph": [], "nnz_support": [], "nnz_kept": []}


def _level(A, S, k, info):
    """Rounds of level k (graph.py's _truss_level): a round is one support product and one filter S >= k - 2 with the
    values reset to 1; the level ends after the first filter that removes nothing or leaves nothing.  S: A's supports
    where known (their first filter is no round), else None.  Returns (A', S')."""
    while True:
        fresh = S is None
        if fresh:
            S = _supports(A)
        rp, c, v = select(S.indptr, S.indices, S.data, "ge", k - 2, fill=1.0)
        new = sp.csr_matrix((v, c, rp), shape=A.shape)
        if fresh:
            info["rounds"] += 1
            info["nnz_graph"].append(A.nnz)
            info["nnz_support"].append(S.nnz)
            info["nnz_kept"].append(new.nnz)
        A = new
        if new.nnz == S.nnz or new.nnz == 0:
            return A, S
        S = None


def k_truss(adj, k):
    """(u, v, info) of the k-truss of ``adj``, k >= 2 (the 2-truss is every edge and takes no round)."""
    if k < 2:
        raise ValueError("k must be at least 2")
    info = _info()
    A = adj.tocsr()
    if k > 2 and A.nnz:
        A, _ = _level(A, None, k, info)
    u, v, _ = _upper(A)
    return u, v, info


def truss_decomposition(adj):
    """(u, v, trussness, info): for every edge the largest k whose k-truss holds it; info = k_max, products and k_truss's
    lists."""
    A = adj.tocsr()
    u, v, _ = _upper(A)
    n = A.shape[0]
    trussness = np.full(len(u), 2, np.int64)
    info = dict(_info(), k_max=2, products=0)
    S, k = None, 3
    while A.nnz:
        A, S = _level(A, S, k, info)
        if A.nnz == 0:
            break
        tu, tv, _ = _upper(A)
        trussness[np.searchsorted(u * n + v, tu * n + tv)] = k
        info["k_max"] = k
        k += 1
    info["products"] = info["rounds"]
    return u, v, trussness, info


def clique_with_path(q=9, path=21):
    """Edge list of K_q with a path of ``path`` edges attached to vertex 0: (n, rows, cols)."""
    r, c = np.triu_indices(q, 1)
    chain = np.concatenate([[0], np.arange(q, q + path)])
    return q + path, np.concatenate([r, chain[:-1]]), np.concatenate([c, chain[1:]])
