"""Graph analytics on the library's products: triangle counting on the masked product (``osp_spgemm_masked``) and Markov
clustering on the plain one with ``osp_csr_inflate_prune`` between two expansions (``markov_cluster``, at the end).

``triangle_count`` is ``sum((L @ L.T) * L)`` for the adjacency L of the graph with every edge oriented from its
lower-ranked end to its higher-ranked end, vertices ranked by (degree, id).  A vertex's out-neighbours then have at least
its own degree, so every row of L has at most sqrt(2m) entries: hub vertices cost no more than any other.  The plumbing
(self loops, symmetrising, deduplication, ranking, L in CSR and CSC) runs in torch on the tensors' device; the product is
the library's.  No reference counterpart.
"""
import numpy as np
import torch

from . import spgemm as _S


def _as_index(x, device):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    return t.to(device=device, dtype=torch.int64)


def oriented_adjacency(rows, cols, n=None, device=None):
    """L of ``triangle_count`` from an edge list (any direction, duplicates and self loops allowed): vertices are
    relabelled by their rank in (degree, id) order, every undirected edge {u, v} becomes one entry L[rank u, rank v] with
    rank u < rank v.  Returns (n, rowptr, colidx, colptr, rowidx) as int64 tensors on `device` (default: the edges'):
    L in CSR and the same L in CSC, indices ascending inside every row / column."""
    device = torch.device(device) if device is not None else (rows.device if torch.is_tensor(rows) else torch.device("cpu"))
    r, c = _as_index(rows, device), _as_index(cols, device)
    if r.shape != c.shape:
        raise ValueError("rows and cols must have the same length")
    if n is None:
        n = int(torch.maximum(r.max(), c.max()).item()) + 1 if r.numel() else 0
    n = int(n)
    if r.numel() and (int(torch.minimum(r.min(), c.min()).item()) < 0 or int(torch.maximum(r.max(), c.max()).item()) >= n):
        raise ValueError(f"vertex ids must lie in [0, {n})")
    keep = r != c
    r, c = r[keep], c[keep]
    # symmetrise and deduplicate: every undirected edge once per direction
    key = torch.unique(torch.cat([r * n + c, c * n + r]))
    u, v = key // n, key % n
    deg = torch.bincount(u, minlength=n)
    rank = torch.empty(n, dtype=torch.int64, device=device)
    rank[torch.argsort(deg * n + torch.arange(n, device=device))] = torch.arange(n, device=device)
    ru, rv = rank[u], rank[v]
    fwd = ru < rv
    src, dst = ru[fwd], rv[fwd]
    csr = torch.sort(src * n + dst).values
    csc = torch.sort(dst * n + src).values
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    colptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    if n:
        rowptr[1:] = torch.cumsum(torch.bincount(csr // n, minlength=n), 0)
        colptr[1:] = torch.cumsum(torch.bincount(csc // n, minlength=n), 0)
    return n, rowptr, csr % n, colptr, csc % n


def triangle_count(rows, cols, n=None, ctx=None):
    """Number of triangles of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n): C<L> = L @ L.T on the
    GPU with f64 ones, summed there.  C[i, j] = |out(i) & out(j)| for every edge i -> j of L, so every triangle is counted
    exactly once.  Exact below 2^53 triangles.  rows / cols: torch tensors (any device; the plumbing runs on cuda:ctx.device)
    or array-likes."""
    from .distributed import _as_tensor
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    n, rowptr, colidx, colptr, rowidx = oriented_adjacency(rows, cols, n, device)
    m = int(colidx.numel())
    if m == 0:
        return 0
    ci, ri = colidx.to(torch.int32), rowidx.to(torch.int32)
    ones = torch.ones(m, dtype=torch.float64, device=device)
    torch.cuda.synchronize(device)   # the library works on its own stream
    # A = L in CSC, B = L.T in CSR (= L in CSC), the mask = L in CSR
    a = (colptr.data_ptr(), ri.data_ptr(), ones.data_ptr())
    res = ctx.spgemm_masked_device(np.float64, n, n, n, a + a, (rowptr.data_ptr(), ci.data_ptr()))
    try:
        vals = _as_tensor(res.device_ptrs()[2], res.nnz, "<f8", device, torch.float64)
        total = float(vals.sum().item())
    finally:
        res.close()
    return int(total)


def walk_pattern(rows, cols, n=None, weights=None, device=None):
    """A + I of ``markov_cluster`` from an edge list (any direction, duplicates and self loops allowed): the graph is made
    symmetric, self loops are dropped, duplicate edges become one (weighted: the MAXIMUM of their weights, whichever
    direction they were given in), and every vertex gets a self loop of weight 1 (weighted: of the largest weight in its
    row, 1 for an isolated vertex).  Returns (n, rowptr int64, colidx int64, vals float64) as tensors on `device`
    (default: the edges'), CSR with ascending columns.  Runs on the CPU as well."""
    device = torch.device(device) if device is not None else (rows.device if torch.is_tensor(rows) else torch.device("cpu"))
    r, c = _as_index(rows, device), _as_index(cols, device)
    if r.shape != c.shape:
        raise ValueError("rows and cols must have the same length")
    if n is None:
        n = int(torch.maximum(r.max(), c.max()).item()) + 1 if r.numel() else 0
    n = int(n)
    if r.numel() and (int(torch.minimum(r.min(), c.min()).item()) < 0 or int(torch.maximum(r.max(), c.max()).item()) >= n):
        raise ValueError(f"vertex ids must lie in [0, {n})")
    keep = r != c
    r, c = r[keep], c[keep]
    both = torch.cat([r * n + c, c * n + r])
    if weights is None:
        key = torch.unique(both)
        w = torch.ones(key.numel(), dtype=torch.float64, device=device)
    else:
        wt = torch.as_tensor(np.asarray(weights, np.float64) if not torch.is_tensor(weights) else weights).to(device=device, dtype=torch.float64)
        if wt.shape != keep.shape:
            raise ValueError("weights must have one entry per edge")
        wt = wt[keep]
        key, inv = torch.unique(both, return_inverse=True)
        w = torch.zeros(key.numel(), dtype=torch.float64, device=device)
        w.scatter_reduce_(0, inv, torch.cat([wt, wt]), reduce="amax", include_self=False)
    u = key // n
    loop = torch.ones(n, dtype=torch.float64, device=device)
    if weights is not None and key.numel():
        loop.scatter_reduce_(0, u, w, reduce="amax", include_self=False)   # (untouched rows, the isolated vertices, keep 1)
    diag = torch.arange(n, dtype=torch.int64, device=device)
    allkey, order = torch.sort(torch.cat([key, diag * n + diag]))
    vals = torch.cat([w, loop])[order]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    if n:
        rowptr[1:] = torch.cumsum(torch.bincount(allkey // n, minlength=n), 0)
    return n, rowptr, allkey % n, vals


def _cluster_labels(n, rowptr, colidx):
    """Vertex j's attractors are the columns of row j; clusters are the connected components of that relation, numbered in
    ascending order of their smallest vertex."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    g = sp.csr_matrix((np.ones(len(colidx), np.int8), np.asarray(colidx, np.int64), np.asarray(rowptr, np.int64)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    _, first = np.unique(lab, return_index=True)
    remap = np.empty(len(first), np.int64)
    remap[np.argsort(first, kind="stable")] = np.arange(len(first))
    return remap[lab]


def markov_cluster(rows, cols, n=None, *, inflation=2.0, threshold=1e-4, max_per_row=1000, max_iter=100, tol=1e-6, weights=None,
                   dtype=np.float64, ctx=None, return_matrix=False):
    """Markov clustering (MCL) of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n), every iteration on
    the GPU: expand T <- T @ T (the library's product, the previous result handed over in HBM), then
    ``inflate_prune(inflation, threshold, max_per_row)``, until ``chaos < tol`` or ``max_iter`` iterations.  Chaos is judged
    after a step only, so at least one iteration runs: the first T of an unweighted graph has uniform rows, whose chaos is 0.

    The walk matrix is kept ROW-stochastic, T = D^-1 (A + I) with A + I from ``walk_pattern``: the transpose of the
    textbook's column-stochastic M ((M^T)^2 = (M^2)^T), so every per-column step of MCL is a per-row step of a CSR result.
    Returns (labels, info): labels[j] = the cluster of vertex j (int64; overlapping clusters merged; numbered in ascending
    order of their smallest vertex); info = iterations, chaos, converged, n_clusters, and per iteration the lists
    nnz_expanded, nnz_kept, ms_product, ms_prune, ms_select (device times), rows_capped, rows_long.  return_matrix=True adds info["matrix"], the final T as
    scipy CSR.  rows / cols / weights: torch tensors (any device) or array-likes."""
    from .sparse_util import _result_as_input
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    dtype = np.dtype(dtype).type
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    n, rowptr, colidx, vals = walk_pattern(rows, cols, n, weights, device)
    info = {"iterations": 0, "chaos": 0.0, "converged": True, "n_clusters": 0, "nnz_expanded": [], "nnz_kept": [], "ms_product": [],
            "ms_prune": [], "ms_select": [], "rows_capped": [], "rows_long": []}
    if n == 0:
        return np.zeros(0, np.int64), info
    ci, va = colidx.to(torch.int32), vals.to(tdt)
    torch.cuda.synchronize(device)   # the library works on its own stream
    # the pattern as a library CSR result: the merge of ONE part is the part itself
    pat = ctx.merge_csr_parts_device(dtype, n, n, [(rowptr.data_ptr(), ci.data_ptr(), va.data_ptr())])
    try:
        T, st = pat.inflate_prune(1.0, 0.0, 0)
    finally:
        pat.close()
    # (the first T has uniform rows, whose chaos is 0 whatever the graph: convergence is judged after a step only)
    info["chaos"], info["converged"] = st["chaos"], False
    try:
        while not info["converged"] and info["iterations"] < max_iter:
            a = _result_as_input(T, device)
            ptrs = (a.rows.data_ptr(), a.cols.data_ptr(), a.vals.data_ptr())
            exp = ctx.spgemm_coo_device(dtype, n, n, n, a.nnz, ptrs, a.nnz, ptrs)
            try:
                new, st = exp.inflate_prune(inflation, threshold, max_per_row)
            finally:
                info["nnz_expanded"].append(exp.nnz)
                info["ms_product"].append(exp.info["ms_total"])
                exp.close()
            torch.cuda.synchronize(device)   # torch holds views of T's arrays: nothing of it is in flight when they go back to the pool
            del a
            T.close()
            T = new
            info["iterations"] += 1
            info["nnz_kept"].append(st["nnz_out"])
            info["ms_prune"].append(st["ms_total"])
            info["ms_select"].append(st["ms_select_kernel"])
            info["rows_capped"].append(st["rows_capped"])
            info["rows_long"].append(st["rows_long"])
            info["chaos"], info["converged"] = st["chaos"], st["chaos"] < tol
        rp, cj, _ = T.to_host()
        labels = _cluster_labels(n, rp, cj)
        if return_matrix:
            info["matrix"] = T.to_scipy()
    finally:
        T.close()
    info["n_clusters"] = int(labels.max()) + 1
    return labels, info
