"""Graph analytics on the library's products: triangle counting on the masked product (``osp_spgemm_masked``), Markov
clustering on the plain one with ``osp_csr_inflate_prune`` between two expansions (``markov_cluster``), and traversals
that use both with the mask filter ``osp_csr_apply_mask`` between two levels (``bfs_levels``, ``betweenness_centrality``),
and edge support and k-truss on the masked product with the entry filter ``osp_csr_select`` between two rounds
(``edge_support``, ``k_truss``, ``truss_decomposition``, at the end), and personalised PageRank, which sums a series of
products with the element-wise union ``osp_csr_ewise`` (``personalized_pagerank``), and k-core, Jaccard similarity and the
clustering coefficient on ``osp_csr_reduce`` / ``osp_csr_apply_vectors`` / ``osp_csr_select_vertices`` (``core_numbers``,
``k_core``, ``jaccard_similarity``, ``local_clustering``), and weighted paths on the semiring product of two results
``osp_csr_mxm`` (``shortest_paths``, ``widest_paths``, ``min_plus_closure``), and the first functions on a DIRECTED graph,
which need the transpose of a result ``osp_csr_transpose`` (``strongly_connected``, ``cocitation``,
``bibliographic_coupling``), and global PageRank and connected components on the product of a result with a dense vector
``osp_csr_mxv`` (``pagerank``, ``connected_components``), and subgraphs as matrices of their own on the submatrix of a result
``osp_csr_extract`` (``induced_subgraph``, ``ego_network``, ``largest_component``), and matrices made from an edge list in
one ``osp_csr_build`` (``adjacency_matrix``, ``laplacian``, ``incidence_matrix``, ``line_graph``), and label spreading and
feature propagation on the product of a result with a dense matrix ``osp_csr_mxd`` (``label_spreading``,
``propagate_features``), and edge scores, landmark distance bounds and a factorisation of the observed entries on the sampled
dense-dense product ``osp_csr_sddmm`` (``edge_scores``, ``landmark_bounds``, ``factorize``), and a minimum spanning forest
and a greedy weighted matching on mxv with the winner's column ``osp_csr_mxv_arg`` (``minimum_spanning_forest``,
``greedy_matching``), and BFS parent trees on the semiring product of two results AT a mask ``osp_csr_mxm_masked``
(``bfs_parents``): the first traversal here that never forms the part of a product it would throw away, and matrices put
together from results with the assignment into a region ``osp_csr_assign`` (``bipartite_adjacency``, ``disjoint_union``,
``replace_subgraph``), and product graphs and Kronecker powers on the Kronecker product of two results ``osp_csr_kron``
(``tensor_product``, ``cartesian_product``, ``strong_product``, ``kronecker_power``), and neighbour sampling, k-nearest-neighbour
graphs and uniform random walks on the row-wise k-select ``osp_csr_select_k`` (``sample_neighbors``, ``knn_graph``,
``random_walks``), and their weighted counterparts on the weighted draws ``osp_csr_draw`` (``weighted_random_walks``,
``weighted_sample_neighbors``, at the end).

``triangle_count`` is ``sum((L @ L.T) * L)`` for the adjacency L of the graph with every edge oriented from its
lower-ranked end to its higher-ranked end, vertices ranked by (degree, id).  A vertex's out-neighbours then have at least
its own degree, so every row of L has at most sqrt(2m) entries: hub vertices cost no more than any other.  The plumbing
(self loops, symmetrising, deduplication, ranking, L in CSR and CSC) runs in torch on the tensors' device; the product is
the library's.  No reference counterpart.
"""
import numpy as np
import torch

from . import spgemm as _S
from .spgemm import _torch_dtype


# ---- what the functions below share ------------------------------------------------------------------------
def _as_index(x, device):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    return t.to(device=device, dtype=torch.int64)


def _edges(rows, cols, n, device, weights=None, wdtype=torch.float64):
    """The one check of an edge list: ``rows`` and ``cols`` as int64 tensors on ``device`` (default: the edges' own, the
    CPU for array-likes), one-dimensional and of one length; ``n`` inferred as the largest id + 1 when None, every id in
    [0, n); ``weights``, when given, one value per edge as a tensor of ``wdtype``.  Returns (device, n, r, c, w), w None
    without weights."""
    device = torch.device(device) if device is not None else (rows.device if torch.is_tensor(rows) else torch.device("cpu"))
    r, c = _as_index(rows, device), _as_index(cols, device)
    if r.shape != c.shape or r.dim() != 1:
        raise ValueError("rows and cols must be lists of the same length")
    if n is None:
        n = int(torch.maximum(r.max(), c.max()).item()) + 1 if r.numel() else 0
    n = int(n)
    if r.numel() and (int(torch.minimum(r.min(), c.min()).item()) < 0 or int(torch.maximum(r.max(), c.max()).item()) >= n):
        raise ValueError(f"vertex ids must lie in [0, {n})")
    w = None
    if weights is not None:
        ndt = np.float32 if wdtype == torch.float32 else np.float64
        w = torch.as_tensor(np.asarray(weights, ndt) if not torch.is_tensor(weights) else weights).to(device=device, dtype=wdtype)
        if w.shape != r.shape:
            raise ValueError("weights must have one entry per edge")
    return device, n, r, c, w


def _rowptr(keys, n, device):
    """The row pointers of n rows from sorted keys ``row * n + col``."""
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    if n:
        rowptr[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return rowptr


def _value_dtype(dtype):
    dtype = np.dtype(dtype).type
    if dtype not in (np.float32, np.float64):
        raise TypeError("dtype must be float32 or float64")
    return dtype


def _setup(dtype, ctx):
    """The context first (without a GPU this is where the callers fail), its torch device, the value dtype checked.
    Returns (ctx, device, dtype)."""
    ctx = ctx or _S.default_context()
    return ctx, torch.device("cuda", ctx.device), _value_dtype(dtype)


def _csr_result(ctx, dtype, M, N, rowptr, cols, vals, device, sync=True):
    """Non-empty CSR arrays (torch, on the device: int64, int32, ``dtype``) as a library result: the merge of ONE part is the
    part itself.  ``sync=False``: the caller has synchronised since the arrays were made."""
    if sync:
        torch.cuda.synchronize(device)   # the library works on its own stream
    return ctx.merge_csr_parts_device(dtype, M, N, [(rowptr.data_ptr(), cols.data_ptr(), vals.data_ptr())])


def _close_all(device, results):
    """Close the results (None allowed) once nothing torch holds of their arrays is in flight."""
    torch.cuda.synchronize(device)
    for r in results:
        if r is not None:
            r.close()


def oriented_adjacency(rows, cols, n=None, device=None):
    """L of ``triangle_count`` from an edge list (any direction, duplicates and self loops allowed): vertices are
    relabelled by their rank in (degree, id) order, every undirected edge {u, v} becomes one entry L[rank u, rank v] with
    rank u < rank v.  Returns (n, rowptr, colidx, colptr, rowidx) as int64 tensors on `device` (default: the edges'):
    L in CSR and the same L in CSC, indices ascending inside every row / column."""
    device, n, r, c, _ = _edges(rows, cols, n, device)
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
    return n, _rowptr(csr, n, device), csr % n, _rowptr(csc, n, device), csc % n


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


def _undirected_keys(rows, cols, n, device, weights=None):
    """What ``walk_pattern`` and ``symmetric_adjacency`` share: the edge list checked, self loops dropped, every remaining
    edge in both directions.  Returns (device, n, both, wt): ``both`` holds the keys u * n + v of the kept edges followed by
    those of their reversals (duplicates still in), ``wt`` the kept edges' weights (None without weights)."""
    device, n, r, c, wt = _edges(rows, cols, n, device, weights)
    keep = r != c
    r, c = r[keep], c[keep]
    return device, n, torch.cat([r * n + c, c * n + r]), wt[keep] if wt is not None else None


def walk_pattern(rows, cols, n=None, weights=None, device=None):
    """A + I of ``markov_cluster`` from an edge list (any direction, duplicates and self loops allowed): the graph is made
    symmetric, self loops are dropped, duplicate edges become one (weighted: the MAXIMUM of their weights, whichever
    direction they were given in), and every vertex gets a self loop of weight 1 (weighted: of the largest weight in its
    row, 1 for an isolated vertex).  Returns (n, rowptr int64, colidx int64, vals float64) as tensors on `device`
    (default: the edges'), CSR with ascending columns.  Runs on the CPU as well."""
    device, n, both, wt = _undirected_keys(rows, cols, n, device, weights)
    if weights is None:
        key = torch.unique(both)
        w = torch.ones(key.numel(), dtype=torch.float64, device=device)
    else:
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
    return n, _rowptr(allkey, n, device), allkey % n, vals


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
    n, rowptr, colidx, vals = walk_pattern(rows, cols, n, weights, device)
    info = {"iterations": 0, "chaos": 0.0, "converged": True, "n_clusters": 0, "nnz_expanded": [], "nnz_kept": [], "ms_product": [],
            "ms_prune": [], "ms_select": [], "rows_capped": [], "rows_long": []}
    if n == 0:
        return np.zeros(0, np.int64), info
    ci, va = colidx.to(torch.int32), vals.to(_torch_dtype(dtype))
    pat = _csr_result(ctx, dtype, n, n, rowptr, ci, va, device)
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


def symmetric_adjacency(rows, cols, n=None, device=None):
    """The adjacency matrix of the undirected simple graph of an edge list (any direction, duplicates and self loops
    allowed): symmetric, every edge once per direction, no self loops, unit values -- ``walk_pattern`` without the loops.
    Returns (n, rowptr int64, colidx int64, vals float64) as tensors on `device` (default: the edges'), CSR with ascending
    columns.  Runs on the CPU as well."""
    device, n, both, _ = _undirected_keys(rows, cols, n, device)
    key = torch.unique(both)
    return n, _rowptr(key, n, device), key % n, torch.ones(key.numel(), dtype=torch.float64, device=device)


class _Adjacency:
    """``symmetric_adjacency`` on the device in the two forms the traversals hand to the library: COO (the B operand of
    ``spgemm_coo_device``) and CSR (the B operand of ``spgemm_masked_device``)."""

    def __init__(self, rows, cols, n, device):
        self.n, self.rowptr, colidx, self.vals = symmetric_adjacency(rows, cols, n, device)
        self.nnz = int(colidx.numel())
        self.cols = colidx.to(torch.int32)
        self.rows = torch.repeat_interleave(torch.arange(self.n, dtype=torch.int32, device=device), self.rowptr[1:] - self.rowptr[:-1])

    def coo_ptrs(self):
        return tuple(t.data_ptr() if self.nnz else 0 for t in (self.rows, self.cols, self.vals))

    def csr_ptrs(self):
        return (self.rowptr.data_ptr(),) + tuple(t.data_ptr() if self.nnz else 0 for t in (self.cols, self.vals))


def _check_sources(sources, n):
    src = np.atleast_1d(np.asarray(sources.cpu() if torch.is_tensor(sources) else sources)).astype(np.int64).ravel()
    if src.size and (src.min() < 0 or src.max() >= n):
        raise ValueError(f"sources must lie in [0, {n})")
    return src


def _device_mask_filter(product, visited):
    return product.apply_mask(visited, complement=True)


def _device_union(ctx, visited, new):
    """V + Nx of a traversal by the element-wise union: the patterns are disjoint, so no value is computed.  The traversals'
    default: measured at a tenth of ``_sort_union``'s time (MEASUREMENTS.md section 0h)."""
    U, st = visited.ewise(new, "union", "first")
    return U, st["ms_total"]


def _sort_union(ctx, visited, new):
    """The same union by the sorting merge of two CSR parts, the default before osp_csr_ewise (tools/time_bfs.py --sort-union)."""
    S, n = visited.shape
    U = ctx.merge_csr_parts_device(np.float64, S, n, [visited.device_ptrs(), new.device_ptrs()])
    return U, U.info["ms_total"]


def _bfs_forward(ctx, device, adj, src, max_levels=None, keep_levels=False, mask_filter=_device_mask_filter, union=_device_union):
    """The forward sweep both traversals share.  Returns (level, sigma, info, levels): the dense int32 / float64
    [len(src), n] tensors on `device`, the per-level lists, and -- with keep_levels -- per level d = 0..D the pair
    (N_d as a CsrResult, its entries' positions row * n + col in the dense arrays); the caller closes those results.
    ``mask_filter(product, visited) -> (CsrResult, stats)`` is the step between the product and the union
    (tools/time_bfs.py --host-mask passes the host round trip); ``union(ctx, visited, new) -> (CsrResult, device ms)`` is the
    step after it, ``_device_union`` or ``_sort_union`` (tools/time_bfs.py --sort-union passes the latter)."""
    from .sparse_util import _result_as_input
    S, n = int(src.size), adj.n
    level = torch.full((S, n), -1, dtype=torch.int32, device=device)
    sigma = torch.zeros((S, n), dtype=torch.float64, device=device)
    info = {"levels": 0, "frontier_nnz": [], "nnz_visited": [], "nnz_product": [], "nnz_new": [], "ms_product": [], "ms_mask": [],
            "ms_union": []}
    levels = []
    if S == 0 or n == 0:
        return level, sigma, info, levels
    s_dev = torch.as_tensor(src, device=device)
    lin0 = torch.arange(S, dtype=torch.int64, device=device) * n + s_dev
    level.view(-1)[lin0] = 0
    sigma.view(-1)[lin0] = 1.0
    rp0 = torch.arange(S + 1, dtype=torch.int64, device=device)
    c0, v0 = s_dev.to(torch.int32), torch.ones(S, dtype=torch.float64, device=device)
    torch.cuda.synchronize(device)   # the library works on its own stream
    # the sources as library CSR results, twice after the one synchronisation.  F = the frontier, V = the visited set
    F = V = None
    try:
        F = _csr_result(ctx, np.float64, S, n, rp0, c0, v0, device, sync=False)
        V = _csr_result(ctx, np.float64, S, n, rp0, c0, v0, device, sync=False)
        if keep_levels:
            levels.append((F, lin0))
        a = _result_as_input(F, device)
        d = 0
        while max_levels is None or d < max_levels:
            d += 1
            P = ctx.spgemm_coo_device(np.float64, S, n, n, a.nnz, (a.rows.data_ptr(), a.cols.data_ptr(), a.vals.data_ptr()), adj.nnz,
                                      adj.coo_ptrs())
            try:
                Nx, st = mask_filter(P, V)
            finally:
                info["frontier_nnz"].append(a.nnz)
                info["nnz_visited"].append(V.nnz)
                info["nnz_product"].append(P.nnz)
                info["ms_product"].append(P.info["ms_total"])
                P.close()
            info["nnz_new"].append(Nx.nnz)
            info["ms_mask"].append(st["ms_total"])
            if Nx.nnz == 0:
                Nx.close()
                info["ms_union"].append(0.0)
                break
            try:
                U, ms_union = union(ctx, V, Nx)
            except Exception:
                Nx.close()
                raise
            info["ms_union"].append(ms_union)
            info["levels"] = d
            torch.cuda.synchronize(device)   # torch holds views of F's arrays: nothing of it is in flight when they go back to the pool
            del a
            if not keep_levels:
                F.close()
            V.close()
            F, V = Nx, U
            a = _result_as_input(F, device)
            lin = a.rows.to(torch.int64)[:a.nnz] * n + a.cols.to(torch.int64)
            level.view(-1)[lin] = d
            sigma.view(-1)[lin] = a.vals
            if keep_levels:
                levels.append((F, lin))
        torch.cuda.synchronize(device)
        del a
    except Exception:
        torch.cuda.synchronize(device)
        for res, _ in levels:
            res.close()
        levels = []
        raise
    finally:
        if F is not None and not keep_levels:
            F.close()
        if V is not None:
            V.close()
    return level, sigma, info, levels


def bfs_levels(rows, cols, n=None, sources=(0,), *, max_levels=None, ctx=None):
    """Breadth-first search from every vertex of ``sources`` at once on the undirected graph with edges (rows[e], cols[e])
    on vertices [0, n), every level on the GPU: with the frontier F (one row per source) and the visited set V as CSR
    results, a level is  P = F @ Adj  (the library's product, F handed over in HBM),  Nx = P<¬V>
    (``CsrResult.apply_mask(V, complement=True)``),  V += Nx  (``merge_csr_parts_device``),  F = Nx,  until Nx is empty or
    ``max_levels`` levels were taken.  With (+, x) and unit edge weights the frontier's values ARE the numbers of shortest
    paths, so they come for free.

    Returns (level, sigma, info): ``level`` int32 [len(sources), n], the distance from the source, -1 where unreached;
    ``sigma`` float64 of the same shape, the number of shortest paths from the source (0 where unreached, exact below
    2^53); ``info`` = levels (the deepest level reached) and per product the lists frontier_nnz, nnz_visited, nnz_product,
    nnz_new, ms_product, ms_mask, ms_union (device times).  Duplicate sources are independent rows; a source out of
    range is a ValueError; an isolated source ends after one product.  float64 only.  rows / cols: torch tensors (any
    device; the plumbing runs on cuda:ctx.device) or array-likes."""
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    adj = _Adjacency(rows, cols, n, device)
    src = _check_sources(sources, adj.n)
    level, sigma, info, _ = _bfs_forward(ctx, device, adj, src, max_levels)
    return level.cpu().numpy(), sigma.cpu().numpy(), info


def betweenness_centrality(rows, cols, n=None, sources=None, *, batch=64, ctx=None):
    """Betweenness centrality (Brandes) of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n), ``batch``
    sources at a time, every product on the GPU.  Returns float64 [n]:  bc[v] = sum over s in ``sources``, s != v, of the
    dependency delta_s(v) -- unnormalised and NOT halved: with all vertices as sources (``sources=None``) an undirected
    graph gives TWICE networkx's ``betweenness_centrality(normalized=False)``, every pair being counted from both ends.

    Forward: the sweep of ``bfs_levels``, keeping every level's pattern N_d and the path counts sigma.  Backward, for
    d = D .. 1:  W_d = (1 + delta) / sigma on N_d's pattern,  T = W_d @ Adj wanted only at N_{d-1}'s pattern -- the masked
    product as it stands (``spgemm_masked_device``, W_d in CSC by a sort on the device) --,  delta += sigma * T there."""
    from .sparse_util import _result_as_input
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    adj = _Adjacency(rows, cols, n, device)
    n = adj.n
    src_all = np.arange(n, dtype=np.int64) if sources is None else _check_sources(sources, n)
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    bc = torch.zeros(n, dtype=torch.float64, device=device)
    for b0 in range(0, src_all.size, int(batch)):
        src = src_all[b0:b0 + int(batch)]
        S = int(src.size)
        _, sigma, _, levels = _bfs_forward(ctx, device, adj, src, keep_levels=True)
        try:
            delta = torch.zeros((S, n), dtype=torch.float64, device=device)
            sg, dl = sigma.view(-1), delta.view(-1)
            for d in range(len(levels) - 1, 0, -1):
                lin = levels[d][1]
                w = (1.0 + dl[lin]) / sg[lin]
                # W_d (S x n) in CSC: entries ordered by (column, row)
                r, c = lin // n, lin % n
                order = torch.argsort(c * S + r)
                wv, ri = w[order].contiguous(), r[order].to(torch.int32)
                colptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
                colptr[1:] = torch.cumsum(torch.bincount(c, minlength=n), 0)
                torch.cuda.synchronize(device)   # the library works on its own stream
                T = ctx.spgemm_masked_device(np.float64, S, n, n, (colptr.data_ptr(), ri.data_ptr(), wv.data_ptr()) + adj.csr_ptrs(),
                                             levels[d - 1][0].device_ptrs()[:2])
                try:
                    t = _result_as_input(T, device)
                    tl = t.rows.to(torch.int64)[:t.nnz] * n + t.cols.to(torch.int64)
                    dl[tl] += sg[tl] * t.vals
                    torch.cuda.synchronize(device)   # torch holds views of T's arrays
                    del t
                finally:
                    T.close()
            dl[levels[0][1]] = 0.0   # delta_s(s) is not part of the sum
            bc += delta.sum(0)
        finally:
            _close_all(device, [res for res, _ in levels])
    return bc.cpu().numpy()


# ---- personalised PageRank ---------------------------------------------------------------------------------
def ppr_steps(alpha, tol, max_iter=None):
    """The number of steps K of ``personalized_pagerank``: the smallest k with alpha^(k+1) < tol (what the series' tail
    beyond step k sums to), capped by ``max_iter``."""
    alpha, tol = float(alpha), float(tol)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1)")
    if not tol > 0.0:
        raise ValueError("tol must be positive")
    k = 0
    while alpha ** (k + 1) >= tol:
        k += 1
    return k if max_iter is None else min(k, max(int(max_iter), 0))


def personalized_pagerank(rows, cols, n=None, sources=(0,), *, alpha=0.85, tol=1e-6, max_iter=None, prune=0.0, ctx=None):
    """Personalised PageRank from every vertex of ``sources`` at once on the undirected graph with edges (rows[e], cols[e])
    on vertices [0, n), every step on the GPU, float64: the truncated series  ppr = (1 - alpha) sum_{k=0..K} alpha^k e_s P^k
    with P = D^-1 Adj (row-stochastic, ``symmetric_adjacency``).  With the term F (one row per source) and the sum PI as CSR
    results, a step is  F <- F @ (alpha P)  (the library's product, F handed over in HBM; the operand holds alpha / deg),
    with ``prune > 0``  F <- F.select("ge", prune),  and  PI <- PI.ewise(F, "union", "plus").  K = ``ppr_steps(alpha, tol,
    max_iter)`` is fixed before the loop; the loop ends early only when F is empty.

    Returns (ppr, info): ``ppr`` float64 [len(sources), n]; without pruning a row sums to 1 - alpha^(K+1) (an isolated
    source keeps 1 - alpha on itself and nothing else).  ``info`` = iterations (steps taken), steps (K), and per step the
    lists frontier_nnz (entries of F going into the product), nnz_result (entries of PI after it), ms_product, ms_union,
    ms_select (device times; 0 where the step did not run).  Duplicate sources are independent rows; a source out of range
    is a ValueError.  rows / cols: torch tensors (any device; the plumbing runs on cuda:ctx.device) or array-likes."""
    from .sparse_util import _result_as_input
    K = ppr_steps(alpha, tol, max_iter)
    alpha, prune = float(alpha), float(prune)
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    adj = _Adjacency(rows, cols, n, device)
    n = adj.n
    src = _check_sources(sources, n)
    S = int(src.size)
    info = {"iterations": 0, "steps": K, "frontier_nnz": [], "nnz_result": [], "ms_product": [], "ms_union": [], "ms_select": []}
    ppr = torch.zeros((S, n), dtype=torch.float64, device=device)
    if S == 0 or n == 0:
        return ppr.cpu().numpy(), info
    # alpha P as the product's COO operand: entry (u, v) holds alpha / deg(u)
    deg = (adj.rowptr[1:] - adj.rowptr[:-1]).to(torch.float64)
    w = (alpha / deg)[adj.rows.to(torch.int64)]
    b_ptrs = tuple(t.data_ptr() if adj.nnz else 0 for t in (adj.rows, adj.cols, w))
    rp0 = torch.arange(S + 1, dtype=torch.int64, device=device)
    c0 = torch.as_tensor(src, device=device).to(torch.int32)
    v0 = torch.full((S,), 1.0 - alpha, dtype=torch.float64, device=device)
    torch.cuda.synchronize(device)   # the library works on its own stream
    # the sources as library CSR results, twice after the one synchronisation.  F = the series' term, PI = its sum
    F = PI = a = None
    try:
        F = _csr_result(ctx, np.float64, S, n, rp0, c0, v0, device, sync=False)
        PI = _csr_result(ctx, np.float64, S, n, rp0, c0, v0, device, sync=False)
        for _ in range(K):
            a = _result_as_input(F, device)
            P = ctx.spgemm_coo_device(np.float64, S, n, n, a.nnz, (a.rows.data_ptr(), a.cols.data_ptr(), a.vals.data_ptr()), adj.nnz, b_ptrs)
            info["frontier_nnz"].append(a.nnz)
            info["ms_product"].append(P.info["ms_total"])
            torch.cuda.synchronize(device)   # torch holds views of F's arrays: nothing of it is in flight when they go back to the pool
            a = None
            F.close()
            F = P
            ms_select = 0.0
            if prune > 0.0:
                F, st = P.select("ge", prune)
                P.close()
                ms_select = st["ms_total"]
            info["ms_select"].append(ms_select)
            info["iterations"] += 1
            if F.nnz == 0:
                info["ms_union"].append(0.0)
                info["nnz_result"].append(PI.nnz)
                break
            U, st = PI.ewise(F, "union", "plus")
            PI.close()
            PI = U
            info["ms_union"].append(st["ms_total"])
            info["nnz_result"].append(PI.nnz)
        a = _result_as_input(PI, device)
        ppr.view(-1)[a.rows.to(torch.int64)[:a.nnz] * n + a.cols.to(torch.int64)] = a.vals
    finally:
        a = None
        _close_all(device, (F, PI))
    return ppr.cpu().numpy(), info


# ---- edge support, k-truss -------------------------------------------------------------------------------
def _truss_info():
    return {"rounds": 0, "nnz_graph": [], "nnz_support": [], "nnz_kept": [], "ms_product": [], "ms_select": []}


def _truss_setup(rows, cols, n, dtype, ctx):
    """What the three truss functions share: the context first (without a GPU this is where they fail), the adjacency on
    its device, and the guard of float32's exact range.  Returns (ctx, device, dtype, adj)."""
    ctx, device, dtype = _setup(dtype, ctx)
    adj = _Adjacency(rows, cols, n, device)
    # a support is below the smaller degree of the edge's ends
    if dtype == np.float32 and adj.nnz and int((adj.rowptr[1:] - adj.rowptr[:-1]).max().item()) >= 1 << 24:
        raise ValueError("float32 holds supports exactly only while the maximum degree is below 2^24: use float64")
    return ctx, device, dtype, adj


def _adjacency_result(ctx, adj, dtype, device):
    """A non-empty ``_Adjacency`` as a library CSR result with unit values of ``dtype``."""
    return _csr_result(ctx, dtype, adj.n, adj.n, adj.rowptr, adj.cols, adj.vals.to(_torch_dtype(dtype)), device)


def _support_product(ctx, A):
    """S = (A @ A)<A> for a SYMMETRIC CSR result A with unit values: S[i, j] = the number of triangles through the edge
    {i, j}; an edge in no triangle has no entry.  A's CSR arrays are also its CSC arrays, so it is A, B and the mask of the
    masked product by its device pointers."""
    n = A.shape[0]
    p = A.device_ptrs()
    return ctx.spgemm_masked_device(A.dtype, n, n, n, p + p, p[:2])


def _upper_entries(A):
    """The entries above the diagonal of the CSR result A -- every undirected edge once --, taken on the device
    (``select("triu", diag=1)``).  Returns (u, v, values) on the host, u < v, ascending by (u, v)."""
    U, _ = A.select("triu", diag=1)
    try:
        rowptr, colidx, vals = U.to_host()
        return np.repeat(np.arange(U.shape[0], dtype=np.int64), np.diff(rowptr)), colidx.astype(np.int64), vals
    finally:
        U.close()


def _truss_level(ctx, A, S, k, info, select_step=None):
    """Rounds of level k on the graph A (a symmetric CSR result with unit values) until a filter removes nothing or leaves
    nothing.  S: A's supports where they are known (``truss_decomposition``: the converged supports of level k - 1; the
    first filter then needs no product and is no round), else None.  A and S are closed here.  Returns (A', S'): the k-truss
    and -- unless it is empty -- its supports, on the same pattern.
    ``select_step(result, op, threshold, fill=...) -> (CsrResult, stats)`` is the step between two products, by default
    ``CsrResult.select`` (tools/time_truss.py --host-select passes the host round trip)."""
    select_step = select_step or _S.CsrResult.select
    while True:
        try:
            fresh = S is None
            if fresh:
                S = _support_product(ctx, A)
            new, st = select_step(S, "ge", float(k - 2), fill=1.0)
        except Exception:
            A.close()
            if S is not None:
                S.close()
            raise
        if fresh:
            info["rounds"] += 1
            info["nnz_graph"].append(A.nnz)
            info["nnz_support"].append(S.nnz)
            info["nnz_kept"].append(new.nnz)
            info["ms_product"].append(S.info["ms_total"])
            info["ms_select"].append(st["ms_total"])
        A.close()
        A = new
        # (the edges the product itself dropped lay in no triangle: no survivor's support changed with them)
        if st["nnz_out"] == st["nnz_in"] or st["nnz_out"] == 0:
            return A, S
        S.close()
        S = None


def edge_support(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The number of triangles through every edge of the undirected graph with edges (rows[e], cols[e]) on vertices
    [0, n) (any direction, duplicates and self loops allowed): S = (A @ A)<A>, the masked product as it stands, with A the
    symmetric adjacency, and of A and S the halves above the diagonal by ``select("triu", diag=1)``.  Returns
    (u, v, support): every edge once, u < v, ascending by (u, v), int64; an edge in no triangle has support 0."""
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    if adj.nnz == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    A = _adjacency_result(ctx, adj, dtype, device)
    try:
        u, v, _ = _upper_entries(A)
        S = _support_product(ctx, A)
        try:
            su, sv, sval = _upper_entries(S)
        finally:
            S.close()
    finally:
        A.close()
    support = np.zeros(len(u), np.int64)
    support[np.searchsorted(u * adj.n + v, su * adj.n + sv)] = sval.astype(np.int64)   # (the product has no entry where it is 0)
    return u, v, support


def k_truss(rows, cols, n=None, k=3, *, dtype=np.float64, ctx=None):
    """The k-truss of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n): the largest subgraph in which
    every edge lies in at least k - 2 triangles of the subgraph (``networkx.k_truss``'s definition).  k >= 2; the 2-truss
    is every edge and takes no round.  A ROUND is one support product S = (A @ A)<A> and one
    ``S.select("ge", k - 2, fill=1.0)``, whose result is the next round's A, B and mask by its device pointers; the loop
    ends after the first round whose filter removes nothing or leaves nothing.

    Returns (u, v, info): the truss's edges once each, u < v, ascending by (u, v), int64; info = rounds, and per round the
    lists nnz_graph, nnz_support, nnz_kept (directed entries: twice the edges), ms_product, ms_select (device times).
    float32 is allowed while every support is exact (maximum degree below 2^24, else ValueError)."""
    return _k_truss(rows, cols, n, k, dtype, ctx)


def _k_truss(rows, cols, n, k, dtype, ctx, select_step=None):
    k = int(k)
    if k < 2:
        raise ValueError("k must be at least 2")
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    info = _truss_info()
    if adj.nnz == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), info
    A = _adjacency_result(ctx, adj, dtype, device)
    if k > 2:
        A, S = _truss_level(ctx, A, None, k, info, select_step)
        S.close()
    try:
        u, v, _ = _upper_entries(A)
    finally:
        A.close()
    return u, v, info


def truss_decomposition(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The trussness of every edge of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n): the largest k
    whose k-truss contains the edge (2 for an edge in no triangle).  Levels k = 3, 4, ... run on the shrinking graph; the
    converged supports of level k are the first filter input of level k + 1, so no product is repeated.

    Returns (u, v, trussness, info): every edge once, u < v, ascending by (u, v), int64; info = k_max (the largest
    trussness; 2 without edges), products (support products in all) and the per-product lists of ``k_truss``."""
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    info = dict(_truss_info(), k_max=2, products=0)
    if adj.nnz == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), info
    A = _adjacency_result(ctx, adj, dtype, device)
    S = None
    try:
        u, v, _ = _upper_entries(A)
        trussness = np.full(len(u), 2, np.int64)
        k = 3
        while True:
            A, S = _truss_level(ctx, A, S, k, info)
            if A.nnz == 0:
                break
            tu, tv, _ = _upper_entries(A)
            trussness[np.searchsorted(u * adj.n + v, tu * adj.n + tv)] = k
            info["k_max"] = k
            k += 1
    finally:
        A.close()
        if S is not None:
            S.close()
    info["products"] = info["rounds"]
    return u, v, trussness, info


# ---- k-core, Jaccard similarity, clustering coefficient --------------------------------------------------
def _degrees(A, deg, device):
    """deg <- the entries per row of the CSR result A (``reduce("rows", "count")``), written on the device into the torch
    vector ``deg`` of A's dtype.  Returns the call's device time."""
    torch.cuda.synchronize(device)   # the library works on its own stream
    _, st = A.reduce("rows", "count", out=deg)
    return st["ms_total"]


def _core_info():
    return {"rounds": 0, "nnz_graph": [], "ms_reduce": [], "ms_select": []}


def _peel_level(A, k, deg, device, info):
    """Rounds of level k on the graph A (a symmetric CSR result): the degrees, and -- unless every vertex that still has an
    edge has at least k of them -- the subgraph induced by the vertices of degree >= k, until nothing is removed.  A is
    closed here when it is replaced.  Returns A', the k-core; ``deg`` holds its degrees."""
    while True:
        ms = _degrees(A, deg, device)
        info["rounds"] += 1
        info["nnz_graph"].append(A.nnz)
        info["ms_reduce"].append(ms)
        keep = deg >= k
        if not bool(((deg > 0) & ~keep).any().item()):
            info["ms_select"].append(0.0)
            return A
        keep8 = keep.to(torch.uint8)
        torch.cuda.synchronize(device)
        try:
            new, st = A.select_vertices(keep8, keep8)
        except Exception:
            A.close()
            raise
        info["ms_select"].append(st["ms_total"])
        A.close()
        A = new


def core_numbers(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The core number of every vertex of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n) (any
    direction, duplicates and self loops allowed): the largest k whose k-core -- the largest subgraph in which every vertex
    has at least k neighbours -- contains the vertex (``networkx.core_number``).  Peeling, every matrix step on the GPU:
    for k = 1, 2, ... a ROUND is  deg = A.reduce("rows", "count")  and, when a vertex with 0 < deg < k exists,
    A = A.select_vertices(deg >= k, deg >= k);  a level ends with the first round that removes nothing.  A vertex removed at
    level k has core number k - 1, an isolated vertex 0.  torch touches the length-n vectors only.

    Returns (core int64[n], info): info = rounds, k_max (the largest core number), and per round the lists nnz_graph
    (directed entries: twice the edges), ms_reduce, ms_select (device times; 0 where the round removed nothing)."""
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    info = dict(_core_info(), k_max=0)
    core = torch.zeros(adj.n, dtype=torch.int64, device=device)
    if adj.nnz == 0:
        return core.cpu().numpy(), info
    deg = torch.empty(adj.n, dtype=_torch_dtype(dtype), device=device)
    A = _adjacency_result(ctx, adj, dtype, device)
    try:
        k = 1
        while True:
            A = _peel_level(A, k, deg, device, info)
            if A.nnz == 0:
                break
            core[deg > 0] = k   # (every vertex that still has an edge is in the k-core)
            info["k_max"] = k
            k += 1
    finally:
        _close_all(device, [A])
    return core.cpu().numpy(), info


def k_core(rows, cols, n=None, k=1, *, dtype=np.float64, ctx=None):
    """The k-core of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n): the largest subgraph in which
    every vertex has at least k neighbours (``networkx.k_core``'s definition), by the rounds of ``core_numbers`` at the one
    level k.  k >= 0; the 0-core and the 1-core hold every edge.

    Returns (u, v, info): the core's edges once each, u < v, ascending by (u, v), int64; info = rounds and the per-round
    lists of ``core_numbers``."""
    k = int(k)
    if k < 0:
        raise ValueError("k must be at least 0")
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    info = _core_info()
    if adj.nnz == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), info
    deg = torch.empty(adj.n, dtype=_torch_dtype(dtype), device=device)
    A = _adjacency_result(ctx, adj, dtype, device)
    try:
        A = _peel_level(A, k, deg, device, info)
        u, v, _ = _upper_entries(A)
    finally:
        _close_all(device, [A])
    return u, v, info


def jaccard_similarity(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The Jaccard similarity |N(u) & N(v)| / |N(u) | N(v)| of the ends of every edge of the undirected graph with edges
    (rows[e], cols[e]) on vertices [0, n), every matrix step on the GPU:  S = (A @ A)<A>  (the common neighbours, the
    masked product as it stands),  D = S.apply_vectors(deg, "second", deg, "plus")  (deg u + deg v on S's pattern),
    U = D.ewise(S, "intersect", "minus")  (the union's size),  J = S.ewise(U, "intersect", "div").  Every value is ONE
    correctly rounded division of two exact integers, so float64 equals ``networkx.jaccard_coefficient`` as floats.

    Returns (u, v, jaccard): every edge once, u < v, ascending by (u, v); jaccard float64, 0 for an edge without a common
    neighbour.  float32 is allowed while deg u + deg v is exact (maximum degree below 2^23, else ValueError); its values are
    the float32 quotients widened."""
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    if adj.nnz == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    if dtype == np.float32 and int((adj.rowptr[1:] - adj.rowptr[:-1]).max().item()) >= 1 << 23:
        raise ValueError("float32 holds deg u + deg v exactly only while the maximum degree is below 2^23: use float64")
    deg = torch.empty(adj.n, dtype=_torch_dtype(dtype), device=device)
    A = _adjacency_result(ctx, adj, dtype, device)
    held = [A]
    try:
        _degrees(A, deg, device)
        u, v, _ = _upper_entries(A)
        S = _support_product(ctx, A)
        held.append(S)
        D, _ = S.apply_vectors(deg, "second", deg, "plus")
        held.append(D)
        U, _ = D.ewise(S, "intersect", "minus")
        held.append(U)
        J, _ = S.ewise(U, "intersect", "div")
        held.append(J)
        ju, jv, jval = _upper_entries(J)
    finally:
        _close_all(device, held)
    jaccard = np.zeros(len(u), np.float64)
    jaccard[np.searchsorted(u * adj.n + v, ju * adj.n + jv)] = jval.astype(np.float64)   # (the product has no entry where it is 0)
    return u, v, jaccard


def local_clustering(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The local clustering coefficient of every vertex of the undirected graph with edges (rows[e], cols[e]) on vertices
    [0, n): with S = (A @ A)<A>,  t = S.reduce("rows", "plus")  is twice the number of triangles through the vertex, and
    the coefficient is  t / (deg (deg - 1)),  0 where deg < 2 -- ONE correctly rounded float64 division of two exact
    integers, so it equals ``networkx.clustering`` as floats.  The division runs on the host on the length-n vectors.

    Returns float64[n].  float32 is allowed while t is exact (maximum degree below 2^12, else ValueError)."""
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    if adj.nnz == 0:
        return np.zeros(adj.n, np.float64)
    if dtype == np.float32 and int((adj.rowptr[1:] - adj.rowptr[:-1]).max().item()) >= 1 << 12:
        raise ValueError("float32 holds a vertex's triangle sum exactly only while the maximum degree is below 2^12: use float64")
    deg = torch.empty(adj.n, dtype=_torch_dtype(dtype), device=device)
    t = torch.empty(adj.n, dtype=_torch_dtype(dtype), device=device)
    A = _adjacency_result(ctx, adj, dtype, device)
    held = [A]
    try:
        _degrees(A, deg, device)
        S = _support_product(ctx, A)
        held.append(S)
        S.reduce("rows", "plus", out=t)
    finally:
        _close_all(device, held)
    # the one division, in float64 on the host: numpy's is the IEEE division whatever the device's
    d64, t64 = deg.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
    cc = np.zeros(adj.n, np.float64)
    some = d64 >= 2.0
    cc[some] = t64[some] / (d64[some] * (d64[some] - 1.0))
    return cc


# ---- weighted paths on the semiring product of two results (osp_csr_mxm) -------------------------------

def weighted_adjacency(rows, cols, n=None, weights=None, *, directed=False, keep="min", device=None):
    """The weighted adjacency matrix of an edge list (duplicates and self loops allowed): self loops are dropped, an
    undirected graph (``directed=False``) gets every edge in both directions, and duplicate edges become one that keeps the
    smallest (``keep="min"``) or the largest (``"max"``) of their weights.  ``weights=None`` means 1.0 for every edge.
    Returns (n, rowptr int64, colidx int64, vals float64) as tensors on `device` (default: the edges'), CSR with ascending
    columns.  Runs on the CPU as well."""
    if keep not in ("min", "max"):
        raise ValueError('keep must be "min" or "max"')
    device, n, r, c, wt = _edges(rows, cols, n, device, weights)
    if wt is None:
        wt = torch.ones(r.numel(), dtype=torch.float64, device=device)
    loop = r != c
    r, c, wt = r[loop], c[loop], wt[loop]
    keys = r * n + c
    if not directed:
        keys, wt = torch.cat([keys, c * n + r]), torch.cat([wt, wt])
    key, inv = torch.unique(keys, return_inverse=True)
    w = torch.zeros(key.numel(), dtype=torch.float64, device=device)
    if key.numel():
        w.scatter_reduce_(0, inv, wt, reduce="amin" if keep == "min" else "amax", include_self=False)
    return n, _rowptr(key, n, device), key % n, w


def directed_pattern(rows, cols, n=None, device=None):
    """The deduplicated 0/1 adjacency matrix of the DIRECTED graph of an edge list: every edge (rows[e], cols[e]) as given,
    one entry however often it is listed, self loops kept, an edge given in both directions as two entries.  Returns
    (n, rowptr int64, colidx int64, vals float64) as tensors on `device` (default: the edges'), CSR with ascending columns.
    Runs on the CPU as well."""
    device, n, r, c, _ = _edges(rows, cols, n, device)
    key = torch.unique(r * n + c)
    return n, _rowptr(key, n, device), key % n, torch.ones(key.numel(), dtype=torch.float64, device=device)


def _check_weights(weights):
    if weights is None:
        return
    w = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights, np.float64)
    if w.size and not bool((w >= 0).all()):
        raise ValueError("weights must be non-negative (and not NaN)")


def _paths_setup(rows, cols, n, weights, directed, keep, dtype, ctx):
    """What the path functions share: the checks of the arguments, the context (without a GPU this is where they fail), and
    the weighted adjacency on its device.  Returns (ctx, device, dtype, n, rowptr, cols int32, vals of dtype)."""
    _value_dtype(dtype)   # (these two before the context: a bad argument is a Python error without a GPU as well)
    _check_weights(weights)
    ctx, device, dtype = _setup(dtype, ctx)
    n, rowptr, colidx, vals = weighted_adjacency(rows, cols, n, weights, directed=directed, keep=keep, device=device)
    return ctx, device, dtype, n, rowptr, colidx.to(torch.int32), vals.to(_torch_dtype(dtype))


def _paths_info():
    return {"rounds": 0, "frontier_nnz": [], "nnz_product": [], "products": [], "ms_product": []}


def _relax_rounds(W, D, F, add, mul, better, keep, max_iter, info):
    """The frontier rounds ``shortest_paths`` and ``widest_paths`` share, every step on the device.  D holds the best value
    known per (source, vertex), F the entries that changed in the last round:

        P   = F.mxm(W, add, mul)                       the values reached through the frontier
        New = P.apply_mask(D, complement=True)         reached for the first time
        Imp = P.intersect(D, "minus").select(better, 0)   P - D < 0 (> 0) iff P beats D: denormals are kept
        F'  = New.union(P.apply_mask(Imp), "first")
        D'  = D.union(P, keep)

    until F' is empty or ``max_iter`` rounds were taken.  D and F are closed here when they are replaced; returns the last D
    and F."""
    while F.nnz and info["rounds"] < max_iter:
        made = []
        try:
            P, st = F.mxm(W, add, mul)
            made.append(P)
            info["rounds"] += 1
            info["frontier_nnz"].append(F.nnz)
            info["nnz_product"].append(P.nnz)
            info["products"].append(st["products"])
            info["ms_product"].append(st["ms_total"])
            New, _ = P.apply_mask(D, complement=True)
            made.append(New)
            Diff, _ = P.intersect(D, "minus")
            made.append(Diff)
            Imp, _ = Diff.select(better, 0.0)
            made.append(Imp)
            Pi, _ = P.apply_mask(Imp)
            made.append(Pi)
            F2, _ = New.union(Pi, "first")
            made.append(F2)
            D2, _ = D.union(P, keep)
        except Exception:
            for r in made:
                r.close()
            raise
        for r in (P, New, Diff, Imp, Pi, F, D):
            r.close()
        F, D = F2, D2
    return D, F


def _semiring_paths(rows, cols, n, sources, weights, directed, max_iter, dtype, ctx, add, mul, better, keep, start, absent):
    ctx, device, dtype, n, rowptr, ci, va = _paths_setup(rows, cols, n, weights, directed, keep, dtype, ctx)
    src = _check_sources(sources, n)
    S = int(src.size)
    tdt = _torch_dtype(dtype)
    out = torch.full((S, n), absent, dtype=tdt, device=device)
    info = _paths_info()
    if S == 0 or n == 0:
        return out.cpu().numpy(), info
    s_dev = torch.as_tensor(src, device=device)
    out.view(-1)[torch.arange(S, dtype=torch.int64, device=device) * n + s_dev] = start
    if ci.numel() == 0:
        return out.cpu().numpy(), info
    max_iter = n if max_iter is None else int(max_iter)
    from .sparse_util import _result_as_input
    rp0 = torch.arange(S + 1, dtype=torch.int64, device=device)
    c0, v0 = s_dev.to(torch.int32), torch.full((S,), start, dtype=tdt, device=device)
    W = D = F = None
    try:
        W = _csr_result(ctx, dtype, n, n, rowptr, ci, va, device)
        D = _csr_result(ctx, dtype, S, n, rp0, c0, v0, device)
        F = _csr_result(ctx, dtype, S, n, rp0, c0, v0, device)
        D, F = _relax_rounds(W, D, F, add, mul, better, keep, max_iter, info)
        a = _result_as_input(D, device)
        out.view(-1)[a.rows.to(torch.int64)[:a.nnz] * n + a.cols.to(torch.int64)] = a.vals
        torch.cuda.synchronize(device)   # torch holds views of D's arrays: nothing of it is in flight when they go back to the pool
        del a
    finally:
        _close_all(device, (W, D, F))
    return out.cpu().numpy(), info


def shortest_paths(rows, cols, n=None, sources=(0,), *, weights=None, directed=False, max_iter=None, dtype=np.float64, ctx=None):
    """Single-source shortest paths from every vertex of ``sources`` at once on the graph with edges (rows[e], cols[e]) of
    weight weights[e] >= 0 on vertices [0, n): a frontier Bellman-Ford under the (MIN, PLUS) semiring, every step on the GPU.
    D (the distances) and F (the frontier) start as the sources with value 0 and are CSR results with one row per source; a
    round is ``P = F.mxm(W, "min", "plus")``, the entries of P that are new or smaller than D's are the next frontier, and
    ``D = D.union(P, "min")`` (``_relax_rounds``).  The loop ends when the frontier is empty, after at most ``max_iter``
    rounds (default n).  ``weights=None`` means 1.0: hop counts.  ``directed=False`` uses every edge in both directions;
    duplicate edges keep the smallest weight, self loops are dropped; a negative (or NaN) weight is a ValueError.

    Returns (dist, info): ``dist`` [len(sources), n] of ``dtype``, +inf where unreachable; ``info`` = rounds and per round the
    lists frontier_nnz, nnz_product, products, ms_product (device time of the product).  A path's length is summed from the
    source outwards, one IEEE addition per edge."""
    return _semiring_paths(rows, cols, n, sources, weights, directed, max_iter, dtype, ctx, "min", "plus", "lt", "min", 0.0, float("inf"))


def widest_paths(rows, cols, n=None, sources=(0,), *, weights=None, directed=False, max_iter=None, dtype=np.float64, ctx=None):
    """Widest (maximum-bottleneck) paths from every vertex of ``sources`` at once: ``shortest_paths``' rounds under the
    (MAX, MIN) semiring.  A path's width is the smallest weight on it; a source starts at +inf, an entry of P replaces D's
    when it is larger, ``D = D.union(P, "max")``.  Duplicate edges keep the largest weight.

    Returns (width, info): ``width`` [len(sources), n] of ``dtype``, 0 where unreachable and +inf at the source; ``info`` as
    ``shortest_paths``."""
    return _semiring_paths(rows, cols, n, sources, weights, directed, max_iter, dtype, ctx, "max", "min", "gt", "max", float("inf"), 0.0)


def min_plus_closure(rows, cols, n=None, *, weights=None, dtype=np.float64, ctx=None):
    """All-pairs distances of a SMALL undirected graph as a CSR result, by repeated squaring under (MIN, PLUS): D starts as
    W with a zero diagonal, a round is ``D = D.union(D.mxm(D, "min", "plus"), "min")``, and the rounds end when D's nnz and
    its row sums (``reduce``) no longer change, after at most ceil(log2 n) of them.  D[i, j] exists iff j is reachable from
    i.  Memory is QUADRATIC in the size of a connected component: this is for graphs of a few thousand vertices.  Weights
    as ``shortest_paths``.  Returns the CsrResult (the caller closes it); its ``rounds`` attribute is the number of
    squarings."""
    ctx, device, dtype, n, rowptr, ci, va = _paths_setup(rows, cols, n, weights, False, "min", dtype, ctx)
    tdt = _torch_dtype(dtype)
    rpi = torch.arange(n + 1, dtype=torch.int64, device=device)
    ident = (rpi, torch.arange(n, dtype=torch.int32, device=device), torch.zeros(n, dtype=tdt, device=device))
    if n == 0:
        raise ValueError("the graph has no vertex")
    D = _csr_result(ctx, dtype, n, n, *ident, device)
    D.rounds = 0
    if ci.numel() == 0:
        return D
    try:
        W = _csr_result(ctx, dtype, n, n, rowptr, ci, va, device)
        try:
            D0, _ = W.union(D, "min")
        finally:
            W.close()
        D.close()
        D = D0
        D.rounds = 0
        sums, _ = D.reduce("rows", "plus")
        for _ in range(int(np.ceil(np.log2(n))) if n > 1 else 0):
            P, _ = D.mxm(D, "min", "plus")
            try:
                D2, _ = D.union(P, "min")
            finally:
                P.close()
            D2.rounds = D.rounds + 1
            sums2, _ = D2.reduce("rows", "plus")
            same = D2.nnz == D.nnz and np.array_equal(sums2.view(np.uint8), sums.view(np.uint8))
            D.close()
            D, sums = D2, sums2.copy()
            if same:
                break
    except Exception:
        D.close()
        raise
    return D


# ---- directed graphs on the transpose of a result (osp_csr_transpose) ---------------------------------

def _scc_info():
    return {"rounds_forward": 0, "rounds_backward": 0, "nnz_forward": 0, "nnz_backward": 0, "ms_transpose": 0.0, "path": 0}


def strongly_connected(rows, cols, n=None, sources=(0,), *, max_iter=None, ctx=None):
    """For every vertex s of ``sources`` the vertices of s's strongly connected component in the DIRECTED graph with edges
    (rows[e], cols[e]) on vertices [0, n), every step on the GPU.  W is the directed unit-weight adjacency as a CSR result;
    the relaxation rounds of ``shortest_paths`` (``_relax_rounds``, (MIN, PLUS)) run forwards on W and backwards on
    ``W.transpose()``, and the members are the coordinates BOTH distance results hold (``intersect``): the vertices s reaches
    that reach s.  Each direction takes at most ``max_iter`` rounds (default n); fewer rounds than the component's diameter
    cut it short.  Duplicate edges and self loops are allowed.

    Returns (member, info): ``member`` bool [len(sources), n], a source always in its own component; ``info`` =
    rounds_forward, rounds_backward, nnz_forward, nnz_backward (the entries of the two distance results), ms_transpose and
    path (the transpose's: 0 nothing launched, 1 row mask, 2 sort)."""
    dtype = np.float64
    ctx, device, dtype, n, rowptr, ci, va = _paths_setup(rows, cols, n, None, True, "min", dtype, ctx)
    src = _check_sources(sources, n)
    S = int(src.size)
    info = _scc_info()
    out = torch.zeros((S, n), dtype=torch.bool, device=device)
    if S == 0 or n == 0:
        return out.cpu().numpy(), info
    s_dev = torch.as_tensor(src, device=device)
    out.view(-1)[torch.arange(S, dtype=torch.int64, device=device) * n + s_dev] = True
    if ci.numel() == 0:
        return out.cpu().numpy(), info
    max_iter = n if max_iter is None else int(max_iter)
    from .sparse_util import _result_as_input
    tdt = _torch_dtype(dtype)
    rp0 = torch.arange(S + 1, dtype=torch.int64, device=device)
    c0, v0 = s_dev.to(torch.int32), torch.zeros(S, dtype=tdt, device=device)
    held, dist = [], {}
    try:
        W = _csr_result(ctx, dtype, n, n, rowptr, ci, va, device)
        held.append(W)
        Wt, st = W.transpose()
        held.append(Wt)
        info["ms_transpose"], info["path"] = st["ms_total"], st["path"]
        for side, graph in (("forward", W), ("backward", Wt)):
            D = _csr_result(ctx, dtype, S, n, rp0, c0, v0, device)
            F = _csr_result(ctx, dtype, S, n, rp0, c0, v0, device)
            rounds = _paths_info()
            D, F = _relax_rounds(graph, D, F, "min", "plus", "lt", "min", max_iter, rounds)   # (closes what it replaces)
            F.close()
            held.append(D)
            dist[side] = D
            info["rounds_" + side], info["nnz_" + side] = rounds["rounds"], D.nnz
        both, _ = dist["forward"].intersect(dist["backward"], "first")
        held.append(both)
        a = _result_as_input(both, device)
        out.view(-1)[a.rows.to(torch.int64)[:a.nnz] * n + a.cols.to(torch.int64)] = True
        torch.cuda.synchronize(device)   # torch holds views of the result's arrays: nothing of it is in flight when they go back to the pool
        del a
    finally:
        _close_all(device, held)
    return out.cpu().numpy(), info


def _directed_pattern_result(rows, cols, n, dtype, ctx):
    """``directed_pattern`` as a CSR result with unit values of ``dtype`` (the context first: without a GPU this is where the
    callers fail).  Returns (ctx, A)."""
    ctx, device, dtype = _setup(dtype, ctx)
    n, rowptr, colidx, vals = directed_pattern(rows, cols, n, device)
    nnz = int(colidx.numel())
    # (an edgeless graph: arrays of one unused element, a pointer is never null)
    ci = colidx.to(torch.int32) if nnz else torch.zeros(1, dtype=torch.int32, device=device)
    va = vals.to(_torch_dtype(dtype)) if nnz else torch.ones(1, dtype=_torch_dtype(dtype), device=device)
    # a count is at most a vertex's degree
    if dtype == np.float32 and nnz and max(int((rowptr[1:] - rowptr[:-1]).max().item()), int(torch.bincount(colidx).max().item())) >= 1 << 24:
        raise ValueError("float32 holds the counts exactly only while the maximum degree is below 2^24: use float64")
    return ctx, _csr_result(ctx, dtype, n, n, rowptr, ci, va, device)


def cocitation(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The co-citation counts of the DIRECTED graph with edges (rows[e], cols[e]) on vertices [0, n): C = A^T A without its
    diagonal, A the deduplicated 0/1 adjacency (self loops kept), so C[u, v] = the number of vertices with an edge to both
    u and v.  ``A.matmul(A, self_transposed=True)`` -- A's CSR arrays are the CSC of A^T, nothing is transposed -- then
    ``select("offdiag")``.  Returns the CsrResult (the caller closes it); the counts are small integers, exact in both
    dtypes."""
    ctx, A = _directed_pattern_result(rows, cols, n, dtype, ctx)
    try:
        P = A.matmul(A, self_transposed=True)
    finally:
        A.close()
    try:
        return P.select("offdiag")[0]
    finally:
        P.close()


def bibliographic_coupling(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The bibliographic coupling counts of the DIRECTED graph: B = A A^T without its diagonal, A as in ``cocitation``, so
    B[u, v] = the number of vertices both u and v have an edge to.  One ``At = A.transpose()`` on the device, then
    ``A.matmul(At)`` and ``select("offdiag")``.  Returns the CsrResult (the caller closes it)."""
    ctx, A = _directed_pattern_result(rows, cols, n, dtype, ctx)
    At = None
    try:
        At, _ = A.transpose()
        P = A.matmul(At)
    finally:
        A.close()
        if At is not None:
            At.close()
    try:
        return P.select("offdiag")[0]
    finally:
        P.close()


# ---- a result times a dense vector (osp_csr_mxv): global PageRank, connected components ---------------------------------------------
def _pattern_result(rows, cols, n, directed, dtype, ctx):
    """The 0/1 pattern of an edge list as a CSR result with unit values of ``dtype``: ``_directed_pattern_result`` (self
    loops kept) for a directed graph, ``symmetric_adjacency`` (a simple graph: no self loops) for an undirected one.
    Returns (ctx, device, dtype, n, A); A is None when the graph has no edge."""
    if directed:
        ctx, A = _directed_pattern_result(rows, cols, n, dtype, ctx)
        n, dtype = A.shape[0], A.dtype
        if A.nnz == 0:
            A.close()
            A = None
        return ctx, torch.device("cuda", ctx.device), dtype, n, A
    ctx, device, dtype, adj = _truss_setup(rows, cols, n, dtype, ctx)
    return ctx, device, dtype, adj.n, _adjacency_result(ctx, adj, dtype, device) if adj.nnz else None


def pagerank(rows, cols, n=None, *, alpha=0.85, tol=1e-6, max_iter=100, directed=False, dtype=np.float64, ctx=None):
    """The PageRank of every vertex of the graph with edges (rows[e], cols[e]) on vertices [0, n) (duplicates allowed;
    ``directed=False``: any direction, self loops dropped; ``directed=True``: self loops kept): the power iteration of
    ``networkx.pagerank`` without weights or personalisation, the matrix step on the GPU.  Once:
    deg = A.reduce("rows", "count") and, for a directed graph, At = A.transpose() (an undirected A is its own transpose).
    Per iteration  s = r / deg (0 where deg == 0);  y = At.mxv(s);  r' = alpha (y + dangling / n) + (1 - alpha) / n  with
    dangling = the sum of r over the vertices of degree 0; it stops when the L1 norm of r' - r is below n tol.  torch
    touches the length-n vectors only, with one synchronisation per iteration (the stop test).

    Returns (rank numpy[n] of ``dtype``, info): info = iterations, converged, err (the last L1 change), nnz, ms_mxv (a list:
    device time per iteration), launches (kernels of all mxv calls).  n == 0 and a graph without edges (uniform rank) launch
    nothing."""
    ctx, device, dtype, n, A = _pattern_result(rows, cols, n, directed, dtype, ctx)
    info = {"iterations": 0, "converged": False, "err": 0.0, "nnz": 0, "ms_mxv": [], "launches": 0}
    if A is None:
        info["converged"] = True
        return np.full(n, 1.0 / n if n else 0.0, dtype), info
    td = _torch_dtype(dtype)
    At = None
    try:
        info["nnz"] = A.nnz
        deg = torch.empty(n, dtype=td, device=device)
        _degrees(A, deg, device)
        At = A.transpose()[0] if directed else A
        has, zero = deg > 0, torch.zeros((), dtype=td, device=device)
        r = torch.full((n,), 1.0 / n, dtype=td, device=device)
        s = torch.where(has, r / deg, zero)
        y = torch.empty(n, dtype=td, device=device)
        torch.cuda.synchronize(device)   # the library works on its own stream
        for _ in range(max_iter):
            _, st = At.mxv(s, out=y)
            dangling = r[~has].sum()
            new = alpha * (y + dangling / n) + (1.0 - alpha) / n
            s = torch.where(has, new / deg, zero)   # (the next step's input, before the one synchronisation)
            err = float((new - r).abs().sum().item())
            r = new
            info["iterations"] += 1
            info["err"] = err
            info["ms_mxv"].append(st["ms_total"])
            info["launches"] += st["launches"]
            if err < n * tol:
                info["converged"] = True
                break
        return r.cpu().numpy(), info
    finally:
        _close_all(device, (A, At))   # (an undirected At is A: closing twice is closing once)


def connected_components(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The connected components of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n) (any direction,
    duplicates and self loops allowed): ``labels[v]`` is the smallest vertex id of v's component.  Labels start as the
    vertices' own ids, held as values of ``dtype``; a ROUND is  y = A.mxv(l, "min", "second")  (the smallest label among a
    vertex's neighbours; A's values are never read),  l' = minimum(l, y),  and one pointer jump  l' = l'[l'];  it ends with
    the first round that changes nothing.  float32 holds ids exactly up to 2^24 only: a larger n is refused.

    Returns (labels int64 numpy[n], info): info = rounds, components, ms_mxv (a list: device time per round), launches."""
    ctx = ctx or _S.default_context()
    if np.dtype(dtype) == np.float32 and n is not None and int(n) > 1 << 24:
        raise ValueError("float32 holds vertex ids exactly only up to n = 2^24: use float64")
    ctx, device, dtype, n, A = _pattern_result(rows, cols, n, False, dtype, ctx)
    if dtype == np.float32 and n > 1 << 24:
        if A is not None:
            A.close()
        raise ValueError("float32 holds vertex ids exactly only up to n = 2^24: use float64")
    info = {"rounds": 0, "components": n, "ms_mxv": [], "launches": 0}
    if A is None:
        return np.arange(n, dtype=np.int64), info
    td = _torch_dtype(dtype)
    try:
        lab = torch.arange(n, dtype=td, device=device)
        y = torch.empty(n, dtype=td, device=device)
        torch.cuda.synchronize(device)   # the library works on its own stream
        while True:
            _, st = A.mxv(lab, "min", "second", out=y)
            new = torch.minimum(lab, y)
            new = new[new.long()]
            info["rounds"] += 1
            info["ms_mxv"].append(st["ms_total"])
            info["launches"] += st["launches"]
            same = torch.equal(new, lab)   # (the round's one synchronisation)
            lab = new
            if same:
                break
        labels = lab.long().cpu().numpy()
    finally:
        _close_all(device, [A])
    info["components"] = int((labels == np.arange(n)).sum())
    return labels, info


# ---- the submatrix of a result (osp_csr_extract): induced subgraphs as matrices of their own ---------------------------------------
def _check_vertices(vertices, n):
    vs = np.atleast_1d(np.asarray(vertices.cpu() if torch.is_tensor(vertices) else vertices)).astype(np.int64).ravel()
    if vs.size and (vs.min() < 0 or vs.max() >= n):
        raise ValueError(f"vertices must lie in [0, {n})")
    if np.unique(vs).size != vs.size:
        raise ValueError("vertices must be distinct")
    return vs


def induced_subgraph(rows, cols, n=None, vertices=(), *, directed=False, dtype=np.float64, ctx=None):
    """The subgraph that ``vertices`` induce in the graph with edges (rows[e], cols[e]) on vertices [0, n), renumbered by
    position in ``vertices``: vertex ``vertices[i]`` is vertex i of the subgraph.  ``vertices`` must be distinct (a duplicate
    is a ValueError) and may come in any order.  The pattern is built as ``pagerank`` builds it (``directed=False``: a simple
    graph, any direction, self loops dropped; ``directed=True``: self loops kept) and cut out on the GPU by
    ``A.extract(vertices, vertices)``: a small matrix of its own, not ``select_vertices``' empty rows and columns.

    Returns (u, v, info): the subgraph's edges in the new numbering, int64, ascending by (u, v) -- once each with u < v for
    an undirected graph, every edge u -> v for a directed one; info = the extract's stats (nnz_in, nnz_gathered, nnz_out,
    ms_total, launches, readbacks, composed) and n (the number of vertices of the subgraph)."""
    ctx, device, dtype, n, A = _pattern_result(rows, cols, n, directed, dtype, ctx)
    try:
        vs = _check_vertices(vertices, n)
        info = dict(_S._lib.ExtractStats().as_dict(), composed=False, n=int(vs.size))
        none = np.zeros(0, np.int64)
        if A is None:
            return none, none.copy(), info
        sub, st = A.extract(vs, vs, space="host")
        info.update(st)
        try:
            if not directed:
                u, v, _ = _upper_entries(sub)
                return u, v, info
            rowptr, colidx, _ = sub.to_host()
            return np.repeat(np.arange(sub.shape[0], dtype=np.int64), np.diff(rowptr)), colidx.astype(np.int64), info
        finally:
            sub.close()
    finally:
        if A is not None:
            A.close()


def ego_network(rows, cols, n=None, center=0, radius=1, *, ctx=None):
    """The ego network of ``center`` in the undirected graph with edges (rows[e], cols[e]) on vertices [0, n)
    (``networkx.ego_graph``): the vertices within ``radius`` steps of ``center`` -- from ``bfs_levels(...,
    max_levels=radius)`` -- ascending, and the subgraph they induce, by ``induced_subgraph``.

    Returns (vertices int64, u, v, info): the edges in the numbering of ``vertices`` (vertex ``vertices[i]`` is i), u < v,
    ascending; info = ``induced_subgraph``'s and levels (the deepest level the search reached)."""
    radius = int(radius)
    if radius < 0:
        raise ValueError("radius must be at least 0")
    level, _, binfo = bfs_levels(rows, cols, n, [center], max_levels=radius, ctx=ctx)
    vertices = np.flatnonzero(level[0] >= 0).astype(np.int64)
    u, v, info = induced_subgraph(rows, cols, level.shape[1], vertices, ctx=ctx)
    info["levels"] = binfo["levels"]
    return vertices, u, v, info


def largest_component(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The largest connected component of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n) as a graph
    of its own: the labels of ``connected_components``, the most frequent label (the smallest on a tie) counted with torch,
    and the subgraph its vertices induce, by ``induced_subgraph``.

    Returns (vertices int64 ascending, u, v, info): the edges in the numbering of ``vertices``, u < v, ascending; info =
    ``induced_subgraph``'s, components and rounds (of ``connected_components``)."""
    labels, cinfo = connected_components(rows, cols, n, dtype=dtype, ctx=ctx)
    nn = len(labels)
    if nn:
        counts = torch.bincount(torch.as_tensor(labels))
        best = int((counts == counts.max()).nonzero()[0].item())   # (the first of the most frequent: the smallest label)
        vertices = np.flatnonzero(labels == best).astype(np.int64)
    else:
        vertices = np.zeros(0, np.int64)
    u, v, info = induced_subgraph(rows, cols, nn, vertices, dtype=dtype, ctx=ctx)
    info["components"], info["rounds"] = cinfo["components"], cinfo["rounds"]
    return vertices, u, v, info


# ---- a result from an edge list (osp_csr_build): adjacency, Laplacian, incidence matrix, line graph --------------------------------
def _build_device(ctx, device, n_rows, n_cols, r, c, w, dup, dtype):
    """``ctx.build`` of int64 index tensors (and a value tensor or None) that live on the device."""
    r32, c32 = r.to(torch.int32).contiguous(), c.to(torch.int32).contiguous()   # (the low 32 bits: a uint32 list's bits)
    w = w.contiguous() if w is not None else None
    torch.cuda.synchronize(device)   # the library works on its own stream
    return ctx.build(n_rows, n_cols, r32, c32, w, dup=dup, dtype=dtype, space="device")[0]


def adjacency_matrix(rows, cols, n=None, weights=None, *, directed=False, loops=False, dup="min", dtype=np.float64, ctx=None):
    """The n x n adjacency matrix of the graph with edges (rows[e], cols[e]) on vertices [0, n) as a CSR result, in ONE
    ``osp_csr_build``: the edge list -- for an undirected graph (``directed=False``) followed by its mirrored copy -- with
    parallel edges combined by ``dup`` in list order (``Context.build``'s operators; ``"count"`` gives multiplicities).
    ``weights=None`` means 1 for every edge.  Self loops are masked out unless ``loops`` (an undirected loop is then listed
    twice, as every edge is).  An edgeless graph gives an empty n x n result.  The caller closes the result."""
    ctx, device, dtype = _setup(dtype, ctx)
    _, n, r, c, w = _edges(rows, cols, n, device, weights, _torch_dtype(dtype))
    if not loops:
        keep = r != c
        r, c = r[keep], c[keep]
        w = w[keep] if w is not None else None
    if not directed:
        r, c = torch.cat([r, c]), torch.cat([c, r])
        w = torch.cat([w, w]) if w is not None else None
    return _build_device(ctx, device, n, n, r, c, w, dup, dtype)


def laplacian(rows, cols, n=None, weights=None, *, dtype=np.float64, ctx=None):
    """The Laplacian L = D - A of the UNDIRECTED graph with edges (rows[e], cols[e]) on vertices [0, n) as a CSR result:
    self loops are dropped, parallel edges add.  ONE ``osp_csr_build`` with ``dup="plus"`` of the four blocks (u, v, -w),
    (v, u, -w), (u, u, w), (v, v, w) concatenated in that order, which fixes every sum's order and with it its bits.  A
    vertex without an edge has an empty row.  The caller closes the result."""
    ctx, device, dtype = _setup(dtype, ctx)
    _, n, r, c, w = _edges(rows, cols, n, device, weights, _torch_dtype(dtype))
    keep = r != c
    u, v = r[keep], c[keep]
    w = w[keep] if w is not None else torch.ones(u.numel(), dtype=_torch_dtype(dtype), device=device)
    return _build_device(ctx, device, n, n, torch.cat([u, v, u, v]), torch.cat([v, u, u, v]), torch.cat([-w, -w, w, w]), "plus", dtype)


def incidence_matrix(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The unoriented incidence matrix of the UNDIRECTED simple graph of an edge list (self loops dropped, parallel edges
    one): the distinct edges {u, v}, u < v, ascending by (u, v), are the edge ids, and B is n x m with B[u, e] = B[v, e] = 1.
    ``adjacency_matrix``, its entries above the diagonal (``select("triu", diag=1)``), then one build.  Returns (B, u, v):
    the CsrResult (the caller closes it) and the edges' ends as int64 arrays on the host."""
    A = adjacency_matrix(rows, cols, n, dtype=dtype, ctx=ctx)
    try:
        u, v, _ = _upper_entries(A)
        n, ctx = A.shape[0], A._ctx
    finally:
        A.close()
    e = np.arange(u.size, dtype=np.int64)
    B, _ = ctx.build(n, u.size, np.concatenate([u, v]), np.concatenate([e, e]), None, dup="error", dtype=A.dtype, space="host")
    return B, u, v


def line_graph(rows, cols, n=None, *, dtype=np.float64, ctx=None):
    """The line graph of the UNDIRECTED simple graph of an edge list: vertex e is edge e of ``incidence_matrix``, and two are
    adjacent when the edges share an end.  ``B.matmul(B, self_transposed=True)`` -- B^T B: the number of shared ends -- then
    ``select("offdiag")``, as ``cocitation`` does.  Returns (L, u, v): the m x m CsrResult with unit values (the caller closes
    it) and the edges' ends."""
    B, u, v = incidence_matrix(rows, cols, n, dtype=dtype, ctx=ctx)
    try:
        if u.size == 0:   # (no edge: nothing to multiply)
            return B._ctx.build(0, 0, [], [], dtype=B.dtype)[0], u, v
        P = B.matmul(B, self_transposed=True)
    finally:
        B.close()
    try:
        return P.select("offdiag")[0], u, v
    finally:
        P.close()


# ---- a result times a dense matrix (osp_csr_mxd): label spreading, feature propagation ---------------------------------------------
def _check_labels(labels, n):
    """``labels`` -- a dict vertex -> class, or a sequence of n class ids with a negative id for "unlabelled" -- as (vertices
    int64, column of each int64, classes): ``classes`` are the distinct classes in ascending order, one column of F each."""
    if isinstance(labels, dict):
        verts = np.fromiter(labels.keys(), np.int64, len(labels))
        vals = list(labels.values())
    else:
        a = np.asarray(labels)
        if a.shape != (n,):
            raise ValueError(f"labels must be a dict or hold one class id per vertex ({n})")
        verts = np.flatnonzero(a >= 0).astype(np.int64)
        vals = a[verts].tolist()
    if verts.size == 0:
        raise ValueError("no vertex is labelled")
    if verts.min() < 0 or verts.max() >= n:
        raise ValueError(f"labelled vertices must lie in [0, {n})")
    classes = sorted(set(vals))
    column = {c: i for i, c in enumerate(classes)}
    return verts, np.array([column[v] for v in vals], np.int64), classes


def _normalised(A, device, td):
    """D^-1/2 A D^-1/2 of the CSR result A as a new result, D its entries per row (``reduce("rows", "count")``; a count of 0
    counts as 1) in ONE ``apply_vectors``.  Returns (S, maximum count)."""
    n = A.shape[0]
    deg = torch.empty(n, dtype=td, device=device)
    _degrees(A, deg, device)
    d = torch.clamp(deg, min=1.0).sqrt().reciprocal()
    maxdeg = int(deg.max().item())   # (synchronises: d is ready for the library's stream)
    return A.apply_vectors(rows=d, row_op="times", cols=d, col_op="times")[0], maxdeg


def label_spreading(rows, cols, n=None, labels=None, *, alpha=0.99, max_iter=30, dtype=np.float64, ctx=None):
    """Zhou et al.'s learning with local and global consistency on the undirected simple graph with edges (rows[e], cols[e])
    on vertices [0, n) (any direction, duplicates and self loops dropped), as ``networkx``'s
    ``node_classification.local_and_global_consistency`` iterates it: S = D^-1/2 A D^-1/2 (a degree of 0 counts as 1), Y0 the
    n x c indicator of ``labels`` (a dict vertex -> class, or n class ids with a negative id for "unlabelled"; the classes in
    ascending order are the columns), F = 0, and ``max_iter`` times  F <- alpha S.mxd(F) + (1 - alpha) Y0.  The matrix step is
    ONE ``osp_csr_mxd`` per iteration, every other operation is torch's on n x c tensors; nothing synchronises inside the loop
    but the call itself.

    Returns (F numpy (n, c) of ``dtype``, predicted: a list of n classes -- the class of each row's largest entry, the first
    on a tie -- and info): info = iterations, classes, nnz, max_degree, ms_mxd (a list: device time per iteration),
    launches.  n == 0 and a graph without edges launch nothing (F is then (1 - alpha) Y0 after the first step)."""
    if labels is None:
        raise ValueError("labels is required")
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1)")
    ctx, device, dtype, n, A = _pattern_result(rows, cols, n, False, dtype, ctx)
    try:
        verts, column, classes = _check_labels(labels, n)
    except Exception:
        if A is not None:
            A.close()
        raise
    info = {"iterations": 0, "classes": classes, "nnz": 0, "max_degree": 0, "ms_mxd": [], "launches": 0}
    td = _torch_dtype(dtype)
    if A is None:
        F = np.zeros((n, len(classes)), dtype)
        if max_iter > 0:
            F[verts, column] = dtype(1.0 - alpha)
        info["iterations"] = max(int(max_iter), 0)
        return F, [classes[i] for i in F.argmax(axis=1)], info
    S = None
    try:
        info["nnz"] = A.nnz
        S, info["max_degree"] = _normalised(A, device, td)
        base = torch.zeros((n, len(classes)), dtype=td, device=device)
        base[torch.as_tensor(verts, device=device), torch.as_tensor(column, device=device)] = 1.0 - alpha
        F = torch.zeros_like(base)
        Z = torch.empty_like(base)
        for _ in range(max_iter):
            torch.cuda.synchronize(device)   # the library works on its own stream
            _, st = S.mxd(F, out=Z)
            F = alpha * Z + base
            info["iterations"] += 1
            info["ms_mxd"].append(st["ms_total"])
            info["launches"] += st["launches"]
        out = F.cpu().numpy()
        return out, [classes[i] for i in out.argmax(axis=1)], info
    finally:
        _close_all(device, (A, S))


def propagate_features(rows, cols, n=None, X=None, hops=2, *, self_loops=True, dtype=np.float64, ctx=None):
    """The SGC / GCN aggregation  A^^hops X  of the n x k feature matrix ``X`` (an array-like or a torch tensor) over the
    undirected simple graph with edges (rows[e], cols[e]) on vertices [0, n):  A^ = D~^-1/2 (A + I) D~^-1/2  with D~ the row
    counts of A + I (``self_loops=True``, Kipf and Welling's renormalisation), or  D^-1/2 A D^-1/2  with a degree of 0
    counting as 1 (``self_loops=False``).  A + I is a ``build`` of the identity and a ``union``; the normalisation is
    ``reduce("rows", "count")`` and ONE ``apply_vectors``; every hop is ONE ``osp_csr_mxd`` that overwrites its iterate.

    Returns (numpy (n, k) of ``dtype``, info): info = hops, nnz (of the matrix that is applied), max_degree (its largest row
    count), ms_mxd (a list: device time per hop), launches.  n == 0 launches nothing; neither does an edgeless graph
    without self loops (the result is 0 once hops >= 1)."""
    if X is None:
        raise ValueError("X is required")
    if hops < 0:
        raise ValueError("hops must be at least 0")
    ctx, device, dtype, n, A = _pattern_result(rows, cols, n, False, dtype, ctx)
    td = _torch_dtype(dtype)
    H = S = At = eye = None
    info = {"hops": int(hops), "nnz": 0, "max_degree": 0, "ms_mxd": [], "launches": 0}
    try:
        H = (X.to(device=device, dtype=td) if torch.is_tensor(X) else torch.as_tensor(np.asarray(X, dtype), device=device)).contiguous().clone()
        if H.dim() != 2 or H.shape[0] != n:
            raise ValueError(f"X must have shape ({n}, k)")
        if n == 0 or H.shape[1] == 0 or hops == 0:
            return H.cpu().numpy(), info
        if self_loops:
            diag = torch.arange(n, dtype=torch.int64, device=device)
            eye = _build_device(ctx, device, n, n, diag, diag, None, "error", dtype)
            At = A.union(eye)[0] if A is not None else eye
        else:
            At = A
        if At is None:   # (no edge and no self loop: the matrix is 0)
            return np.zeros(tuple(H.shape), dtype), info
        info["nnz"] = At.nnz
        S, info["max_degree"] = _normalised(At, device, td)
        for _ in range(hops):
            torch.cuda.synchronize(device)   # the library works on its own stream
            _, st = S.mxd(H, out=H)
            info["ms_mxd"].append(st["ms_total"])
            info["launches"] += st["launches"]
        return H.cpu().numpy(), info
    finally:
        _close_all(device, (A, eye, At, S))   # (At may be A or eye: closing twice is closing once)


# ---- dense x dense on a result's pattern (osp_csr_sddmm): edge scores, landmark bounds, factorisation -------------------------------
def _dense_on_device(X, rows, device, td, what):
    """``X`` (an array-like or a torch tensor) as a contiguous (rows, k) tensor of ``td`` on the device."""
    T = (X.to(device=device, dtype=td) if torch.is_tensor(X) else torch.as_tensor(np.asarray(X), device=device).to(td)).contiguous()
    if T.dim() != 2 or T.shape[0] != rows:
        raise ValueError(f"{what} must have shape ({rows}, k)")
    return T


def _result_coo(E):
    """(u, v, values) of the CSR result E on the host, ascending by (u, v)."""
    rowptr, colidx, vals = E.to_host()
    return np.repeat(np.arange(E.shape[0], dtype=np.int64), np.diff(rowptr)), colidx.astype(np.int64), vals


def _inverse_norms(T, td):
    """1 / ||row|| of every row of T, the norm taken in float64 and a norm of 0 counting as 1, as a tensor of ``td``."""
    nrm = T.double().pow(2).sum(dim=1).sqrt()
    return (1.0 / torch.where(nrm == 0, torch.ones_like(nrm), nrm)).to(td)


def edge_scores(rows, cols, n=None, X=None, Y=None, kind="dot", directed=False, *, dtype=np.float64, ctx=None):
    """A score per edge of the graph with edges (rows[e], cols[e]) on vertices [0, n) from the vertex embeddings ``X`` (n x k)
    and ``Y`` (n x k; None: X): ``kind="dot"`` is  X[u] . Y[v],  ``"cosine"`` that divided by ||X[u]|| ||Y[v]|| (a norm of 0
    counts as 1, so the score is 0).  The pattern is deduplicated as ``pagerank`` does it (``directed=True``: self loops kept;
    ``directed=False``: a simple graph, every edge once with u < v: ``select("triu", diag=1)`` of the symmetric pattern); the
    dot products are ONE ``osp_csr_sddmm`` on it, in ``reduce``'s bit-defined order; the cosine is ONE ``apply_vectors`` of the
    inverse norms after it.  The norms (taken in float64) are torch's.

    Returns (u, v, score, info): the edges ascending by (u, v) as int64 arrays, the scores as a numpy array of ``dtype``;
    info = nnz, k, launches, ms_sddmm, ms_apply.  n == 0 and a graph without edges launch nothing."""
    if kind not in ("dot", "cosine"):
        raise ValueError('kind must be "dot" or "cosine"')
    if X is None:
        raise ValueError("X is required")
    ctx, device, dtype, n, A = _pattern_result(rows, cols, n, directed, dtype, ctx)
    td = _torch_dtype(dtype)
    info = {"nnz": 0, "k": 0, "launches": 0, "ms_sddmm": 0.0, "ms_apply": 0.0}
    P = E = Z = None
    try:
        Xd = _dense_on_device(X, n, device, td, "X")
        Yd = Xd if Y is None else _dense_on_device(Y, n, device, td, "Y")
        if Yd.shape[1] != Xd.shape[1]:
            raise ValueError("X and Y must have the same number of columns")
        info["k"] = int(Xd.shape[1])
        if A is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, dtype), info
        P = A if directed else A.select("triu", diag=1)[0]
        info["nnz"] = P.nnz
        rx = ry = None
        if kind == "cosine":
            rx = _inverse_norms(Xd, td)
            ry = rx if Yd is Xd else _inverse_norms(Yd, td)
        torch.cuda.synchronize(device)   # the library works on its own stream
        E, st = P.sddmm(Xd, Yd)
        info["launches"], info["ms_sddmm"] = st["launches"], st["ms_total"]
        if kind == "cosine":
            Z, st = E.apply_vectors(rows=rx, row_op="times", cols=ry, col_op="times")
            info["launches"] += st["launches"]
            info["ms_apply"] = st["ms_total"]
        u, v, score = _result_coo(Z if Z is not None else E)
        return u, v, score.copy(), info
    finally:
        _close_all(device, (A, P, E, Z))   # (a directed P is A: closing twice is closing once)


def landmark_bounds(rows, cols, n=None, landmarks=(0,), pairs=(), weights=None, *, dtype=np.float64, ctx=None):
    """The landmark (triangle-inequality) upper bound  min_c d(c, u) + d(c, v)  of the distance of every vertex pair (u, v) of
    ``pairs`` (a list of pairs, or an array of shape (q, 2); a pair may repeat) on the undirected graph ``shortest_paths``
    reads from (rows, cols, weights), c running over ``landmarks``:  d = shortest_paths(.., landmarks)  is k x n,
    D = d.T  is n x k, the distinct pairs are a pattern (``Context.build`` with ``dup="first"``), and
    ``P.sddmm(D, D, "min", "plus")`` is the bound per pair, one IEEE addition per landmark and the minimum of those.

    Returns (bound, info): ``bound`` numpy[q] of ``dtype`` in the callers' pair order, +inf where no landmark reaches both
    ends (and for every pair when there is no landmark); info = landmarks, pairs, distinct_pairs, launches, ms_sddmm and
    ``paths``, the info of ``shortest_paths``."""
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    d, pinfo = shortest_paths(rows, cols, n, landmarks, weights=weights, dtype=dtype, ctx=ctx)
    dtype, (k, n) = d.dtype.type, d.shape
    if pr.size and (pr.min() < 0 or pr.max() >= n):
        raise ValueError(f"pairs must lie in [0, {n})")
    info = {"landmarks": int(k), "pairs": int(len(pr)), "distinct_pairs": 0, "launches": 0, "ms_sddmm": 0.0, "paths": pinfo}
    if len(pr) == 0:
        return np.zeros(0, dtype), info
    ctx, device, dtype = _setup(dtype, ctx)
    P = E = None
    try:
        D = torch.as_tensor(np.ascontiguousarray(d.T), device=device)
        P, _ = ctx.build(n, n, pr[:, 0], pr[:, 1], None, dup="first", dtype=dtype, space="host")
        info["distinct_pairs"] = P.nnz
        torch.cuda.synchronize(device)   # the library works on its own stream
        E, st = P.sddmm(D, D, "min", "plus")
        info["launches"], info["ms_sddmm"] = st["launches"], st["ms_total"]
        u, v, bound = _result_coo(E)
        return bound[np.searchsorted(u * n + v, pr[:, 0] * n + pr[:, 1])], info
    finally:
        _close_all(device, (P, E))


def factorize(rows, cols, vals, shape, rank, steps, lr, reg=0.0, U0=None, V0=None, seed=0, dup="error", *, dtype=np.float64, ctx=None):
    """A rank-``rank`` factorisation  S ~ U V^T  of the M x N sparse matrix with the observed entries (rows[t], cols[t],
    vals[t]) (``shape`` = (M, N); repeats combined by ``dup``, ``Context.build``'s operators) by ``steps`` steps of gradient
    descent on  1/2 sum e^2 + reg/2 (|U|^2 + |V|^2)  over the OBSERVED entries, everything sparse on the GPU.  A step is
    ``E = S.sddmm(U, V, accum="minus")``  (e = s - u.v on S's pattern),  ``gU = E.mxd(V)``,  ``gV = E.transpose().mxd(U)``,
    then  U += lr (gU - reg U)  and  V += lr (gV - reg V),  both from the old U and V; the dense updates are torch's.
    ``U0`` (M x rank) and ``V0`` (N x rank) default to  numpy.random.default_rng(seed).standard_normal / sqrt(rank),  U first.

    Returns (U numpy (M, rank), V numpy (N, rank), info): info = nnz, steps, loss (a list: the sum of e^2 of every step's E,
    that is BEFORE the step's update, summed in float64 on the device), launches, ms_sddmm and ms_mxd (lists, per step).
    ``rank == 0``, ``steps == 0`` and an empty list are legal."""
    M, N = (int(x) for x in shape)
    rank, steps = int(rank), int(steps)
    if M < 0 or N < 0 or rank < 0 or steps < 0:
        raise ValueError("shape, rank and steps must not be negative")
    ctx, device, dtype = _setup(dtype, ctx)
    td = _torch_dtype(dtype)
    rng = np.random.default_rng(seed)
    init = [None, None]
    for i, (given, m, what) in enumerate(((U0, M, "U0"), (V0, N, "V0"))):
        a = np.asarray(given, dtype) if given is not None else (rng.standard_normal((m, rank)) / np.sqrt(max(rank, 1))).astype(dtype)
        if a.shape != (m, rank):
            raise ValueError(f"{what} must have shape ({m}, {rank})")
        init[i] = torch.as_tensor(np.ascontiguousarray(a), device=device)
    U, V = init
    from .distributed import _as_tensor
    info = {"nnz": 0, "steps": 0, "loss": [], "launches": 0, "ms_sddmm": [], "ms_mxd": []}
    S = None
    losses = []
    try:
        S, _ = ctx.build(M, N, rows, cols, vals, dup=dup, dtype=dtype, space="host")
        info["nnz"] = S.nnz
        for _ in range(steps):
            E = Et = None
            try:
                torch.cuda.synchronize(device)   # the library works on its own stream
                E, st = S.sddmm(U, V, accum="minus")
                gU, su = E.mxd(V)
                Et, _ = E.transpose()
                gV, sv = Et.mxd(U)
                e = _as_tensor(E.device_ptrs()[2], E.nnz, "<f4" if dtype == np.float32 else "<f8", device, td)
                losses.append(e.double().pow(2).sum())
                U, V = U + lr * (gU - reg * U), V + lr * (gV - reg * V)
                del e
            finally:
                _close_all(device, (E, Et))
            info["steps"] += 1
            info["launches"] += st["launches"] + su["launches"] + sv["launches"]
            info["ms_sddmm"].append(st["ms_total"])
            info["ms_mxd"].append(su["ms_total"] + sv["ms_total"])
        info["loss"] = [float(x) for x in torch.stack(losses).cpu()] if losses else []
        return U.cpu().numpy(), V.cpu().numpy(), info
    finally:
        _close_all(device, (S,))


# ---- mxv with the winner's column (osp_csr_mxv_arg): spanning forest, matching ------------------------------
def _arg_setup(rows, cols, n, weights, keep, dtype, ctx):
    """What the two functions below share: the checks of the arguments (before the context: a bad argument is a Python error
    without a GPU as well), the context (without a GPU this is where they fail), the weighted adjacency on its device with
    the weights as ``dtype`` holds them, and the guard of float32's exact range (vertex ids are held as values).  Returns
    (ctx, device, dtype, n, W): W a CSR result, None when the graph has no edge."""
    dtype = _value_dtype(dtype)
    if weights is not None:
        w = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights, np.float64)
        if np.isnan(w).any():
            raise ValueError("weights must not be NaN")
    if dtype == np.float32 and n is not None and int(n) > 1 << 24:
        raise ValueError("float32 holds vertex ids exactly only up to n = 2^24: use float64")
    ctx, device, dtype = _setup(dtype, ctx)
    n, rowptr, colidx, vals = weighted_adjacency(rows, cols, n, weights, keep=keep, device=device)
    if dtype == np.float32 and n > 1 << 24:
        raise ValueError("float32 holds vertex ids exactly only up to n = 2^24: use float64")
    if colidx.numel() == 0:
        return ctx, device, dtype, n, None
    return ctx, device, dtype, n, _csr_result(ctx, dtype, n, n, rowptr, colidx.to(torch.int32), vals.to(_torch_dtype(dtype)), device)


def minimum_spanning_forest(rows, cols, n=None, weights=None, *, dtype=np.float64, ctx=None):
    """The minimum spanning forest of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n) (any direction,
    self loops dropped, duplicate edges keep their smallest weight; ``weights=None``: 1.0 each), under the STRICT TOTAL ORDER
    on edges (w, min(u, v), max(u, v)) with w the weight as ``dtype`` holds it.  Under a strict total order the minimum
    spanning forest is unique, so the result is defined exactly, ties included: it is what Kruskal's algorithm gives on the
    edges sorted by that key.

    Boruvka, the matrix on the device in every round.  Labels l start as the vertices' own ids, held as values of ``dtype``
    (float32: n <= 2^24).  A ROUND:
      the cross edges  D = Wc.apply_vectors(rows=l, row_op="second", cols=l, col_op="minus")  (l[i] - l[j] on Wc's pattern),
      mask = D.select("ne", 0),  Wc = Wc.apply_mask(mask)  -- Wc only ever shrinks, so each round filters the previous
      round's (the first round's Wc is W: without self loops every edge is a cross edge); it stops when Wc has no entries;
      (y, arg) = Wc.mxv_arg(None, "min", "first")  -- the lightest cross edge of every vertex;
      the best edge of every component, the hooking and the pointer jumping in torch, on length-n vectors.
    ``arg[v]`` is the SMALLEST column among v's lightest cross edges, and that is v's smallest edge under the total order:
    for two neighbours j1 < j2 of v with equal weight, either j1 < j2 < v, and the keys are (j1, v) < (j2, v); or
    j1 < v < j2, and (j1, v) < (v, j2) because j1 < v; or v < j1 < j2, and (v, j1) < (v, j2).  A component's best edge is
    the smallest (y, min, max) among its vertices.  Two components may choose the same edge (it is then taken once and the
    smaller label becomes the root); under a strict order the chosen edges form no other cycle.

    Returns (u, v, w, info): the forest's edges, u < v, ascending by (u, v), int64 and ``dtype``; info = rounds,
    components (n - the number of edges), ms_mxv_arg (a list: device time per round), launches (kernels of all library
    calls).  n == 0 and a graph without edges launch nothing."""
    ctx, device, dtype, n, W = _arg_setup(rows, cols, n, weights, "min", dtype, ctx)
    info = {"rounds": 0, "components": n, "ms_mxv_arg": [], "launches": 0}
    if W is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, dtype), info
    td = _torch_dtype(dtype)
    Wc, keys, wts = W, [], []
    try:
        lab = torch.arange(n, dtype=torch.int64, device=device)
        while True:
            if info["rounds"]:
                labv = lab.to(td)
                torch.cuda.synchronize(device)   # the library works on its own stream
                D, sd = Wc.apply_vectors(rows=labv, row_op="second", cols=labv, col_op="minus")
                try:
                    mask, sm = D.select("ne", 0)
                finally:
                    D.close()
                try:
                    new, sa = Wc.apply_mask(mask)
                finally:
                    mask.close()
                info["launches"] += sd["launches"] + sm["launches"] + sa["launches"]
                if Wc is not W:
                    Wc.close()
                Wc = new
            if Wc.nnz == 0:
                break
            torch.cuda.synchronize(device)
            y, arg, st = Wc.mxv_arg(None, "min", "first")
            info["rounds"] += 1
            info["ms_mxv_arg"].append(st["ms_total"])
            info["launches"] += st["launches"]
            # the best edge of every component: the smallest y, then the smallest key min * n + max among those
            v = torch.nonzero(arg >= 0).squeeze(1)
            o, comp, yv = arg[v], lab[v], y[v]
            best = torch.full((n,), float("inf"), dtype=td, device=device)
            best.scatter_reduce_(0, comp, yv, reduce="amin", include_self=True)
            tie = yv == best[comp]
            v, o, comp, yv = v[tie], o[tie], comp[tie], yv[tie]
            key = torch.minimum(v, o) * n + torch.maximum(v, o)
            kbest = torch.full((n,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=device)
            kbest.scatter_reduce_(0, comp, key, reduce="amin", include_self=True)
            won = key == kbest[comp]
            o, comp, yv, key = o[won], comp[won], yv[won], key[won]     # one edge per component that has a cross edge
            # hooking: a component points at the one its edge leads to; of two that chose the same edge the smaller label stays a root
            parent = torch.arange(n, dtype=torch.int64, device=device)
            parent[comp] = lab[o]
            root = (parent[parent[comp]] == comp) & (comp < parent[comp])
            parent[comp[root]] = comp[root]
            keys.append(key[~root])
            wts.append(yv[~root])
            while True:   # pointer jumping
                nxt = parent[parent]
                if torch.equal(nxt, parent):
                    break
                parent = nxt
            lab = parent[lab]
        key = torch.cat(keys) if keys else torch.zeros(0, dtype=torch.int64, device=device)
        wt = torch.cat(wts) if wts else torch.zeros(0, dtype=td, device=device)
        order = torch.argsort(key)
        key, wt = key[order].cpu().numpy(), wt[order].cpu().numpy()
    finally:
        _close_all(device, (W, Wc))   # (closing twice is closing once)
    info["components"] = n - len(key)
    return key // n, key % n, wt, info


def greedy_matching(rows, cols, n=None, weights=None, *, dtype=np.float64, ctx=None):
    """The greedy weighted matching of the undirected graph with edges (rows[e], cols[e]) on vertices [0, n) (any direction,
    self loops dropped, duplicate edges keep their largest weight; ``weights=None``: 1.0 each): the matching a sequential
    pass over the edges in the STRICT TOTAL ORDER (larger w first, then min(u, v), then max(u, v)) builds, w the weight as
    ``dtype`` holds it, computed by handshake rounds with the matrix on the device.  A ROUND:
      Wf = Wf.select_vertices(free, free)  (the edges between free vertices; the first round's Wf is W); stop when it is empty;
      (y, arg) = Wf.mxv_arg(None, "max", "first")  -- every free vertex's heaviest free neighbour, the smallest id among
      ties, which is its best edge under the total order (the three cases of ``minimum_spanning_forest``);
      the pairs with arg[arg[v]] == v are matched.
    An edge is locally dominant when it is the best edge of both its ends; under a strict total order the locally dominant
    edges of every round are exactly edges the sequential greedy pass takes, and the round's best edge overall is one of
    them, so every round matches a pair and the result is the sequential one: defined exactly, and MAXIMAL (no edge has both
    ends free).  With non-negative weights its weight is at least half the optimum (Preis 1999).

    Returns (mate int64[n], info): mate[v] is v's partner, -1 for a free vertex; info = rounds, pairs, ms_mxv_arg (a list:
    device time per round), launches (kernels of all library calls).  n == 0 and a graph without edges launch nothing."""
    ctx, device, dtype, n, W = _arg_setup(rows, cols, n, weights, "max", dtype, ctx)
    info = {"rounds": 0, "pairs": 0, "ms_mxv_arg": [], "launches": 0}
    if W is None:
        return np.full(n, -1, np.int64), info
    Wf = W
    try:
        mate = torch.full((n,), -1, dtype=torch.int64, device=device)
        ids = torch.arange(n, dtype=torch.int64, device=device)
        while True:
            if info["rounds"]:
                free = (mate < 0).to(torch.uint8)
                torch.cuda.synchronize(device)   # the library works on its own stream
                new, ss = Wf.select_vertices(free, free)
                info["launches"] += ss["launches"]
                if Wf is not W:
                    Wf.close()
                Wf = new
            if Wf.nnz == 0:
                break
            torch.cuda.synchronize(device)
            _, arg, st = Wf.mxv_arg(None, "max", "first", values=False)
            info["rounds"] += 1
            info["ms_mxv_arg"].append(st["ms_total"])
            info["launches"] += st["launches"]
            has = arg >= 0
            back = arg[torch.where(has, arg, ids)]
            shake = has & (back == ids)
            mate = torch.where(shake, arg, mate)
        mate = mate.cpu().numpy()
    finally:
        _close_all(device, (W, Wf))   # (closing twice is closing once)
    info["pairs"] = int((mate >= 0).sum()) // 2
    return mate, info


# ---- the semiring product at a mask (osp_csr_mxm_masked): BFS parent trees -------------------------------------
def bfs_parents(rows, cols, n=None, sources=(0,), *, directed=False, max_levels=None, ctx=None):
    """The breadth-first parent tree of every vertex of ``sources`` at once on the graph with edges (rows[e], cols[e]) on
    vertices [0, n) (duplicates allowed; ``directed=False``: any direction, self loops dropped; ``directed=True``: an edge
    leads from rows[e] to cols[e]), every level on the GPU.  With A the 0/1 adjacency, the frontier F and the parents found
    so far P as S x n CSR results (one row per source), a level is

        Nx = F.mxm(A, "min", "first", mask=P, complement=True)     next<NOT parents> = frontier (min.first) A
        P  = P.ewise(Nx, "union", "first")                         (the patterns are disjoint)
        F  = Nx.apply_vectors(col_op="second", cols=arange(n))     an entry at (s, k) carries the value k

    so an entry of Nx at (s, v) is the smallest vertex id among v's neighbours on the previous level -- v's parent -- and a
    product that lands on a vertex already reached is dropped where it is formed: it is never sorted, folded or written.
    Ids are exact in float64.  The levels end when Nx is empty or ``max_levels`` levels were taken.

    Returns (parent int64 [len(sources), n], level int32 of the same shape, info): ``parent[s, source] = source`` and
    ``level[s, source] = 0``; an unreached vertex has parent -1 and level -1.  ``info`` = levels (the deepest level reached)
    and per product the lists frontier_nnz, products (formed), products_kept, nnz_new and ms_mxm (device time).  Duplicate
    sources are independent rows; a source out of range is a ValueError.  rows / cols: torch tensors (any device; the
    plumbing runs on cuda:ctx.device) or array-likes."""
    from .sparse_util import _result_as_input
    ctx, device, _, n, A = _pattern_result(rows, cols, n, directed, np.float64, ctx)
    F = P = None
    try:
        src = _check_sources(sources, n)
        S = int(src.size)
        parent = torch.full((S, n), -1, dtype=torch.int64, device=device)
        level = torch.full((S, n), -1, dtype=torch.int32, device=device)
        info = {"levels": 0, "frontier_nnz": [], "products": [], "products_kept": [], "nnz_new": [], "ms_mxm": []}
        if S and n:
            s_dev = torch.as_tensor(src, device=device)
            lin0 = torch.arange(S, dtype=torch.int64, device=device) * n + s_dev
            parent.view(-1)[lin0] = s_dev
            level.view(-1)[lin0] = 0
        if S and n and A is not None:
            rp0 = torch.arange(S + 1, dtype=torch.int64, device=device)
            c0, v0 = s_dev.to(torch.int32), s_dev.to(torch.float64)
            ids = torch.arange(n, dtype=torch.float64, device=device)
            torch.cuda.synchronize(device)   # the library works on its own stream
            F = _csr_result(ctx, np.float64, S, n, rp0, c0, v0, device, sync=False)
            P = _csr_result(ctx, np.float64, S, n, rp0, c0, v0, device, sync=False)
            d = 0
            while max_levels is None or d < max_levels:
                d += 1
                Nx, st = F.mxm(A, "min", "first", mask=P, complement=True)
                try:
                    info["frontier_nnz"].append(F.nnz)
                    info["products"].append(st["products"])
                    info["products_kept"].append(st["products_kept"])
                    info["nnz_new"].append(Nx.nnz)
                    info["ms_mxm"].append(st["ms_total"])
                    if Nx.nnz == 0:
                        break
                    info["levels"] = d
                    a = _result_as_input(Nx, device)
                    lin = a.rows.to(torch.int64)[:a.nnz] * n + a.cols.to(torch.int64)
                    parent.view(-1)[lin] = a.vals.to(torch.int64)
                    level.view(-1)[lin] = d
                    torch.cuda.synchronize(device)   # torch holds views of Nx's arrays: nothing of it is in flight when it is closed
                    del a
                    U, _ = P.ewise(Nx, "union", "first")
                    P.close()
                    P = U
                    Fn, _ = Nx.apply_vectors(col_op="second", cols=ids)
                    F.close()
                    F = Fn
                finally:
                    Nx.close()
        return parent.cpu().numpy(), level.cpu().numpy(), info
    finally:
        _close_all(device, (A, F, P))


# ---- a result assigned into a region of another (osp_csr_assign): block matrices, a subgraph put back -------------------------------
def bipartite_adjacency(rows, cols, shape, weights=None, *, dup="plus", dtype=np.float64, ctx=None):
    """The (m + n) x (m + n) adjacency matrix [[0, B], [B^T, 0]] of the bipartite graph with biadjacency edge list
    (rows[e], cols[e]) in ``shape`` = (m, n), as a CSR result (``networkx.bipartite.from_biadjacency_matrix``: row vertex i
    is vertex i, column vertex k is vertex m + k): B in one ``Context.build`` (repeated edges combined by ``dup``,
    ``weights=None`` means 1), its transpose, and ``spgemm.block_matrix`` of the two.  The caller closes the result."""
    ctx, device, dtype = _setup(dtype, ctx)
    m, n = (int(d) for d in shape)
    if m < 0 or n < 0:
        raise ValueError("shape must be (m, n) with m, n >= 0")
    _, _, r, c, w = _edges(rows, cols, None, device, weights, _torch_dtype(dtype))   # (no id below 0; the two sides have ranges of their own)
    if r.numel() and (int(r.max().item()) >= m or int(c.max().item()) >= n):
        raise ValueError(f"rows must lie in [0, {m}) and cols in [0, {n})")
    B = _build_device(ctx, device, m, n, r, c, w, dup, dtype)
    Bt = None
    try:
        Bt, _ = B.transpose()
        return _S.block_matrix([[None, B], [Bt, None]])[0]
    finally:
        _close_all(device, [B, Bt])


def disjoint_union(graphs, *, directed=False, dtype=np.float64, ctx=None):
    """The disjoint union of a short list of graphs (rows, cols, n) (``networkx.disjoint_union_all``): the block-diagonal
    adjacency matrix, graph g's vertex v renumbered ``offsets[g] + v``.  Every block is ``adjacency_matrix`` of its graph
    (unit weights; ``directed=False``: symmetric, self loops dropped; ``directed=True``: self loops kept), the union is
    ``spgemm.block_matrix`` of the diagonal grid: one pass over the growing result per graph.  Returns (result, offsets
    int64 of len(graphs) + 1); the caller closes the result."""
    ctx, device, dtype = _setup(dtype, ctx)
    graphs = [tuple(g) for g in graphs]
    blocks = []
    try:
        for r, c, n in graphs:
            blocks.append(adjacency_matrix(r, c, n, directed=directed, loops=directed, dtype=dtype, ctx=ctx))
        offsets = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int64)
        if not blocks:
            return ctx.build(0, 0, [], [], dtype=dtype, space="host")[0], offsets
        grid = [[b if i == k else None for k in range(len(blocks))] for i, b in enumerate(blocks)]
        return _S.block_matrix(grid)[0], offsets
    finally:
        _close_all(device, blocks)


def replace_subgraph(rows, cols, n, vertices, sub_rows, sub_cols, *, directed=False, dtype=np.float64, ctx=None):
    """The graph with edges (rows[e], cols[e]) on vertices [0, n) with the subgraph that ``vertices`` induce REPLACED by the
    graph with edges (sub_rows[e], sub_cols[e]), which is numbered by position in ``vertices`` (its vertex i is
    ``vertices[i]``): the inverse of ``induced_subgraph``.  Both patterns are built as ``adjacency_matrix`` builds them
    (``directed=False``: symmetric, self loops dropped; ``directed=True``: self loops kept) and the one is put into the
    other on the GPU by ``A.assign(S, vertices, vertices)``: the edges inside ``vertices`` are removed, the given ones
    added, every other edge stays.  ``vertices`` must be distinct and in [0, n) (else a ValueError) and may come in any
    order.

    Returns (u, v, info): the new graph's edges, int64, ascending by (u, v) -- once each with u < v for an undirected
    graph, every edge u -> v for a directed one; info = the assign's stats and n."""
    ctx, device, dtype = _setup(dtype, ctx)
    A = S = out = None
    try:
        A = adjacency_matrix(rows, cols, n, directed=directed, loops=directed, dtype=dtype, ctx=ctx)
        n = A.shape[0]
        vs = _check_vertices(vertices, n)
        S = adjacency_matrix(sub_rows, sub_cols, int(vs.size), directed=directed, loops=directed, dtype=dtype, ctx=ctx)
        out, st = A.assign(S, vs, vs, None, "host")
        info = dict(st, n=n)
        if not directed:
            u, v, _ = _upper_entries(out)
            return u, v, info
        rowptr, colidx, _ = out.to_host()
        return np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)), colidx.astype(np.int64), info
    finally:
        _close_all(device, [A, S, out])


# ---- the Kronecker product of two results (osp_csr_kron): product graphs, Kronecker powers ---------------------------------------------
# A graph argument is (rows, cols, n), as in disjoint_union; vertex (u, v) of a product of g (n1 vertices) and h (n2) is
# u * n2 + v.  The adjacency matrices are adjacency_matrix's (unit weights; directed=False: symmetric, self loops dropped;
# directed=True: self loops kept).
def _identity(ctx, device, n, dtype):
    """The n x n identity as a CSR result, in one ``Context.build``."""
    d = torch.arange(n, dtype=torch.int64, device=device)
    return _build_device(ctx, device, n, n, d, d, None, "error", dtype)


def _product_parts(g, h, directed, dtype, ctx):
    (r1, c1, n1), (r2, c2, n2) = tuple(g), tuple(h)
    A = adjacency_matrix(r1, c1, n1, directed=directed, loops=directed, dtype=dtype, ctx=ctx)
    try:
        return A, adjacency_matrix(r2, c2, n2, directed=directed, loops=directed, dtype=dtype, ctx=ctx)
    except BaseException:
        A.close()
        raise


def tensor_product(g, h, *, directed=False, dtype=np.float64, ctx=None):
    """The tensor (Kronecker, categorical) product of two graphs (``networkx.tensor_product``): (u, v) ~ (u', v') when
    u ~ u' in g AND v ~ v' in h -- ``A_g (x) A_h`` in one ``CsrResult.kron``.  Returns (result, info): the product's
    adjacency matrix, which the caller closes, and the kron's stats with n (its vertices)."""
    ctx, device, dtype = _setup(dtype, ctx)
    A = B = None
    try:
        A, B = _product_parts(g, h, directed, dtype, ctx)
        out, st = A.kron(B)
        return out, dict(st, n=out.shape[0])
    finally:
        _close_all(device, [A, B])


def cartesian_product(g, h, *, directed=False, dtype=np.float64, ctx=None):
    """The Cartesian product of two graphs (``networkx.cartesian_product``): (u, v) ~ (u', v') when u = u' and v ~ v' in h,
    or u ~ u' in g and v = v' -- ``A_g (x) I  union  I (x) A_h``, two ``CsrResult.kron`` with an identity from one
    ``Context.build`` each, joined by ``union("plus")``.  Returns (result, info): the adjacency matrix, which the caller
    closes; info = n, nnz, launches and ms_total of the three calls."""
    ctx, device, dtype = _setup(dtype, ctx)
    A = B = I1 = I2 = L = R = None
    try:
        A, B = _product_parts(g, h, directed, dtype, ctx)
        I1, I2 = _identity(ctx, device, A.shape[0], dtype), _identity(ctx, device, B.shape[0], dtype)
        L, s1 = A.kron(I2)
        R, s2 = I1.kron(B)
        out, s3 = L.union(R, "plus")
        steps = (s1, s2, s3)
        return out, {"n": out.shape[0], "nnz": out.nnz, "launches": sum(s["launches"] for s in steps),
                     "ms_total": sum(s["ms_total"] for s in steps)}
    finally:
        _close_all(device, [A, B, I1, I2, L, R])


def strong_product(g, h, *, directed=False, dtype=np.float64, ctx=None):
    """The strong product of two graphs (``networkx.strong_product``): the union of ``tensor_product`` and
    ``cartesian_product``, joined by ``union("plus")``.  Returns (result, info) as ``cartesian_product`` does."""
    ctx, device, dtype = _setup(dtype, ctx)
    T = Cp = None
    try:
        T, s1 = tensor_product(g, h, directed=directed, dtype=dtype, ctx=ctx)
        Cp, s2 = cartesian_product(g, h, directed=directed, dtype=dtype, ctx=ctx)
        out, s3 = T.union(Cp, "plus")
        steps = (s1, s2, s3)
        return out, {"n": out.shape[0], "nnz": out.nnz, "launches": sum(s["launches"] for s in steps),
                     "ms_total": sum(s["ms_total"] for s in steps)}
    finally:
        _close_all(device, [T, Cp])


def kronecker_power(rows, cols, n, k, *, directed=False, loops=True, dtype=np.float64, ctx=None):
    """The k-th Kronecker power ``A (x) A (x) ... (x) A`` (k factors, folded from the left) of the adjacency matrix of the
    graph with edges (rows[e], cols[e]) on vertices [0, n): the deterministic Kronecker graph of a seed, the model behind
    R-MAT, whose vertices (n^k), entries (nnz^k), degrees (outer products of the seed's) and -- for a loop-free symmetric
    seed -- triangles (6^(k-1) t^k) are known in closed form.  ``loops=True`` keeps the seed's self loops (a Kronecker
    graph's usual seed has them).  Returns (result, info): the matrix, which the caller closes; info = n (= n^k), nnz
    (= nnz^k), nnz_seed, ms_steps (the k - 1 products' times) and ms_total."""
    ctx, device, dtype = _setup(dtype, ctx)
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    A = out = None
    try:
        A = adjacency_matrix(rows, cols, n, directed=directed, loops=loops, dtype=dtype, ctx=ctx)
        out, ms, nnz_seed = A, [], A.nnz
        for _ in range(k - 1):
            nxt, st = out.kron(A)
            if out is not A:
                _close_all(device, [out])
            out = nxt
            ms.append(st["ms_total"])
        if out is A:
            A = None   # (k = 1: the seed itself is the result)
        return out, {"n": out.shape[0], "nnz": out.nnz, "nnz_seed": nnz_seed, "ms_steps": ms, "ms_total": sum(ms)}
    except BaseException:
        if out is not None and out is not A:
            out.close()
        raise
    finally:
        _close_all(device, [A])


# ---- the row-wise k-select (osp_csr_select_k): neighbour sampling, kNN graphs, random walks ----------------------------------------
def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    return int(seed)


def _vertex_list(vertices, n, what):
    """A list of vertex ids in [0, n), repeats allowed, as an int64 numpy array."""
    a = np.asarray(vertices.cpu() if torch.is_tensor(vertices) else vertices)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be integers")
    vs = np.atleast_1d(a).astype(np.int64).ravel()
    if vs.size and (vs.min() < 0 or vs.max() >= n):
        raise ValueError(f"{what} must lie in [0, {n})")
    return vs


def _rows_of(A, vertices, device):
    """``A.extract(rows=vertices)`` of an int64 tensor on the device: row i of the result is row ``vertices[i]`` of A."""
    v32 = vertices.to(torch.int32).contiguous()
    torch.cuda.synchronize(device)   # the library works on its own stream
    return A.extract(rows=v32)[0]


def sample_neighbors(rows, cols, n, seeds, fanouts, *, seed=0, directed=False, ctx=None):
    """GraphSAGE's neighbour sampling on the graph with edges (rows[e], cols[e]) on vertices [0, n) (``directed=False``: a
    simple graph, self loops dropped; ``directed=True``: the out-neighbours, self loops kept): ``len(fanouts)`` hops from
    ``seeds``.  Per hop h, with ``frontier`` the vertex list so far (hop 0: ``seeds``):

    1. ``F = A.extract(rows=frontier)`` -- one row per listed vertex, columns in the graph's numbering;
    2. ``B_h = F.select_k(fanouts[h], "random", seed=seed + h)`` -- at most ``fanouts[h]`` uniformly chosen neighbours of each;
    3. the next frontier is the current one followed by the columns of ``B_h`` it does not hold yet, ascending
       (``reduce("cols", "count")`` and torch on the device; only this list comes to the host).

    The random key hashes the FRONTIER-LOCAL row number, not the vertex: a vertex listed twice in ``seeds`` gets two
    independent samples, and the same vertex in another position or hop another one.  For fixed arguments the result is
    the same on every run.

    Returns (blocks, frontiers, info): ``blocks[h]`` is ``B_h``, a ``len(frontiers[h]) x n`` CsrResult with unit float32
    values, which the caller closes; ``frontiers`` has ``len(fanouts) + 1`` int64 arrays; info = nnz (per hop), launches
    (the k-selects' kernels), rows_capped (per hop) and ms_total (the k-selects')."""
    seed = _check_seed(seed)
    fanouts = [int(f) for f in fanouts]
    if any(f < 1 or f > 0xffffffff for f in fanouts):
        raise ValueError("every fanout must lie in [1, 2^32 - 1]")
    ctx, device, dtype = _setup(np.float32, ctx)
    A = adjacency_matrix(rows, cols, n, directed=directed, loops=directed, dtype=dtype, ctx=ctx)
    blocks = []
    try:
        n = A.shape[0]
        first = _vertex_list(seeds, n, "seeds")
        frontier = torch.as_tensor(first, device=device)
        frontiers = [first]
        seen = torch.zeros(n, dtype=torch.bool, device=device)
        seen[frontier] = True
        count = torch.empty(max(n, 1), dtype=_torch_dtype(dtype), device=device)
        info = {"nnz": [], "launches": 0, "rows_capped": [], "ms_total": 0.0}
        for h, fanout in enumerate(fanouts):
            F = _rows_of(A, frontier, device)
            try:
                B, st = F.select_k(fanout, "random", seed=(seed + h) % (1 << 64))
            finally:
                F.close()
            blocks.append(B)
            info["nnz"].append(B.nnz)
            info["rows_capped"].append(st["rows_capped"])
            info["launches"] += st["launches"]
            info["ms_total"] += st["ms_total"]
            B.reduce("cols", "count", out=count[:n])
            new = ((count[:n] > 0) & ~seen).nonzero().flatten()
            seen[new] = True
            frontier = torch.cat([frontier, new])
            frontiers.append(frontier.cpu().numpy())
        return blocks, frontiers, info
    except BaseException:
        _close_all(device, blocks)
        raise
    finally:
        _close_all(device, [A])


def knn_graph(rows, cols, n, weights, k, *, largest=True, symmetric="union", dtype=np.float64, ctx=None):
    """The k-nearest-neighbour sparsification of the weighted UNDIRECTED graph with edges (rows[e], cols[e]) on vertices
    [0, n) (self loops dropped; of parallel edges the strongest counts: the largest weight with ``largest``, else the
    smallest): ONE ``select_k(k, "largest" | "smallest")`` on the weighted adjacency S keeps every vertex's k strongest
    edges (ties to the lower neighbour id; a NaN weight ranks after every number), then

    * ``symmetric="union"``:  ``S.union(S^T, "max")`` (``"min"`` for smallest) -- an edge stays when EITHER end lists it;
    * ``symmetric="mutual"``: ``S.intersect(S^T, "first")`` -- when BOTH ends list it;
    * ``symmetric=None``:     S itself, the directed graph u -> (its k strongest neighbours).

    Returns (result, info): the n x n CsrResult, which the caller closes; info = the k-select's stats, n and nnz (of the
    result)."""
    if symmetric not in ("union", "mutual", None):
        raise ValueError('symmetric must be "union", "mutual" or None')
    k = int(k)
    if not 1 <= k <= 0xffffffff:
        raise ValueError("k must lie in [1, 2^32 - 1]")
    if weights is None:
        raise ValueError("knn_graph needs weights")
    ctx, device, dtype = _setup(dtype, ctx)
    W = S = T = None
    try:
        W = adjacency_matrix(rows, cols, n, weights, dup="max" if largest else "min", dtype=dtype, ctx=ctx)
        S, st = W.select_k(k, "largest" if largest else "smallest")
        if symmetric is None:
            out, S = S, None
        else:
            T, _ = S.transpose()
            out = S.union(T, "max" if largest else "min")[0] if symmetric == "union" else S.intersect(T, "first")[0]
        return out, dict(st, n=out.shape[0], nnz=out.nnz)
    finally:
        _close_all(device, [W, S, T])


def random_walks(rows, cols, n, starts, length, *, seed=0, directed=False, ctx=None):
    """Uniform random walks of ``length`` steps from every vertex of ``starts`` (repeats allowed) on the graph with edges
    (rows[e], cols[e]) on vertices [0, n) (``directed`` as in ``sample_neighbors``).  One step moves every walker at once:
    ``A.extract(rows=current).select_k(1, "random", seed=seed + step)`` -- row w of the extract is walker w's vertex, and
    the one entry the select keeps is a uniformly chosen neighbour.  The key hashes the walker's number, so two walkers on
    one vertex move independently.  A walker on a vertex without neighbours stays there, and from that step on its entries
    are -1.

    Returns an int64 array ``(len(starts), length + 1)``: column 0 is ``starts``, column t the walkers' vertices after t
    steps (or -1)."""
    seed = _check_seed(seed)
    length = int(length)
    if length < 0:
        raise ValueError("length must be at least 0")
    ctx, device, dtype = _setup(np.float32, ctx)
    A = adjacency_matrix(rows, cols, n, directed=directed, loops=directed, dtype=dtype, ctx=ctx)
    try:
        current = _vertex_list(starts, A.shape[0], "starts").copy()
        walks = np.full((current.size, length + 1), -1, np.int64)
        walks[:, 0] = current
        alive = np.ones(current.size, bool)
        for step in range(length):
            F = _rows_of(A, torch.as_tensor(current, device=device), device)
            try:
                B, _ = F.select_k(1, "random", seed=(seed + step) % (1 << 64))
            finally:
                F.close()
            try:
                rowptr, colidx, _ = B.to_host()
            finally:
                B.close()
            moved = np.diff(rowptr) == 1
            alive &= moved
            current[moved] = colidx.astype(np.int64)
            walks[alive, step + 1] = current[alive]
        return walks
    finally:
        _close_all(device, [A])


# ---- the row-wise scan and the weighted draws (osp_csr_scan, osp_csr_draw): weighted walks and weighted neighbour sampling ----------
def weighted_random_walks(rows, cols, n, weights, starts, length, *, seed=0, directed=False, dtype=np.float64, ctx=None):
    """Random walks of ``length`` steps from every vertex of ``starts`` (repeats allowed) on the WEIGHTED graph with edges
    (rows[e], cols[e], weights[e]) on vertices [0, n): a step goes to a neighbour with probability (the edge's weight) /
    (the sum of the vertex's weights).  ``directed`` as in ``sample_neighbors``; parallel edges ADD (the adjacency is built
    with ``dup="plus"``, in list order); an edge whose weight is not positive and finite is never taken.  One step moves
    every walker at once: ``A.extract(rows=current).draw(1, seed=seed + step)`` -- row w of the extract is walker w's
    vertex, and the draw hashes the walker's number, so two walkers on one vertex move independently.  Only the walkers'
    vector moves between steps; no CSR comes to the host.  A walker on a vertex it cannot leave (no neighbour, or no positive
    finite weight) stays there, and from that step on its entries are -1, as in ``random_walks``.

    Returns an int64 array ``(len(starts), length + 1)``: column 0 is ``starts``, column t the walkers' vertices after t
    steps (or -1)."""
    seed = _check_seed(seed)
    length = int(length)
    if length < 0:
        raise ValueError("length must be at least 0")
    if weights is None:
        raise ValueError("weighted_random_walks needs weights")
    ctx, device, dtype = _setup(dtype, ctx)
    A = adjacency_matrix(rows, cols, n, weights, directed=directed, loops=directed, dup="plus", dtype=dtype, ctx=ctx)
    try:
        current = torch.as_tensor(_vertex_list(starts, A.shape[0], "starts"), device=device)
        walks = torch.full((current.numel(), length + 1), -1, dtype=torch.int64, device=device)
        walks[:, 0] = current
        alive = torch.ones(current.numel(), dtype=torch.bool, device=device)
        for step in range(length):
            F = _rows_of(A, current, device)
            try:
                picked, _ = F.draw(1, seed=(seed + step) % (1 << 64))
            finally:
                F.close()
            picked = picked[:, 0]
            moved = picked >= 0
            alive &= moved
            current = torch.where(moved, picked, current)
            walks[:, step + 1] = torch.where(alive, current, torch.full_like(current, -1))
        return walks.cpu().numpy()
    finally:
        _close_all(device, [A])


def weighted_sample_neighbors(rows, cols, n, weights, seeds, fanouts, *, seed=0, directed=False, dtype=np.float64, ctx=None):
    """Neighbour sampling in proportion to edge weights, with replacement, on the graph of ``weighted_random_walks``
    (parallel edges add): ``len(fanouts)`` hops from ``seeds``.  Per hop h, with ``frontier`` the vertex list so far:

    1. ``F = A.extract(rows=frontier)``;
    2. ``F.draw(fanouts[h], seed=seed + h)`` -- ``fanouts[h]`` draws per frontier vertex;
    3. the (frontier-local row, column) pairs that are not -1 go through ONE ``Context.build(dup="count")``: ``B_h``'s
       values are the MULTIPLICITIES of the draws (the numerator of the importance-sampling estimator), and every row that
       can be drawn from sums to ``fanouts[h]``;
    4. the next frontier is formed as ``sample_neighbors`` forms it: the current one followed by the columns of ``B_h`` it
       does not hold yet, ascending.

    The draw hashes the FRONTIER-LOCAL row number, as ``sample_neighbors`` does.  Returns (blocks, frontiers, info):
    ``blocks[h]`` is a ``len(frontiers[h]) x n`` CsrResult, which the caller closes; ``frontiers`` has ``len(fanouts) + 1``
    int64 arrays; info = nnz (per hop), rows_without (per hop), launches (the draws' kernels) and ms_total (the draws')."""
    seed = _check_seed(seed)
    fanouts = [int(f) for f in fanouts]
    if any(f < 1 or f > 0xffffffff for f in fanouts):
        raise ValueError("every fanout must lie in [1, 2^32 - 1]")
    if weights is None:
        raise ValueError("weighted_sample_neighbors needs weights")
    ctx, device, dtype = _setup(dtype, ctx)
    A = adjacency_matrix(rows, cols, n, weights, directed=directed, loops=directed, dup="plus", dtype=dtype, ctx=ctx)
    blocks = []
    try:
        n = A.shape[0]
        first = _vertex_list(seeds, n, "seeds")
        frontier = torch.as_tensor(first, device=device)
        frontiers = [first]
        seen = torch.zeros(n, dtype=torch.bool, device=device)
        seen[frontier] = True
        count = torch.empty(max(n, 1), dtype=_torch_dtype(dtype), device=device)
        info = {"nnz": [], "rows_without": [], "launches": 0, "ms_total": 0.0}
        for h, fanout in enumerate(fanouts):
            F = _rows_of(A, frontier, device)
            try:
                picked, st = F.draw(fanout, seed=(seed + h) % (1 << 64))
            finally:
                F.close()
            local = torch.arange(frontier.numel(), device=device).repeat_interleave(fanout)
            picked = picked.flatten()
            keep = picked >= 0
            B = _build_device(ctx, device, frontier.numel(), n, local[keep], picked[keep], None, "count", dtype)
            blocks.append(B)
            info["nnz"].append(B.nnz)
            info["rows_without"].append(st["rows_without"])
            info["launches"] += st["launches"]
            info["ms_total"] += st["ms_total"]
            B.reduce("cols", "count", out=count[:n])
            new = ((count[:n] > 0) & ~seen).nonzero().flatten()
            seen[new] = True
            frontier = torch.cat([frontier, new])
            frontiers.append(frontier.cpu().numpy())
        return blocks, frontiers, info
    except BaseException:
        _close_all(device, blocks)
        raise
    finally:
        _close_all(device, [A])
