"""Graph analytics on the masked product (``osp_spgemm_masked``).

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
