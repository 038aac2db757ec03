"""The numpy model that judges osp_csr_assign (include/outerspace_spgemm_assign.h), CsrResult.assign's composed path for
general column lists, spgemm.block_matrix and graph.bipartite_adjacency / disjoint_union / replace_subgraph.  The assign is
written the way the header defines it -- a's entry (i, k) gets the coordinate (rows[i], cols[k]), the entries of c inside
rows x cols are dropped (no accum) or met (accum), the two sorted lists are merged -- and shares nothing with scipy's
``lil`` assignment, which tests/test_assign_cpu.py holds it against."""
import numpy as np

from tests import ewise_model
from tests import extract_model

ACCUM_OPS = ewise_model.UNION_OPS      # plus times min max first second
COPY_OPS = ewise_model.COPY_OPS


def _keys(rowptr, col, ncol):
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    return row, row * np.int64(ncol) + col.astype(np.int64)


def assign(c, ncol, a, a_ncol, rows=None, cols=None, accum=None):
    """``osp_csr_assign``: c, a = (rowptr, col, val).  Returns ((rowptr, col, val), computed, stats): ``computed`` marks the
    entries whose value is op(c, a) and not a copy; stats = nnz_c, nnz_a, nnz_region, nnz_both, nnz_out, readbacks and
    no_work (the shapes that launch nothing).  A wrong shape of a and a bad list are ValueErrors, but -- as the header says
    -- a list is not read in a no-work shape."""
    c_ptr, c_col, c_val = np.asarray(c[0], np.int64), np.asarray(c[1], np.uint32), np.asarray(c[2])
    a_ptr, a_col, a_val = np.asarray(a[0], np.int64), np.asarray(a[1], np.uint32), np.asarray(a[2])
    if accum is not None and accum not in ACCUM_OPS:
        raise ValueError(accum)
    assert c_val.dtype == a_val.dtype
    M, nnz_c, nnz_a = len(c_ptr) - 1, len(c_col), len(a_col)
    rows = None if rows is None else np.asarray(rows, np.int64).ravel()
    cols = None if cols is None else np.asarray(cols, np.int64).ravel()
    m = M if rows is None else len(rows)
    n = ncol if cols is None else len(cols)
    if (len(a_ptr) - 1, a_ncol) != (m, n):
        raise ValueError(f"a is {len(a_ptr) - 1} x {a_ncol}, the region {m} x {n}")
    stats = {"nnz_c": nnz_c, "nnz_a": nnz_a, "nnz_region": 0, "nnz_both": 0, "nnz_out": 0, "readbacks": 0, "no_work": True}
    none = np.zeros(0, bool)

    def copy_of(x_ptr, x_col, x_val):
        stats["nnz_out"] = len(x_col)
        return (x_ptr.copy(), x_col.copy(), x_val.copy()), np.zeros(len(x_col), bool), stats

    if M == 0 or nnz_c + nnz_a == 0:
        return (np.zeros(M + 1, np.int64), c_col[:0].copy(), c_val[:0].copy()), none, stats
    if m == 0 or n == 0 or (accum is not None and nnz_a == 0):
        return copy_of(c_ptr, c_col, c_val)
    if rows is None and cols is None and accum is None:
        return copy_of(a_ptr, a_col, a_val)
    stats["no_work"], stats["readbacks"] = False, 1
    if rows is not None:
        if rows.min() < 0 or rows.max() >= M:
            raise ValueError("a row index is not below M")
        if len(np.unique(rows)) != len(rows):
            raise ValueError("a row index is repeated")
    if cols is not None and (cols.min() < 0 or cols.max() >= ncol or np.any(cols[1:] <= cols[:-1])):
        raise ValueError("the columns are not strictly ascending and below N")
    # a in c's coordinates, sorted by them (the rows may come in any order, the columns ascend)
    a_row, _ = _keys(a_ptr, a_col, a_ncol)
    big_row = a_row if rows is None else rows[a_row]
    big_col = a_col.astype(np.int64) if cols is None else cols[a_col.astype(np.int64)]
    ka = big_row * np.int64(ncol) + big_col
    order = np.argsort(ka, kind="stable")
    ka, va = ka[order], a_val[order]
    assert np.all(np.diff(ka) > 0)
    # c's entries inside the region
    c_row, kc = _keys(c_ptr, c_col, ncol)
    # (nothing here is as long as ncol: the model runs at 2^32 - 1 columns too)
    region = np.ones(nnz_c, bool) if rows is None else np.isin(c_row, rows)
    if cols is not None:
        region &= np.isin(c_col.astype(np.int64), cols)
    q = np.searchsorted(ka, kc)
    c_hit = np.zeros(nnz_c, bool)
    inside = q < nnz_a
    c_hit[inside] = ka[q[inside]] == kc[inside]
    assert not np.any(c_hit & ~region)
    stats["nnz_region"], stats["nnz_both"] = int(region.sum()), int(c_hit.sum())
    va = va.copy()
    a_computed = np.zeros(nnz_a, bool)
    if accum is not None:
        va[q[c_hit]] = ewise_model.apply_op(accum, c_val[c_hit], va[q[c_hit]])
        a_computed[q[c_hit]] = True
    kept = ~(region if accum is None else c_hit)       # what c's side writes
    own, own_val = kc[kept], c_val[kept]
    pos_a = np.arange(nnz_a) + np.searchsorted(own, ka)
    pos_c = np.arange(len(own)) + np.searchsorted(ka, own)
    keys = np.empty(nnz_a + len(own), np.int64)
    val = np.empty(len(keys), c_val.dtype)
    computed = np.zeros(len(keys), bool)
    keys[pos_a], keys[pos_c] = ka, own
    val[pos_a], val[pos_c] = va, own_val
    computed[pos_a] = a_computed
    assert np.all(np.diff(keys) > 0)
    rowptr = np.zeros(M + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(keys // ncol, minlength=M))
    stats["nnz_out"] = len(keys)
    return (rowptr, (keys % ncol).astype(np.uint32), val), computed, stats


def assign_any(c, ncol, a, a_ncol, rows=None, cols=None, accum=None):
    """``CsrResult.assign``: the direct path for ascending (or no) columns, else a's columns reordered by
    ``extract(cols=argsort(cols))`` and assigned with the sorted list.  Returns ((rowptr, col, val), computed)."""
    if cols is None or extract_model.is_ascending(cols):
        return assign(c, ncol, a, a_ncol, rows, cols, accum)[:2]
    cols = np.asarray(cols, np.int64).ravel()
    if a_ncol != len(cols):
        raise ValueError("a's columns are not the list's")
    order = np.argsort(cols, kind="stable")
    sorted_a = extract_model.extract_any(*a, a_ncol, None, order)
    return assign(c, ncol, sorted_a, a_ncol, rows, cols[order], accum)[:2]


def embed(a, a_ncol, shape, rows=None, cols=None):
    """``CsrResult.embed``: a assigned into an empty result of ``shape``."""
    M, N = shape
    empty = (np.zeros(M + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.asarray(a[2]).dtype))
    return assign_any(empty, N, a, a_ncol, rows, cols)[0]


# ---- block matrices ------------------------------------------------------------------------------------------------------------------
def block_matrix(blocks, dtype=np.float64):
    """``spgemm.block_matrix`` on a grid of ((rowptr, col, val), ncol) or None: one assign per block into a growing result.
    Returns ((rowptr, col, val), (M, N))."""
    grid = [list(row) for row in blocks]
    if not grid or not grid[0] or any(len(row) != len(grid[0]) for row in grid):
        raise ValueError("blocks must be a non-empty rectangular grid")
    heights, widths = [None] * len(grid), [None] * len(grid[0])
    for i, row in enumerate(grid):
        for k, b in enumerate(row):
            if b is None:
                continue
            for sizes, at, got in ((heights, i, len(b[0][0]) - 1), (widths, k, b[1])):
                if sizes[at] is not None and sizes[at] != got:
                    raise ValueError("inconsistent block sizes")
                sizes[at] = got
    if None in heights or None in widths:
        raise ValueError("a block row or column is all None")
    r0, c0 = np.concatenate([[0], np.cumsum(heights)]).astype(np.int64), np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    M, N = int(r0[-1]), int(c0[-1])
    out = (np.zeros(M + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dtype))
    for i, row in enumerate(grid):
        for k, b in enumerate(row):
            if b is None:
                continue
            out = assign(out, N, b[0], b[1], np.arange(r0[i], r0[i + 1]), np.arange(c0[k], c0[k + 1]))[0]
    return out, (M, N)


# ---- the graph functions ---------------------------------------------------------------------------------------------------------------
def _pattern(n, rows, cols, directed):
    """The 0/1 adjacency of an edge list as (rowptr, col, val): undirected = symmetric without self loops, directed = as
    given with self loops; parallel edges once."""
    r, c = np.asarray(rows, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    if not directed:
        keep = r != c
        r, c = np.concatenate([r[keep], c[keep]]), np.concatenate([c[keep], r[keep]])
    keys = np.unique(r * np.int64(max(n, 1)) + c)
    rowptr = np.zeros(n + 1, np.int64)
    if n:
        rowptr[1:] = np.cumsum(np.bincount(keys // n, minlength=n))
    return rowptr, (keys % max(n, 1)).astype(np.uint32), np.ones(len(keys))


def _edges_of(csr, directed):
    u = np.repeat(np.arange(len(csr[0]) - 1, dtype=np.int64), np.diff(csr[0]))
    v = csr[1].astype(np.int64)
    if not directed:
        up = u < v
        u, v = u[up], v[up]
    return u, v


def bipartite_adjacency(rows, cols, shape, weights=None):
    """graph.bipartite_adjacency: (rowptr, col, val) of [[0, B], [B^T, 0]], repeated edges summed."""
    m, n = shape
    r, c = np.asarray(rows, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    w = np.ones(len(r)) if weights is None else np.asarray(weights, np.float64).ravel()

    def build(nrow, ncol, rr, cc):
        keys, inv = np.unique(rr * np.int64(max(ncol, 1)) + cc, return_inverse=True)
        val = np.zeros(len(keys))
        np.add.at(val, inv, w)      # (list order)
        rowptr = np.zeros(nrow + 1, np.int64)
        if nrow and len(keys):
            rowptr[1:] = np.cumsum(np.bincount(keys // max(ncol, 1), minlength=nrow))
        return (rowptr, (keys % max(ncol, 1)).astype(np.uint32), val), ncol

    return block_matrix([[None, build(m, n, r, c)], [build(n, m, c, r), None]])[0]


def disjoint_union(graphs, directed=False):
    """graph.disjoint_union: ((rowptr, col, val), offsets)."""
    blocks = [(_pattern(n, r, c, directed), n) for r, c, n in graphs]
    offsets = np.concatenate([[0], np.cumsum([n for _, n in blocks])]).astype(np.int64)
    if not blocks:
        return (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0)), offsets
    grid = [[b if i == k else None for k in range(len(blocks))] for i, b in enumerate(blocks)]
    return block_matrix(grid)[0], offsets


def replace_subgraph(n, rows, cols, vertices, sub_rows, sub_cols, directed=False):
    """graph.replace_subgraph: (u, v), ascending by (u, v); u < v for an undirected graph."""
    vs = np.asarray(vertices, np.int64).ravel()
    if vs.size and (vs.min() < 0 or vs.max() >= n):
        raise ValueError("vertices must lie in [0, n)")
    if len(np.unique(vs)) != len(vs):
        raise ValueError("vertices must be distinct")
    A, Sub = _pattern(n, rows, cols, directed), _pattern(len(vs), sub_rows, sub_cols, directed)
    out = assign_any(A, n, Sub, len(vs), vs, vs)[0]
    return _edges_of(out, directed)
