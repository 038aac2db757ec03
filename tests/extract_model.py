"""The numpy model that judges osp_csr_extract (include/outerspace_spgemm_extract.h), CsrResult.extract's composed path for
general column lists, and graph.induced_subgraph / ego_network / largest_component.  The extract is written the way the
header defines it -- the gathered rows in list order, a column kept when the list names it, renumbered by its rank --
and shares nothing with scipy's fancy indexing, which tests/test_extract_cpu.py holds it against."""
import numpy as np

from tests import mxv_model
from tests import transpose_model


def extract(rowptr, col, val, ncol, rows=None, cols=None):
    """``osp_csr_extract``: ((rowptr, col, val) of out, stats) with stats = nnz_in, nnz_gathered, nnz_out, readbacks.  A bad
    list is a ValueError, but -- as the header says -- not in an empty shape, where no list is read."""
    rowptr, col, val = np.asarray(rowptr, np.int64), np.asarray(col, np.uint32), np.asarray(val)
    M, nnz_in = len(rowptr) - 1, len(col)
    rows = None if rows is None else np.asarray(rows, np.int64).ravel()
    cols = None if cols is None else np.asarray(cols, np.int64).ravel()
    m = M if rows is None else len(rows)
    n = ncol if cols is None else len(cols)
    stats = {"nnz_in": nnz_in, "nnz_gathered": nnz_in if rows is None else 0, "nnz_out": 0, "readbacks": 0}
    if nnz_in == 0 or m == 0 or n == 0:
        return (np.zeros(m + 1, np.int64), col[:0].copy(), val[:0].copy()), stats
    if rows is None and cols is None:
        stats["nnz_out"] = nnz_in
        return (rowptr.copy(), col.copy(), val.copy()), stats
    if rows is not None and (rows.min() < 0 or rows.max() >= M):
        raise ValueError("a row index is not below M")
    if cols is not None and (cols.min() < 0 or cols.max() >= ncol or np.any(cols[1:] <= cols[:-1])):
        raise ValueError("the columns are not strictly ascending and below N")
    # the gathered matrix: g its row pointer, src the position in `in` of each of its entries
    if rows is None:
        g, src = rowptr, np.arange(nnz_in, dtype=np.int64)
    else:
        lens = rowptr[rows + 1] - rowptr[rows]
        g = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        src = np.repeat(rowptr[rows] - g[:-1], lens) + np.arange(g[-1], dtype=np.int64)
    stats["nnz_gathered"] = int(g[-1])
    stats["readbacks"] = 1 if rows is None or cols is None or g[-1] == 0 else 2
    if cols is None:
        keep, new = np.ones(len(src), bool), col[src]
    else:
        rank = np.full(ncol, -1, np.int64)
        rank[cols] = np.arange(len(cols))
        new = rank[col[src].astype(np.int64)]
        keep = new >= 0
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)    # kept entries before each gathered entry
    stats["nnz_out"] = int(before[-1])
    return (before[g], new[keep].astype(np.uint32), val[src[keep]]), stats


def is_ascending(cols):
    c = np.asarray(cols, np.int64)
    return bool(np.all(c[1:] > c[:-1]))


def extract_any(rowptr, col, val, ncol, rows=None, cols=None):
    """``CsrResult.extract``: the direct path for ascending (or no) columns, else the composition
    transpose -> row gather by cols -> transpose -> row gather by rows.  Returns (rowptr, col, val)."""
    if cols is None or is_ascending(cols):
        return extract(rowptr, col, val, ncol, rows, cols)[0]
    M = len(rowptr) - 1
    t = transpose_model.transpose(rowptr, col, val, ncol)              # ncol x M
    y = extract(*t, M, rows=cols)[0]                                   # len(cols) x M
    z = transpose_model.transpose(*y, M)                               # M x len(cols)
    return extract(*z, len(np.asarray(cols).ravel()), rows=rows)[0]


# ---- the graph functions ---------------------------------------------------------------------------------------------------------
def induced_subgraph(n, rows, cols, vertices, directed=False):
    """graph.induced_subgraph: (u, v) in the numbering of ``vertices``, ascending by (u, v); u < v for an undirected graph."""
    vs = np.asarray(vertices, np.int64).ravel()
    if len(np.unique(vs)) != len(vs):
        raise ValueError("vertices must be distinct")
    A = mxv_model.pattern(n, rows, cols, directed)
    rowptr, col, _ = extract_any(A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, n, vs, vs)
    u = np.repeat(np.arange(len(vs), dtype=np.int64), np.diff(rowptr))
    v = col.astype(np.int64)
    if not directed:
        up = u < v
        u, v = u[up], v[up]
    return u, v


def ego_network(n, rows, cols, center, radius):
    """graph.ego_network: (vertices within ``radius`` steps of ``center``, ascending; u; v)."""
    A = mxv_model.pattern(n, rows, cols, False)
    dist = np.full(n, -1, np.int64)
    dist[center] = 0
    frontier = np.array([center])
    for d in range(1, radius + 1):
        nb = np.unique(np.concatenate([A.indices[A.indptr[f]:A.indptr[f + 1]] for f in frontier] + [np.zeros(0, A.indices.dtype)]))
        frontier = nb[dist[nb] < 0]
        if len(frontier) == 0:
            break
        dist[frontier] = d
    vertices = np.flatnonzero(dist >= 0).astype(np.int64)
    return (vertices,) + induced_subgraph(n, rows, cols, vertices)


def largest_component(n, rows, cols):
    """graph.largest_component: (vertices of the most frequent label -- the smallest on a tie --, ascending; u; v)."""
    if n == 0:
        none = np.zeros(0, np.int64)
        return none, none, none
    labels, _ = mxv_model.connected_components(n, rows, cols)
    best = int(np.argmax(np.bincount(labels, minlength=n)))           # (argmax: the first of the largest)
    vertices = np.flatnonzero(labels == best).astype(np.int64)
    return (vertices,) + induced_subgraph(n, rows, cols, vertices)
