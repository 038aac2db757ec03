"""Numpy models that judge osp_csr_mxv_arg (tests/test_gpu_mxv_arg.py) and the graph functions built on it
(tests/test_gpu_forest_matching.py): checkers only; nothing here runs on the GPU.

``mxv_arg`` takes y from tests/mxv_model.py's ``mxv`` (imported, not copied) and arg from a literal loop over every row's
products, which are tests/vector_model.py's ``apply_vectors`` on the column side.  ``kruskal`` and ``greedy_matching`` are the
sequential algorithms on the edges sorted by the strict total orders graph.py names; tests/test_mxv_arg_cpu.py checks them
against scipy and networkx, which share nothing with them."""
import numpy as np

from tests import mxv_model, vector_model

ADD_OPS = ["min", "max"]
MUL_OPS = mxv_model.MUL_OPS
GROUPS = mxv_model.GROUPS


def products(rowptr, col, val, x, mul):
    """mul(in[i, j], x[j]) of every entry, in val's dtype: osp_csr_mxv's products."""
    if mul == "first":
        return val
    return vector_model.apply_vectors(np.asarray(rowptr, np.int64), col, val, cols=np.asarray(x, val.dtype), col_op=mul)[0]


def arg_rows(rowptr, col, prod, add):
    """The definition, entry by entry: a NaN is passed over; a product takes the lead only when it is strictly better under
    the IEEE comparison (so -0.0 and +0.0 tie), and columns ascend, so the first of equals -- the smallest column -- stays.
    A row that never finds a leader gives -1."""
    ptr, cl, pl = np.asarray(rowptr).tolist(), np.asarray(col).tolist(), np.asarray(prod).tolist()
    is_min = add == "min"
    arg = np.full(len(ptr) - 1, -1, np.int64)
    for i in range(len(ptr) - 1):
        best, bc = 0.0, -1
        for t in range(ptr[i], ptr[i + 1]):
            p = pl[t]
            if p != p:
                continue
            if bc < 0 or (p < best if is_min else p > best):
                best, bc = p, cl[t]
        arg[i] = bc
    return arg


def mxv_arg(rowptr, col, val, x, add, mul):
    """osp_csr_mxv_arg.  Returns (y of val's dtype, arg int64, rows of more than 2048 entries, rows whose arg is -1)."""
    if add not in ADD_OPS or mul not in MUL_OPS:
        raise ValueError((add, mul))
    y, nlong = mxv_model.mxv(rowptr, col, val, x, add, mul)
    arg = arg_rows(rowptr, col, products(rowptr, col, val, x, mul), add)
    return y, arg, nlong, int((arg < 0).sum())


# ---- the graph functions ------------------------------------------------------------------------------------------------------------
def simple_edges(n, rows, cols, weights, keep, dtype):
    """graph.weighted_adjacency's undirected edge set, once each: self loops dropped, u < v, duplicates keep their smallest
    (``keep="min"``) or largest (``"max"``) weight; the weights rounded to ``dtype``.  Returns (u, v, w), ascending by (u, v)."""
    r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    w = np.ones(len(r)) if weights is None else np.asarray(weights, np.float64)
    ok = r != c
    u, v, w = np.minimum(r, c)[ok], np.maximum(r, c)[ok], w[ok]
    key, inv = np.unique(u * n + v, return_inverse=True)
    out = np.full(len(key), np.inf if keep == "min" else -np.inf)
    (np.minimum if keep == "min" else np.maximum).at(out, inv, w)
    return key // n, key % n, out.astype(dtype)


def kruskal(n, u, v, w):
    """The minimum spanning forest of the simple graph (u[e], v[e]) with weights w under the strict total order
    (w, min, max): a union-find over the edges sorted by that key.  Returns (u, v, w) of the forest, u < v, ascending by
    (u, v)."""
    u, v, w = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(w)
    a, b = np.minimum(u, v), np.maximum(u, v)
    order = np.lexsort((b, a, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    took = []
    for e in order.tolist():
        ra, rb = find(int(a[e])), find(int(b[e]))
        if ra != rb:
            parent[ra] = rb
            took.append(e)
    took = np.array(took, np.int64)
    took = took[np.lexsort((b[took], a[took]))] if len(took) else took
    return a[took], b[took], w[took]


def greedy_matching(n, u, v, w):
    """The sequential greedy matching over the edges sorted by (-w, min, max): an edge is taken when both its ends are free.
    Returns mate int64[n], -1 for a free vertex."""
    u, v, w = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(w)
    a, b = np.minimum(u, v), np.maximum(u, v)
    mate = np.full(n, -1, np.int64)
    for e in np.lexsort((b, a, -w)).tolist():
        if a[e] != b[e] and mate[a[e]] < 0 and mate[b[e]] < 0:
            mate[a[e]], mate[b[e]] = b[e], a[e]
    return mate


# ---- the graphs the forest and matching tests share -----------------------------------------------------------------------------------
def graphs():
    """name -> (n, rows, cols, weights or None)."""
    rng = np.random.default_rng(23)
    n8, r8, c8 = mxv_model._rmat(8, 11)
    n10, r10, c10 = mxv_model._rmat(10, 12)
    n7, r7, c7 = mxv_model._rmat(7, 14)
    path = np.arange(38)
    leaves = np.arange(1, 2201)
    extra_r, extra_c = rng.integers(0, 2201, 3000), rng.integers(0, 2201, 3000)
    a, b = np.triu_indices(6, 1)
    return {
        "rmat8 weights 1..4": (n8, r8, c8, rng.integers(1, 5, len(r8)).astype(np.float64)),
        "rmat10 random weights": (n10, r10, c10, rng.random(len(r10))),
        "path of 39": (39, path, path + 1, rng.integers(1, 4, 38).astype(np.float64)),
        "star": (12, np.zeros(11, np.int64), np.arange(1, 12), rng.integers(1, 3, 11).astype(np.float64)),
        "two components and isolated vertices": (16, np.concatenate([a, a + 8]), np.concatenate([b, b + 8]),
                                                 rng.integers(1, 4, 2 * len(a)).astype(np.float64)),   # (6, 7, 14, 15 are alone)
        "all-equal weights": (n7, r7, c7, None),
        "star of 2200 leaves plus random edges": (2201, np.concatenate([np.zeros(2200, np.int64), extra_r]),
                                                  np.concatenate([leaves, extra_c]), rng.integers(1, 6, 5200).astype(np.float64)),
    }
