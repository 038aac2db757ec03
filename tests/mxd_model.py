"""Numpy models that judge osp_csr_mxd (tests/test_gpu_mxd.py) and the graph functions built on it
(tests/test_gpu_propagate.py): checkers only; nothing here runs on the GPU.

``mxd`` IS the contract include/outerspace_spgemm_mxd.h states: tests/mxv_model.py's ``mxv`` column by column (imported, not
copied).  ``serial_R`` is the order in which ONE lane of outerspace_amd/csrc/osp_mxd.h evaluates R's tree -- the leaves in
bit-reversed order, finished subtrees kept like the digits of a binary counter -- written as a literal loop;
tests/test_mxd_cpu.py checks that it gives ``vector_model.reduce_segments``'s bits.  ``label_spreading`` and
``propagate_features`` follow graph.py step for step; the CPU test checks them against networkx and scipy, which share nothing
with them."""
import numpy as np
import scipy.sparse as sp

from tests import mxv_model
from tests import vector_model

ADD_OPS = mxv_model.ADD_OPS
MUL_OPS = mxv_model.MUL_OPS
MAX_COLS = 65536
KS = [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 130]   # every packing, a partial tile and three tiles


def lanes_per_row(k):
    """The power of two >= min(k, 64)."""
    lanes = 1
    while lanes < min(k, 64):
        lanes *= 2
    return lanes


def mxd(rowptr, col, val, X, add, mul, k=None):
    """osp_csr_mxd.  Returns (Y of val's dtype, shape (M, k); rows of more than 2048 entries)."""
    rowptr = np.asarray(rowptr, np.int64)
    M = len(rowptr) - 1
    k = np.shape(X)[1] if k is None else k
    Y = np.empty((M, k), val.dtype)
    nlong = int((np.diff(rowptr) > vector_model.BLOCK).sum())
    for c in range(k):
        x = None if X is None else np.ascontiguousarray(np.asarray(X, val.dtype)[:, c])
        Y[:, c], nlong = mxv_model.mxv(rowptr, col, val, x, add, mul)
    return Y, nlong


def expected_launches(rowptr, scan_launches=None):
    """stats.launches of osp_csr_mxd by the header's formula; with a long row the scan's own count is needed."""
    lens = np.diff(np.asarray(rowptr, np.int64))
    nnz = int(lens.sum())
    if len(lens) == 0 or nnz == 0:
        return 0
    if nnz <= vector_model.BLOCK:
        return 1
    if not (lens > vector_model.BLOCK).any():
        return 3
    return 3 + 1 + scan_launches + 2


def _comb(op, a, b):
    """a (+) b on two scalars of one dtype: vector_model.combine's expressions."""
    with np.errstate(all="ignore"):
        if op == "plus":
            return a + b
        if op == "min":
            return b if b < a else a
        if op == "max":
            return b if b > a else a
    raise ValueError(op)


def _serial_short(e, op):
    """R of the at most 2048 values e by one lane: leaf i of the walk is lane bitreverse(i); after it, one merge per
    trailing 1-bit of i with the EARLIER subtree on the left."""
    m = len(e)
    assert m <= vector_model.BLOCK
    idv = vector_model.identity(op, e.dtype)
    lgw = 6 if m > 32 else 0 if m <= 1 else (m - 1).bit_length()
    stack = [None] * 6
    v = idv
    for i in range(1 << lgw):
        lane = int(format(i, "b").zfill(lgw)[::-1], 2) if lgw else 0
        v = idv
        for t in range(lane, m, vector_model.WAVE):
            v = _comb(op, v, e[t])
        for j in range(6):
            if not (i >> j) & 1:
                stack[j] = v
                break
            v = _comb(op, stack[j], v)
            stack[j] = None   # (every entry is read once)
    return v


def serial_R(e, op):
    """R of the values e in the one-lane order: blocks of 2048 first when there are more, then R of their results."""
    e = np.ascontiguousarray(e)
    while len(e) > vector_model.BLOCK:
        e = np.array([_serial_short(e[b:b + vector_model.BLOCK], op) for b in range(0, len(e), vector_model.BLOCK)], e.dtype)
    return e.dtype.type(_serial_short(e, op))


# ---- the graph functions ----------------------------------------------------------------------------------------------------------
def _csr(A, dtype):
    return A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(dtype)


def normalised(A, dtype):
    """graph.py's _normalised: (rowptr, col, values of D^-1/2 A D^-1/2 in ``dtype``, the largest row count)."""
    rp, c, v = _csr(A, dtype)
    deg = vector_model.reduce(rp, c, v, A.shape[1], "rows", "count")[0]
    d = (dtype(1.0) / np.sqrt(np.maximum(deg, dtype(1.0)))).astype(dtype)
    s = vector_model.apply_vectors(rp, c, v, rows=d, row_op="times", cols=d, col_op="times")[0]
    return rp, c, s, int(deg.max()) if len(deg) else 0


def check_labels(labels, n):
    """graph.py's _check_labels for a dict: (vertices, columns, classes ascending)."""
    verts = np.fromiter(labels.keys(), np.int64, len(labels))
    classes = sorted(set(labels.values()))
    column = {c: i for i, c in enumerate(classes)}
    return verts, np.array([column[v] for v in labels.values()], np.int64), classes


def label_spreading(n, rows, cols, labels, alpha=0.99, max_iter=30, dtype=np.float64):
    """graph.label_spreading step for step.  Returns (F, predicted, info): iterations, classes, nnz, max_degree."""
    dtype = np.dtype(dtype).type
    A = mxv_model.pattern(n, rows, cols, False)
    verts, column, classes = check_labels(labels, n)
    info = {"iterations": 0, "classes": classes, "nnz": int(A.nnz), "max_degree": 0}
    base = np.zeros((n, len(classes)), dtype)
    base[verts, column] = dtype(1.0 - alpha)
    F = np.zeros_like(base)
    if A.nnz == 0:
        info["iterations"] = max_iter
        F = base if max_iter > 0 else F
        return F, [classes[i] for i in F.argmax(axis=1)], info
    rp, c, s, info["max_degree"] = normalised(A, dtype)
    for _ in range(max_iter):
        Z = mxd(rp, c, s, F, "plus", "times")[0]
        F = (dtype(alpha) * Z + base).astype(dtype)
        info["iterations"] += 1
    return F, [classes[i] for i in F.argmax(axis=1)], info


def propagate_features(n, rows, cols, X, hops=2, self_loops=True, dtype=np.float64):
    """graph.propagate_features step for step.  Returns (A^^hops X, info): hops, nnz, max_degree."""
    dtype = np.dtype(dtype).type
    H = np.array(X, dtype, ndmin=2)
    info = {"hops": hops, "nnz": 0, "max_degree": 0}
    if n == 0 or H.shape[1] == 0 or hops == 0:
        return H, info
    A = mxv_model.pattern(n, rows, cols, False)
    if self_loops:
        A = (A + sp.identity(n, format="csr")).tocsr()
        A.data[:] = 1.0
        A.sort_indices()
    if A.nnz == 0:
        return np.zeros_like(H), info
    info["nnz"] = int(A.nnz)
    rp, c, s, info["max_degree"] = normalised(A, dtype)
    for _ in range(hops):
        H = mxd(rp, c, s, H, "plus", "times")[0]
    return H, info


# ---- float64 references that share nothing with the models (scipy products) ----------------------------------------------------------
def reference_S(n, rows, cols, self_loops=False):
    """D^-1/2 (A [+ I]) D^-1/2 as a float64 scipy CSR, a count of 0 counting as 1."""
    A = mxv_model.pattern(n, rows, cols, False).astype(np.float64)
    if self_loops:
        A = (A + sp.identity(n, format="csr")).tocsr()
    deg = np.asarray(A.sum(axis=1)).ravel()
    deg[deg == 0] = 1.0
    d = sp.diags(1.0 / np.sqrt(deg))
    return (d @ A @ d).tocsr(), int(deg.max()) if n else 0


def reference_label_spreading(n, rows, cols, labels, alpha=0.99, max_iter=30):
    """(F float64, max degree) of the iteration evaluated with scipy in float64."""
    S, maxdeg = reference_S(n, rows, cols)
    verts, column, classes = check_labels(labels, n)
    base = np.zeros((n, len(classes)))
    base[verts, column] = 1.0 - alpha
    F = np.zeros_like(base)
    for _ in range(max_iter):
        F = alpha * (S @ F) + base
    return F, maxdeg


def reference_propagate(n, rows, cols, X, hops=2, self_loops=True):
    """(A^^hops X, |A^|^hops |X|, max row count) in float64 with scipy."""
    S, maxdeg = reference_S(n, rows, cols, self_loops)
    H, Habs = np.asarray(X, np.float64), np.abs(np.asarray(X, np.float64))
    for _ in range(hops):
        H, Habs = S @ H, abs(S) @ Habs
    return H, Habs, maxdeg


def label_bound(max_iter, maxdeg, dtype):
    """The relative entry-wise distance label_spreading may have from the float64 evaluation: every term is non-negative, so
    a step loses at most (row length + a few) roundings, and the steps add."""
    return 2.0 * max_iter * (maxdeg + 8) * float(np.finfo(dtype).eps)


def propagate_bound(hops, maxdeg, dtype):
    """The factor of |A^|^hops |X| propagate_features may be away from the float64 evaluation, entry-wise."""
    return 2.0 * hops * (maxdeg + 8) * float(np.finfo(dtype).eps)


def margins(F):
    """The relative gap between each row's two largest entries: (top - second) / top, 0 where top is 0 or F has one column."""
    if F.shape[1] < 2:
        return np.zeros(F.shape[0])
    top2 = np.sort(F, axis=1)[:, -2:]
    with np.errstate(all="ignore"):
        return np.where(top2[:, 1] > 0, (top2[:, 1] - top2[:, 0]) / top2[:, 1], 0.0)


# ---- the graphs both test files share ----------------------------------------------------------------------------------------------------
def _karate():
    import networkx as nx
    G = nx.karate_club_graph()
    e = np.array(G.edges(), np.int64)
    return G.number_of_nodes(), e[:, 0], e[:, 1]


def propagate_graphs():
    """name -> (n, rows, cols): the karate club, R-MAT 8, and the karate club with an isolated vertex and a separate
    component (a triangle) that holds no labelled vertex."""
    nk, rk, ck = _karate()
    n8, r8, c8 = mxv_model._rmat(8, 11)
    return {
        "karate": (nk, rk, ck),
        "rmat8": (n8, r8, c8),
        "karate + isolated + unlabelled triangle": (nk + 4, np.concatenate([rk, [nk + 1, nk + 2, nk + 3]]),
                                                    np.concatenate([ck, [nk + 2, nk + 3, nk + 1]])),
    }


def labellings(name, n, nclasses):
    """A dict vertex -> class with ``nclasses`` classes: the labelled vertices are spread over the graph's first vertices (the
    ones of the karate club, or R-MAT's low ids, which have edges), deterministic per (graph, nclasses)."""
    rng = np.random.default_rng(1000 + nclasses + len(name))
    limit = 34 if name.startswith("karate") else n
    verts = rng.choice(limit, size=max(2 * nclasses, limit // 8), replace=False)
    return {int(v): int(i % nclasses) for i, v in enumerate(verts)}
