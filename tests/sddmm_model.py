"""Numpy models that judge osp_csr_sddmm (tests/test_gpu_sddmm.py) and the graph functions built on it
(tests/test_gpu_edge_models.py): checkers only; nothing here runs on the GPU.

``sddmm`` IS the contract include/outerspace_spgemm_sddmm.h states: the k products of every entry are a segment of
tests/vector_model.py's ``reduce_segments`` (imported, not copied), and ``sddmm_by_mxv`` is the header's equivalence --
tests/mxv_model.py's ``mxv`` of the one-row CSR of X[i, :] with Y[j, :] -- entry by entry.  ``edge_scores``,
``landmark_bounds`` and ``factorize`` follow graph.py step for step; the ``reference_*`` functions are float64 evaluations
with scipy, networkx and plain numpy that share nothing with them (tests/test_sddmm_cpu.py compares the two)."""
import numpy as np
import scipy.sparse as sp

from tests import build_model
from tests import ewise_model
from tests import mxd_model
from tests import mxv_model
from tests import semiring_model
from tests import transpose_model
from tests import vector_model

ADD_OPS = mxv_model.ADD_OPS
MUL_OPS = mxv_model.MUL_OPS
ACCUM_OPS = ["plus", "times", "minus", "div", "min", "max", "second"]   # osp_csr_apply_vectors' table
ARITHMETIC = ("plus", "times", "minus", "div")                          # a NaN that comes out of these has the hardware's payload
MAX_COLS = mxd_model.MAX_COLS
KS = [0, 1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 130]

lanes_per_entry = mxd_model.lanes_per_row   # the power of two >= min(k, 64)


def expected_launches(nnz):
    """stats.launches of osp_csr_sddmm: ONE kernel when `in` has entries, whatever k is."""
    return 1 if nnz else 0


def _rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def products(rowptr, col, X, Y, mul, k, dtype):
    """The (nnz, k) array of mul(X[i, c], Y[j, c]), X's element in a's place; "first" reads no Y, "second" no X."""
    rowptr = np.asarray(rowptr, np.int64)
    nnz = len(col)
    a = np.asarray(X, dtype)[_rows_of(rowptr)] if mul != "second" else np.zeros((nnz, k), dtype)
    b = np.asarray(Y, dtype)[col.astype(np.int64)] if mul != "first" else np.zeros((nnz, k), dtype)
    assert a.shape == b.shape == (nnz, k)
    return ewise_model.apply_op(mul, a, b)


def sddmm(rowptr, col, val, X, Y, add="plus", mul="times", accum="second", k=None):
    """osp_csr_sddmm: the values of the result (its pattern is the input's), and whether a NaN among them may carry the
    hardware's payload."""
    if add not in ADD_OPS or mul not in MUL_OPS or (accum is not None and accum not in ACCUM_OPS):
        raise ValueError((add, mul, accum))
    k = np.shape(X if X is not None else Y)[1] if k is None else k
    prod = products(rowptr, col, X, Y, mul, k, val.dtype)
    d = vector_model.reduce_segments(np.arange(len(col) + 1, dtype=np.int64) * k, np.ascontiguousarray(prod).ravel(), add)[0]
    computed = add == "plus" or accum in ARITHMETIC
    if accum in (None, "second"):
        return d, computed
    return ewise_model.apply_op(accum, val, d), computed


def sddmm_by_mxv(rowptr, col, X, Y, add, mul, entries):
    """d of the listed entries by the header's equivalence: mxv of the one-row CSR that holds X[i, :] at the columns 0..k-1
    with the vector Y[j, :]."""
    rows = _rows_of(np.asarray(rowptr, np.int64))
    k = X.shape[1]
    one = (np.array([0, k], np.int64), np.arange(k, dtype=np.uint32))
    return np.array([mxv_model.mxv(*one, np.ascontiguousarray(X[rows[p]]), Y[int(col[p])], add, mul)[0][0] for p in entries], X.dtype)


def main_pattern(dtype, seed=91):
    """The 70 x 4200 pattern of the packing tests: rows of 0, 1, 2, 3, 63, 64, 65 and 4097 entries, 50 empty rows, a last row
    of 2.  Returns (ncol, (rowptr, col, val))."""
    lengths = [0, 1, 2, 3, 63, 64, 65, 4097] + [0] * 61 + [2]
    assert len(lengths) == 70
    ncol = 4200
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=m, replace=False)) for m in lengths]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dtype)
    return ncol, (rowptr, col, val)


def fma_telling_dense():
    """(X, Y) in float32, 8 x 200 each, from tests/mxv_model.py's input that tells a fused multiply-add from two roundings:
    row i of X holds mxv's row i (130 to 200 entries, so every lane folds a second product into a partial that is not zero),
    row i of Y the vector's elements at that row's columns.  What is past a row's length is 0 on both sides: the products
    there are +0.0 and a partial that is not -0.0 does not change when +0.0 is added, fused or not."""
    ncol, (rowptr, col, val), x = mxv_model.fma_telling_input()
    M, k = len(rowptr) - 1, int(np.diff(rowptr).max())
    X, Y = np.zeros((M, k), np.float32), np.zeros((M, k), np.float32)
    for i in range(M):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        X[i, :e - b], Y[i, :e - b] = val[b:e], x[col[b:e].astype(np.int64)]
    return X, Y


def fma_diagonal(X, Y):
    """What a CONTRACTED fold would give at the entries (i, i) under (plus, times): mxv_model.fma_mxv_plus_times on the rows."""
    k = X.shape[1]
    one = (np.array([0, k], np.int64), np.arange(k, dtype=np.uint32))
    return np.array([mxv_model.fma_mxv_plus_times(*one, np.ascontiguousarray(X[i]), Y[i])[0] for i in range(len(X))], np.float32)


# ---- the graph functions ----------------------------------------------------------------------------------------------------------
def score_pattern(n, rows, cols, directed):
    """graph.edge_scores' pattern as (rowptr, col): the deduplicated edges, for an undirected graph once each with u < v."""
    A = mxv_model.pattern(n, rows, cols, directed)
    if not directed:
        A = sp.triu(A, 1).tocsr()
        A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.uint32)


def inverse_norms(X, dtype):
    nrm = np.sqrt((np.asarray(X, np.float64) ** 2).sum(axis=1))
    return (1.0 / np.where(nrm == 0, 1.0, nrm)).astype(dtype)


def edge_scores(n, rows, cols, X, Y=None, kind="dot", directed=False, dtype=np.float64):
    """graph.edge_scores step for step.  Returns (u, v, score of ``dtype``)."""
    dtype = np.dtype(dtype).type
    X = np.asarray(X, dtype)
    Y = X if Y is None else np.asarray(Y, dtype)
    rowptr, col = score_pattern(n, rows, cols, directed)
    u, v = _rows_of(rowptr), col.astype(np.int64)
    if len(col) == 0:
        return u, v, np.zeros(0, dtype)
    score = sddmm(rowptr, col, np.ones(len(col), dtype), X, Y)[0]
    if kind == "cosine":
        score = vector_model.apply_vectors(rowptr, col, score, inverse_norms(X, dtype), "times", inverse_norms(Y, dtype), "times")[0]
    return u, v, score


def reference_edge_scores(n, rows, cols, X, Y=None, kind="dot", directed=False):
    """(u, v, score float64, ||x_u|| ||y_v||) by one Python loop over the distinct edges: shares nothing with the model."""
    X = np.asarray(X, np.float64)
    Y = X if Y is None else np.asarray(Y, np.float64)
    edges = set()
    for a, b in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist()):
        if directed:
            edges.add((a, b))
        elif a != b:
            edges.add((min(a, b), max(a, b)))
    edges = sorted(edges)
    u, v = np.array([e[0] for e in edges], np.int64), np.array([e[1] for e in edges], np.int64)
    score, scale = np.zeros(len(edges)), np.zeros(len(edges))
    for t, (a, b) in enumerate(edges):
        dot = float(np.dot(X[a], Y[b]))
        na, nb = float(np.linalg.norm(X[a])), float(np.linalg.norm(Y[b]))
        scale[t] = na * nb
        score[t] = dot if kind == "dot" else (dot / (na * nb) if na and nb else 0.0)
    return u, v, score, scale


def landmark_bounds(n, rows, cols, landmarks, pairs, weights=None, dtype=np.float64):
    """graph.landmark_bounds step for step: the model of shortest_paths, its transpose, the distinct pairs as a pattern
    (build with dup="first"), sddmm under (min, plus), the callers' order."""
    dtype = np.dtype(dtype).type
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    W = semiring_model.weighted_adjacency(rows, cols, n, weights, dtype=dtype)
    d = semiring_model.shortest_paths(W, n, landmarks)[0]
    if len(pr) == 0:
        return np.zeros(0, dtype)
    D = np.ascontiguousarray(d.T)
    (rowptr, col, val), _, _ = build_model.build(n, n, pr[:, 0], pr[:, 1], None, dup="first", dtype=dtype)
    bound = sddmm(rowptr, col, val, D, D, "min", "plus")[0]
    keys = _rows_of(rowptr) * n + col.astype(np.int64)
    return bound[np.searchsorted(keys, pr[:, 0] * n + pr[:, 1])]


def factorize_step(S, shape, U, V):
    """One step's library outputs on (U, V): (e on S's pattern, gU, gV), as graph.factorize forms them."""
    rowptr, col, val = S
    e = sddmm(rowptr, col, val, U, V, "plus", "times", "minus")[0]
    gU = mxd_model.mxd(rowptr, col, e, V, "plus", "times", k=U.shape[1])[0]
    t = transpose_model.transpose(rowptr, col, e, shape[1])
    gV = mxd_model.mxd(*t, U, "plus", "times", k=U.shape[1])[0]
    return e, gU, gV


def factorize(rows, cols, vals, shape, rank, steps, lr, reg=0.0, U0=None, V0=None, seed=0, dup="error", dtype=np.float64):
    """graph.factorize step for step.  Returns (U, V, info): nnz, steps, loss."""
    dtype = np.dtype(dtype).type
    M, N = shape
    rng = np.random.default_rng(seed)
    U = np.asarray(U0, dtype) if U0 is not None else (rng.standard_normal((M, rank)) / np.sqrt(max(rank, 1))).astype(dtype)
    V = np.asarray(V0, dtype) if V0 is not None else (rng.standard_normal((N, rank)) / np.sqrt(max(rank, 1))).astype(dtype)
    S = build_model.build(M, N, rows, cols, vals, dup=dup, dtype=dtype)[0]
    info = {"nnz": len(S[1]), "steps": 0, "loss": []}
    lr, reg = dtype(lr), dtype(reg)
    for _ in range(steps):
        e, gU, gV = factorize_step(S, shape, U, V)
        info["loss"].append(float((e.astype(np.float64) ** 2).sum()))
        U, V = (U + lr * (gU - reg * U)).astype(dtype), (V + lr * (gV - reg * V)).astype(dtype)
        info["steps"] += 1
    return U, V, info


def planted_case():
    """The planted rank-3 20 x 15 matrix with a seeded 60 % of its entries observed, fixed starting points, and the step size
    and count chosen so that the float64 model's loss never increases and its final / initial ratio lies in [1e-4, 1e-1]
    (tests/test_sddmm_cpu.py asserts both).  Returns a dict: rows, cols, vals, shape, rank, steps, lr, U0, V0."""
    rng = np.random.default_rng(2024)
    M, N, rank = 20, 15, 3
    A = rng.standard_normal((M, rank)) @ rng.standard_normal((rank, N))
    seen = np.flatnonzero(rng.random(M * N) < 0.6)
    rows, cols = seen // N, seen % N
    return {"rows": rows, "cols": cols, "vals": A[rows, cols], "shape": (M, N), "rank": rank, "steps": 60, "lr": 0.02,
            "U0": 0.5 * rng.standard_normal((M, rank)), "V0": 0.5 * rng.standard_normal((N, rank))}


def karate():
    return mxd_model._karate()
