"""Numpy models that judge osp_csr_reduce, osp_csr_apply_vectors and osp_csr_select_vertices (tests/test_gpu_vector.py) and the
graph functions built on them (tests/test_gpu_kcore.py): checkers only; nothing here runs on the GPU.

``reduce`` follows include/outerspace_spgemm_vector.h's definition of R operation by operation -- the 64 lane values, the
butterfly, the blocks of 2048 of a longer segment and the recursion over their results -- vectorised over the segments that
take the same number of steps.  Lanes and steps that hold no element are filled with the identity: combining with it changes no
bit (x + +0.0 is x for every x a lane can hold, since a lane starts from +0.0 and a sum that begins there is never -0.0; a
comparison with an infinity of the identity's sign never takes it).  tests/test_vector_cpu.py checks that against a literal
loop.  The graph models follow graph.py's rounds so that their ``info`` lists can be compared round for round;
tests/test_vector_cpu.py checks them against networkx, which shares nothing with them."""
import numpy as np
import scipy.sparse as sp

from tests import ewise_model
from tests import truss_model

AXES = ["rows", "cols"]                        # in the enum's order
REDUCE_OPS = ["plus", "min", "max", "count"]   # in the enum's order
APPLY_OPS = ["plus", "times", "min", "max", "second", "minus", "div"]   # osp_ewise_op_t without "first"
WAVE = 64
BLOCK = 2048


def identity(op, dtype):
    return np.dtype(dtype).type({"plus": 0.0, "min": np.inf, "max": -np.inf}[op])


def combine(op, a, b):
    """a (+) b on arrays of one dtype: one addition, or a copy of one operand (a comparison with a NaN is false: a stays)."""
    with np.errstate(all="ignore"):
        if op == "plus":
            return a + b
        if op == "min":
            return np.where(b < a, b, a)
        if op == "max":
            return np.where(b > a, b, a)
    raise ValueError(op)


def _short(starts, lens, vals, op):
    """R of every segment vals[starts[s] : starts[s] + lens[s]], all of at most BLOCK entries."""
    out = np.empty(len(starts), vals.dtype)
    if not len(starts):
        return out
    idv = identity(op, vals.dtype)
    steps = -(-lens // WAVE)                                     # elements per lane, at most
    # lanes that matter: all 64 once a lane holds two elements, else the next power of two (the others hold the identity)
    width = np.minimum(WAVE, 1 << np.searchsorted(1 << np.arange(7), lens))
    for key in np.unique(steps * 128 + width):
        t, w = int(key) // 128, int(key) % 128
        sel = np.flatnonzero((steps == t) & (width == w))
        cols = max(t, 1) * w
        off = np.arange(cols, dtype=np.int64)
        inside = off[None, :] < lens[sel][:, None]
        idx = np.where(inside, starts[sel][:, None] + off[None, :], 0)
        arr = np.where(inside, vals[idx] if len(vals) else idv, idv).reshape(len(sel), max(t, 1), w)
        p = np.full((len(sel), w), idv, vals.dtype)
        for step in range(t):                                    # p_l = p_l (+) e_{l + 64 t}
            p = combine(op, p, arr[:, step, :])
        d = w // 2
        while d:                                                 # p_l = p_l (+) p_{l + d} for l < d
            p = combine(op, p[:, :d], p[:, d:2 * d])
            d //= 2
        out[sel] = p[:, 0]
    return out


def reduce_segments(ptr, vals, op):
    """R of every segment of (ptr, vals).  Returns (values, number of segments longer than BLOCK)."""
    ptr = np.asarray(ptr, np.int64)
    lens = np.diff(ptr)
    out = np.full(len(lens), identity(op, vals.dtype), vals.dtype)
    short = lens <= BLOCK
    out[short] = _short(ptr[:-1][short], lens[short], vals, op)
    long_ = np.flatnonzero(~short)
    if len(long_):
        nblk = -(-lens[long_] // BLOCK)
        blkptr = np.concatenate([[0], np.cumsum(nblk)]).astype(np.int64)
        which = np.repeat(np.arange(len(long_)), nblk)
        b = np.arange(blkptr[-1], dtype=np.int64) - blkptr[which]
        partial = _short(ptr[long_][which] + b * BLOCK, np.minimum(BLOCK, lens[long_][which] - b * BLOCK), vals, op)
        out[long_] = reduce_segments(blkptr, partial, op)[0]
    return out, len(long_)


def column_view(rowptr, col, val, ncol):
    """(colptr, rows, vals) of the CSR: one stable sort by column, so a column's entries keep ascending row order."""
    order = np.argsort(col, kind="stable")
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    colptr = np.zeros(ncol + 1, np.int64)
    colptr[1:] = np.cumsum(np.bincount(col.astype(np.int64), minlength=ncol))
    return colptr, row[order], val[order]


def reduce(rowptr, col, val, ncol, axis, op):
    """osp_csr_reduce.  Returns (vector of val's dtype, long_segments)."""
    if axis not in AXES or op not in REDUCE_OPS:
        raise ValueError((axis, op))
    rowptr = np.asarray(rowptr, np.int64)
    ptr, v = (rowptr, val) if axis == "rows" else column_view(rowptr, col, val, ncol)[::2]
    if op == "count":
        return np.diff(ptr).astype(val.dtype), int((np.diff(ptr) > BLOCK).sum())
    return reduce_segments(ptr, v, op)


def apply_vectors(rowptr, col, val, rows=None, row_op=None, cols=None, col_op=None):
    """osp_csr_apply_vectors: col_op(row_op(c, rows[i]), cols[j]); an op of None skips its side.  Returns (values of val's
    dtype, computed): ``computed`` marks the values that came out of an arithmetic operation (their NaNs' payloads are the
    hardware's)."""
    if row_op is None and col_op is None:
        raise ValueError("both sides are None")
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    out, computed = val, False
    for op, vec, index in ((row_op, rows, row), (col_op, cols, col.astype(np.int64))):
        if op is None:
            continue
        if op not in APPLY_OPS:
            raise ValueError(op)
        out = ewise_model.apply_op(op, out, np.asarray(vec, val.dtype)[index])
        computed = op not in ewise_model.COPY_OPS or (computed and op != "second")
    return out, computed


def select_vertices(rowptr, col, val, keep_rows=None, keep_cols=None):
    """osp_csr_select_vertices.  Returns (rowptr, col, val)."""
    if keep_rows is None and keep_cols is None:
        raise ValueError("both keep vectors are None")
    nrow = len(rowptr) - 1
    row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(rowptr))
    keep = np.ones(len(col), bool)
    if keep_rows is not None:
        keep &= np.asarray(keep_rows)[row] != 0
    if keep_cols is not None:
        keep &= np.asarray(keep_cols)[col.astype(np.int64)] != 0
    out_ptr = np.zeros(nrow + 1, np.int64)
    out_ptr[1:] = np.cumsum(np.bincount(row[keep], minlength=nrow))
    return out_ptr, col[keep], val[keep]


# ---- k-core, Jaccard similarity, clustering coefficient ---------------------------------------------------------------------------
def _core_info():
    return {"rounds": 0, "nnz_graph": []}


def _peel_level(A, k, info):
    """Rounds of level k (graph.py's _peel_level): the degrees, then -- unless every vertex that still has an edge has at
    least k -- the subgraph induced by the vertices of degree >= k.  Returns (A', deg)."""
    while True:
        deg = np.diff(A.indptr)
        info["rounds"] += 1
        info["nnz_graph"].append(int(A.nnz))
        keep = deg >= k
        if not np.any((deg > 0) & ~keep):
            return A, deg
        rp, c, v = select_vertices(A.indptr.astype(np.int64), A.indices, A.data, keep, keep)
        A = sp.csr_matrix((v, c, rp), shape=A.shape)


def core_numbers(adj):
    """(core int64[n], info) of the symmetric 0/1 scipy CSR ``adj``: info = rounds, nnz_graph per round, k_max."""
    A = adj.tocsr()
    A.sort_indices()
    core = np.zeros(A.shape[0], np.int64)
    info = dict(_core_info(), k_max=0)
    k = 1
    while A.nnz:
        A, deg = _peel_level(A, k, info)
        if A.nnz == 0:
            break
        core[deg > 0] = k
        info["k_max"] = k
        k += 1
    return core, info


def k_core(adj, k):
    """(u, v, info) of the k-core of ``adj``: its edges once each, u < v, ascending."""
    if k < 0:
        raise ValueError("k must be at least 0")
    A = adj.tocsr()
    A.sort_indices()
    info = _core_info()
    if A.nnz:
        A, _ = _peel_level(A, k, info)
    u, v, _ = truss_model._upper(A)
    return u, v, info


def jaccard_similarity(adj, dtype=np.float64):
    """(u, v, jaccard float64) of every edge of ``adj``, u < v, ascending: S / ((deg u + deg v) - S) on the supports'
    pattern, one operation of ``dtype`` each, 0 where the edge has no common neighbour."""
    n = adj.shape[0]
    u, v, _ = truss_model._upper(adj)
    S = truss_model._supports(adj)
    rp, c, s = S.indptr.astype(np.int64), S.indices.astype(np.uint32), S.data.astype(dtype)
    deg = np.diff(adj.indptr).astype(dtype)
    d, _ = apply_vectors(rp, c, s, deg, "second", deg, "plus")
    j = ewise_model.apply_op("div", s, ewise_model.apply_op("minus", d, s))
    ju, jv, jval = truss_model._upper(sp.csr_matrix((j, c.astype(np.int64), rp), shape=adj.shape))
    out = np.zeros(len(u), np.float64)
    out[np.searchsorted(u * n + v, ju * n + jv)] = jval.astype(np.float64)
    return u, v, out


def local_clustering(adj, dtype=np.float64):
    """float64[n]: t / (deg (deg - 1)) with t = the row sums of the supports (R's order; the sums are exact integers), 0
    where deg < 2."""
    S = truss_model._supports(adj)
    t, _ = reduce(S.indptr.astype(np.int64), S.indices.astype(np.uint32), S.data.astype(dtype), adj.shape[1], "rows", "plus")
    deg = np.diff(adj.indptr).astype(np.float64)
    out = np.zeros(adj.shape[0], np.float64)
    some = deg >= 2
    out[some] = t.astype(np.float64)[some] / (deg[some] * (deg[some] - 1.0))
    return out


def clique_with_pendant(q=6):
    """Edge list of K_q with one pendant vertex attached to vertex 0: (n, rows, cols)."""
    r, c = np.triu_indices(q, 1)
    return q + 1, np.concatenate([r, [0]]), np.concatenate([c, [q]])
