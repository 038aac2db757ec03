"""Numpy models that judge osp_csr_mxv (tests/test_gpu_mxv.py) and the graph functions built on it
(tests/test_gpu_rank_components.py): checkers only; nothing here runs on the GPU.

``mxv`` IS the composition include/outerspace_spgemm_mxv.h names: tests/vector_model.py's ``apply_vectors`` on the column
side, then its ``reduce_segments`` over the rows (imported, not copied).  ``pagerank`` and ``connected_components`` follow
graph.py's rounds step for step; tests/test_mxv_cpu.py checks them against networkx and scipy, which share nothing with
them."""
import numpy as np
import scipy.sparse as sp

from tests import vector_model

ADD_OPS = ["plus", "min", "max"]
MUL_OPS = ["times", "plus", "min", "max", "first", "second"]
GROUPS = [4, 8, 16, 32, 64]


def mxv(rowptr, col, val, x, add, mul):
    """osp_csr_mxv.  Returns (y of val's dtype, rows of more than 2048 entries)."""
    if add not in ADD_OPS or mul not in MUL_OPS:
        raise ValueError((add, mul))
    rowptr = np.asarray(rowptr, np.int64)
    prod = val if mul == "first" else vector_model.apply_vectors(rowptr, col, val, cols=np.asarray(x, val.dtype), col_op=mul)[0]
    return vector_model.reduce_segments(rowptr, np.ascontiguousarray(prod), add)


def fma_mxv_plus_times(rowptr, col, val, x):
    """What a CONTRACTED fold would give under (plus, times) on float32 rows of at most 2048 entries: every step of a lane's
    fold as one fused multiply-add, p = float32(float64(a) * float64(x) + float64(p)) -- the product (exact in float64) is
    never rounded to float32 on its own -- then the butterfly as it is.  A lane's first step gives the rounded product
    either way (p is +0.0), so only rows of more than 64 entries can tell.  Used only to show that an input does."""
    assert val.dtype == np.float32
    xs = np.asarray(x, np.float32)
    out = np.zeros(len(rowptr) - 1, np.float32)
    for i in range(len(rowptr) - 1):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        assert e - b <= vector_model.BLOCK
        p = np.zeros(vector_model.WAVE, np.float32)
        for t in range(b, e, vector_model.WAVE):
            k = min(vector_model.WAVE, e - t)
            exact = val[t:t + k].astype(np.float64) * xs[col[t:t + k].astype(np.int64)].astype(np.float64)
            p[:k] = (exact + p[:k].astype(np.float64)).astype(np.float32)
        d = vector_model.WAVE // 2
        while d:
            p = p[:d] + p[d:2 * d]
            d //= 2
        out[i] = p[0]
    return out


def fma_telling_input():
    """(ncol, (rowptr, col, val), x) in float32: 8 rows of 130 to 200 random entries, so that every lane folds a second
    product into a partial that is not zero."""
    rng = np.random.default_rng(5)
    ncol = 512
    lengths = rng.integers(130, 201, 8)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=int(k), replace=False)) for k in lengths]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(np.float32)
    x = rng.standard_normal(ncol).astype(np.float32)
    return ncol, (rowptr, col, val), x


# ---- the graphs the rank and component tests share --------------------------------------------------------------------------------
def _rmat(scale, seed):
    from outerspace_amd import generators as gen
    n, r, c, _ = gen.rmat_coo(scale, 4, "g500", seed=seed)
    return n, r.astype(np.int64), c.astype(np.int64)


def rank_graphs():
    """name -> (n, rows, cols, directed)."""
    n8, r8, c8 = _rmat(8, 11)
    n10, r10, c10 = _rmat(10, 12)
    path = np.arange(39)
    return {
        "rmat8 undirected": (n8, r8, c8, False),
        "rmat8 directed": (n8, r8, c8, True),
        "rmat10 directed": (n10, r10, c10, True),
        "dangling": (7, np.array([0, 0, 1, 2, 3, 3]), np.array([1, 2, 2, 0, 4, 5]), True),   # 4, 5 and 6 have no out-edge
        "path": (40, path, path + 1, False),
        "edgeless": (5, np.zeros(0, np.int64), np.zeros(0, np.int64), False),
    }


def component_graphs():
    """name -> (n, rows, cols)."""
    out = {}
    for scale, seed in ((8, 11), (10, 12), (12, 13)):
        out[f"rmat{scale}"] = _rmat(scale, seed)
    path = np.arange(999)
    out["path"] = (1000, path, path + 1)
    a, b = np.triu_indices(6, 1)
    out["two cliques"] = (13, np.concatenate([a, a + 7]), np.concatenate([b, b + 7]))   # (vertex 6 is alone)
    out["isolated vertices"] = (9, np.array([1, 5, 5]), np.array([3, 7, 5]))
    return out


def pattern(n, rows, cols, directed):
    """graph.py's pattern as scipy CSR of 0/1: deduplicated; directed keeps self loops, undirected is symmetric without."""
    r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if not directed:
        keep = r != c
        r, c = np.concatenate([r[keep], c[keep]]), np.concatenate([c[keep], r[keep]])
    A = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    A.data[:] = 1.0
    A.sort_indices()
    return A


def _csr(A, dtype):
    return A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(dtype)


def pagerank(n, rows, cols, directed=False, alpha=0.85, tol=1e-6, max_iter=100, dtype=np.float64):
    """graph.pagerank step for step.  Returns (rank, info): iterations, converged, err, nnz."""
    dtype = np.dtype(dtype).type
    A = pattern(n, rows, cols, directed)
    info = {"iterations": 0, "converged": False, "err": 0.0, "nnz": 0}
    if A.nnz == 0:
        info["converged"] = True
        return np.full(n, 1.0 / n if n else 0.0, dtype), info
    info["nnz"] = int(A.nnz)
    deg = vector_model.reduce(*_csr(A, dtype), n, "rows", "count")[0]
    At = _csr(A.T.tocsr(), dtype) if directed else _csr(A, dtype)
    has = deg > 0
    r = np.full(n, 1.0 / n, dtype)
    for _ in range(max_iter):
        with np.errstate(all="ignore"):
            s = np.where(has, r / deg, dtype(0))
        y = mxv(*At, s, "plus", "times")[0]
        dangling = r[~has].sum(dtype=dtype)
        new = (dtype(alpha) * (y + dangling / dtype(n)) + dtype((1.0 - alpha) / n)).astype(dtype)
        err = float(np.abs(new - r).sum(dtype=dtype))
        r = new
        info["iterations"] += 1
        info["err"] = err
        if err < n * tol:
            info["converged"] = True
            break
    return r, info


def connected_components(n, rows, cols, dtype=np.float64):
    """graph.connected_components round for round.  Returns (labels int64, info): rounds, components."""
    dtype = np.dtype(dtype).type
    if dtype == np.float32 and n > 1 << 24:
        raise ValueError("float32 holds vertex ids exactly only up to n = 2^24")
    A = pattern(n, rows, cols, False)
    info = {"rounds": 0, "components": n}
    if A.nnz == 0:
        return np.arange(n, dtype=np.int64), info
    csr = _csr(A, dtype)
    lab = np.arange(n).astype(dtype)
    while True:
        y = mxv(*csr, lab, "min", "second")[0]
        new = np.minimum(lab, y)
        new = new[new.astype(np.int64)]
        info["rounds"] += 1
        same = np.array_equal(new, lab)
        lab = new
        if same:
            break
    labels = lab.astype(np.int64)
    info["components"] = int((labels == np.arange(n)).sum())
    return labels, info
