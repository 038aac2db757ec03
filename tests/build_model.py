"""A literal numpy model of ``osp_csr_build`` (include/outerspace_spgemm_build.h) and of the graph functions built on it
(``graph.adjacency_matrix``, ``laplacian``, ``incidence_matrix``, ``line_graph``): a stable lexicographic sort, then a
Python-level left fold of every run in list order, in the dtype, giving bits.  It also models the call's stats.  Nothing
here is fast or clever; tests/test_build_cpu.py checks it against scipy, numpy's ``ufunc.at``, a dict and networkx."""
import os
import re

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "outerspace_amd", "csrc")
# a run of more entries than this is folded by a wave (and counted in long_runs)
LONG_RUN = int(re.search(r"kBuildLongRun\s*=\s*(\d+)", open(os.path.join(_CSRC, "osp_build.h")).read()).group(1))
_COMPACT = open(os.path.join(_CSRC, "osp_compact.h")).read()
CHUNK = int(re.search(r"kCompactThreads\s*=\s*(\d+)", _COMPACT).group(1)) * int(re.search(r"kCompactRounds\s*=\s*(\d+)", _COMPACT).group(1))
_SORT = open(os.path.join(_CSRC, "osp_sort.h")).read()
SORT_TILE = int(re.search(r"kRsThreads\s*=\s*(\d+)", _SORT).group(1)) * int(re.search(r"kRsItems\s*=\s*(\d+)", _SORT).group(1))
_PRIMS = open(os.path.join(_CSRC, "osp_prims.h")).read()
SCAN_TILE = int(re.search(r"kScanThreads\s*=\s*(\d+)", _PRIMS).group(1)) * int(re.search(r"kScanItems\s*=\s*(\d+)", _PRIMS).group(1))
SCAN_SMALL_TILES = int(re.search(r"kScanSmallTiles\s*=\s*(\d+)", _PRIMS).group(1))
RADIX = int(re.search(r"kRadix\s*=\s*(\d+)", _PRIMS).group(1))

DUP_OPS = ("error", "plus", "min", "max", "first", "last", "count")
ERR_ARG, ERR_RANGE, ERR_DUPLICATE = 2, 6, 233


class BuildError(ValueError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _scan_launches(n):
    return 1 if n == 0 or -(-n // SCAN_TILE) <= SCAN_SMALL_TILES else 3


def _bits_for(n):
    b = 0
    while n > (1 << b):
        b += 1
    return b


def launches(M, N, nnz):
    """Kernels of a call on a non-empty shape: the zeroing of two words, the two sorts (a histogram, a scan and a scatter
    per pass), two gathers and the sorted row pointer, the heads and their scan, the row pointer and the write."""
    passes = (max(1, _bits_for(N)) + 7) // 8 + (max(1, _bits_for(M)) + 7) // 8
    per_pass = 2 + _scan_launches(-(-nnz // SORT_TILE) * RADIX)
    return 1 + passes * per_pass + 3 + 1 + _scan_launches(-(-nnz // 64)) + 2


def build(M, N, rows, cols, vals=None, dup="plus", dtype=np.float64):
    """``osp_csr_build``: returns ((rowptr int64, col uint32, val dtype), stats, layout).  stats: nnz_in, nnz_out, long_runs,
    launches, readbacks.  layout: ``order`` (the list positions in sorted order), ``head`` (the sorted position of every run's
    first entry) and ``length`` (the runs' lengths) -- where the runs lie in the sorted order, for tests that place them.
    Raises BuildError with the status the library returns."""
    if dup not in DUP_OPS:
        raise BuildError(ERR_ARG, "dup")
    dtype = np.dtype(dtype).type
    r, c = np.asarray(rows, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    nnz = len(r)
    if len(c) != nnz or M >= 0xffffffff or N > 0xffffffff or nnz >= 0xffffffff:
        raise BuildError(ERR_ARG, "shape")
    stats = {"nnz_in": nnz, "nnz_out": 0, "long_runs": 0, "launches": 0, "readbacks": 0}
    none = np.zeros(0, np.int64)
    if nnz == 0 or M == 0 or N == 0:   # nothing is launched, no list is read
        return (np.zeros(M + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dtype)), stats, {"order": none, "head": none, "length": none}
    stats["launches"], stats["readbacks"] = launches(M, N, nnz), 1
    if (r >= M).any() or (c >= N).any() or (r < 0).any() or (c < 0).any():
        raise BuildError(ERR_RANGE, "an index of the list is outside its dimension")
    order = np.lexsort((c, r))   # stable: equal coordinates stay in list order
    rs, cs = r[order], c[order]
    first = np.ones(nnz, bool)
    first[1:] = (rs[1:] != rs[:-1]) | (cs[1:] != cs[:-1])
    head = np.flatnonzero(first)
    length = np.diff(np.append(head, nnz))
    if dup == "error" and len(head) < nnz:
        raise BuildError(ERR_DUPLICATE, "duplicate coordinate")
    v = None if vals is None or dup == "count" else np.ascontiguousarray(vals, dtype).ravel()
    out = np.empty(len(head), dtype)
    if dup == "count":
        out[:] = length.astype(dtype)
    elif v is None:
        if dup == "plus":   # the chain 1 + 1 + ... stays at 2^24 in float32
            out[:] = (np.minimum(length, 1 << 24) if dtype == np.float32 else length).astype(dtype)
        else:
            out[:] = 1
    else:
        ob, vb = bits(out), bits(v)
        ob[:] = vb[order[head]]                      # a run of one entry: the bits, untouched
        for k in np.flatnonzero(length > 1):
            idx = order[head[k]:head[k] + length[k]]   # the run's list positions, ascending
            if dup == "first":
                continue
            if dup == "last":
                ob[k] = vb[idx[-1]]
                continue
            acc, at = v[idx[0]], idx[0]
            with np.errstate(all="ignore"):
                for t in idx[1:]:
                    x = v[t]
                    if dup == "plus":
                        acc = dtype(acc + x)
                    elif (x < acc) if dup == "min" else (x > acc):
                        acc, at = x, t
            if dup == "plus":
                out[k] = acc
            else:
                ob[k] = vb[at]
    folds = v is not None and dup in ("plus", "min", "max")
    stats["nnz_out"] = len(head)
    if folds:
        stats["long_runs"] = int((length > LONG_RUN).sum())
        if len(head) < nnz:
            stats["readbacks"] = 2
    rowptr = np.zeros(M + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rs[head], minlength=M))
    return (rowptr, cs[head].astype(np.uint32), out), stats, {"order": order, "head": head, "length": length}


# ---- the graph functions -----------------------------------------------------------------------------------------------------------
def _edges(n, rows, cols, weights, dtype):
    r, c = np.asarray(rows, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    if len(r) and (min(r.min(), c.min()) < 0 or max(r.max(), c.max()) >= n):
        raise ValueError(f"vertex ids must lie in [0, {n})")
    w = None if weights is None else np.asarray(weights, dtype).ravel()
    return r, c, w


def adjacency_matrix(n, rows, cols, weights=None, directed=False, loops=False, dup="min", dtype=np.float64):
    """graph.adjacency_matrix: (rowptr, col, val)."""
    r, c, w = _edges(n, rows, cols, weights, dtype)
    if not loops:
        keep = r != c
        r, c, w = r[keep], c[keep], (w[keep] if w is not None else None)
    if not directed:
        r, c, w = np.concatenate([r, c]), np.concatenate([c, r]), (np.concatenate([w, w]) if w is not None else None)
    return build(n, n, r, c, w, dup, dtype)[0]


def laplacian(n, rows, cols, weights=None, dtype=np.float64):
    """graph.laplacian: one build of the four blocks, in their order: (rowptr, col, val)."""
    dtype = np.dtype(dtype).type
    r, c, w = _edges(n, rows, cols, weights, dtype)
    keep = r != c
    u, v = r[keep], c[keep]
    w = w[keep] if w is not None else np.ones(len(u), dtype)
    return build(n, n, np.concatenate([u, v, u, v]), np.concatenate([v, u, u, v]), np.concatenate([-w, -w, w, w]), "plus", dtype)[0]


def _upper(csr):
    rowptr, col, _ = csr
    u = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    v = col.astype(np.int64)
    keep = u < v
    return u[keep], v[keep]


def incidence_matrix(n, rows, cols, dtype=np.float64):
    """graph.incidence_matrix: ((rowptr, col, val) of B, u, v)."""
    u, v = _upper(adjacency_matrix(n, rows, cols, dtype=dtype))
    e = np.arange(len(u), dtype=np.int64)
    return build(n, len(u), np.concatenate([u, v]), np.concatenate([e, e]), None, "error", dtype)[0], u, v


def line_graph(n, rows, cols, dtype=np.float64):
    """graph.line_graph: ((rowptr, col, val) of L, u, v): B^T B without its diagonal."""
    (rowptr, col, val), u, v = incidence_matrix(n, rows, cols, dtype)
    m = len(u)
    B = sp.csr_matrix((val.astype(np.float64), col.astype(np.int64), rowptr), shape=(n, m))
    P = sp.coo_matrix(B.T @ B)
    off = P.row != P.col
    L = sp.csr_matrix((P.data[off], (P.row[off], P.col[off])), shape=(m, m))
    L.sort_indices()
    return (L.indptr.astype(np.int64), L.indices.astype(np.uint32), L.data.astype(dtype)), u, v
