"""The numpy model of osp_csr_inflate_prune and of graph.markov_cluster (include/outerspace_spgemm_mcl.h): the defined
order of additions, the tie rule (among equal values the lower column wins), the rescue rule.  Not a test module: both
test_mcl_cpu.py and test_gpu_mcl.py import this one copy."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components


def ordered_sum(e):
    """p_l = e_l + e_{l+64} + ... left to right for l = 0..63, then p_l += p_{l+d} for l < d, d = 32, 16, .., 1; p_0."""
    e = np.asarray(e)
    dt = e.dtype
    m = len(e)
    pad = np.zeros((m + 63) // 64 * 64 if m else 64, dt)
    pad[:m] = e
    p = np.zeros(64, dt)
    for row in pad.reshape(-1, 64):
        p = p + row
    d = 32
    while d:
        p[:d] = p[:d] + p[d:2 * d]
        d //= 2
    return p[0]


def prune_row(v, thr, cap):
    """Indices (ascending) of the entries of one row that stay."""
    n = len(v)
    if n == 0:
        return np.zeros(0, np.int64), False, False
    cand = np.nonzero(v >= thr)[0]
    if len(cand) == 0:
        order = np.lexsort((np.arange(n), -v))      # largest value first, ties to the lower column
        return order[:1], False, True
    if cap and len(cand) > cap:
        order = np.lexsort((cand, -v[cand]))
        return np.sort(cand[order[:cap]]), True, False
    return cand, False, False


def inflate(v, power):
    dt = v.dtype.type
    if power == 1:
        return v.copy()
    if power == 2:
        return v * v
    return np.power(v, dt(power))


def inflate_prune(rowptr, colidx, vals, power=2.0, threshold=0.0, max_per_row=0):
    """-> (rowptr, colidx, vals, stats) of the step, vals' dtype throughout."""
    vals = np.asarray(vals)
    dt = vals.dtype.type
    thr = dt(threshold)
    M = len(rowptr) - 1
    out_ptr = np.zeros(M + 1, np.int64)
    cols, outs = [], []
    capped = rescued = 0
    chaos = dt(0)
    with np.errstate(under="ignore", invalid="ignore", divide="ignore"):
        for r in range(M):
            b, e = int(rowptr[r]), int(rowptr[r + 1])
            v = vals[b:e]
            keep, was_capped, was_rescued = prune_row(v, thr, max_per_row)
            capped += was_capped
            rescued += was_rescued
            out_ptr[r + 1] = out_ptr[r] + len(keep)
            if len(keep) == 0:
                continue
            w = inflate(v[keep], power)
            out = w / ordered_sum(w)
            c = out.max() - ordered_sum(out * out)
            if c > chaos:
                chaos = c
            cols.append(np.asarray(colidx[b:e])[keep])
            outs.append(out)
    col = np.concatenate(cols).astype(np.uint32) if cols else np.zeros(0, np.uint32)
    val = np.concatenate(outs).astype(vals.dtype) if outs else np.zeros(0, vals.dtype)
    stats = {"nnz_in": int(rowptr[M]), "nnz_out": int(out_ptr[M]), "rows_capped": capped, "rows_rescued": rescued, "chaos": float(chaos)}
    return out_ptr, col, val, stats


def walk_pattern(rows, cols, n, weights=None):
    """A + I as scipy CSR (float64): symmetric, no duplicate edges (the maximum of duplicate weights), self loops of weight 1
    (weighted: of the row's largest weight, 1 for an isolated vertex)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    w = np.ones(len(rows)) if weights is None else np.asarray(weights, np.float64)
    keep = rows != cols
    rows, cols, w = rows[keep], cols[keep], w[keep]
    best = {}
    for u, v, x in zip(np.concatenate([rows, cols]), np.concatenate([cols, rows]), np.concatenate([w, w])):
        k = (int(u), int(v))
        best[k] = max(best.get(k, -np.inf), x)
    loop = np.ones(n)
    if weights is not None:
        seen = np.zeros(n, bool)
        for (u, _), x in best.items():
            loop[u] = x if not seen[u] else max(loop[u], x)
            seen[u] = True
    for i in range(n):
        best[(i, i)] = loop[i]
    keys = sorted(best)
    A = sp.csr_matrix((np.array([best[k] for k in keys]), (np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64))),
                      shape=(n, n))
    A.sort_indices()
    return A


def labels_of(n, rowptr, colidx):
    g = sp.csr_matrix((np.ones(len(colidx), np.int8), np.asarray(colidx, np.int64), np.asarray(rowptr, np.int64)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    out = np.full(n, -1, np.int64)
    nxt = 0
    seen = {}
    for j in range(n):             # numbered in ascending order of the smallest vertex
        if lab[j] not in seen:
            seen[lab[j]] = nxt
            nxt += 1
        out[j] = seen[lab[j]]
    return out


def scipy_square(n, rowptr, colidx, vals):
    """T @ T with scipy (NOT the library's order of additions: for runs that only need the clustering)."""
    T = sp.csr_matrix((vals, np.asarray(colidx, np.int64), rowptr), shape=(n, n))
    C = (T @ T).tocsr()
    C.sort_indices()
    return C.indptr.astype(np.int64), C.indices.astype(np.uint32), C.data.astype(vals.dtype)


def markov_cluster(rows, cols, n, *, inflation=2.0, threshold=1e-4, max_per_row=1000, max_iter=100, tol=1e-6, weights=None,
                   dtype=np.float64, square=scipy_square):
    """The loop of graph.markov_cluster.  `square(n, rowptr, colidx, vals)` -> the CSR of T @ T (ascending columns); pass one
    that sums in ascending k to reproduce the library bit for bit.  -> (labels, info, (rowptr, colidx, vals) of the final T)."""
    A = walk_pattern(rows, cols, n, weights)
    rp, ci, va, st = inflate_prune(A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(dtype), 1.0, 0.0, 0)
    info = {"iterations": 0, "chaos": st["chaos"], "converged": False, "nnz_expanded": [], "nnz_kept": []}   # (judged after a step only)
    while not info["converged"] and info["iterations"] < max_iter:
        ep, ec, ev = square(n, rp, ci, va)
        rp, ci, va, st = inflate_prune(ep, ec, ev, inflation, threshold, max_per_row)
        info["iterations"] += 1
        info["nnz_expanded"].append(int(ep[-1]))
        info["nnz_kept"].append(st["nnz_out"])
        info["chaos"], info["converged"] = st["chaos"], st["chaos"] < tol
    return labels_of(n, rp, ci), info, (rp, ci, va)


def planted_partition(seed, nblocks=8, lo=5, hi=40, density=0.7):
    """Disjoint dense blocks of lo..hi vertices (density `density`, a spanning path in every block) plus n/10 random extra
    edges.  -> (n, rows, cols, truth labels numbered by smallest vertex)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, nblocks)
    n = int(sizes.sum())
    truth = np.repeat(np.arange(nblocks), sizes)
    rows, cols = [], []
    start = 0
    for s in sizes:
        s = int(s)
        iu, ju = np.triu_indices(s, 1)
        pick = rng.random(len(iu)) < density
        rows += [start + iu[pick], start + np.arange(s - 1)]
        cols += [start + ju[pick], start + np.arange(1, s)]
        start += s
    extra = n // 10
    rows.append(rng.integers(0, n, extra))
    cols.append(rng.integers(0, n, extra))
    return n, np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64), truth.astype(np.int64)
