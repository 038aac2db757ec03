"""The numpy model that judges osp_csr_transpose (include/outerspace_spgemm_transpose.h) and graph.strongly_connected: the
transpose is a STABLE sort of the entries by column -- the input is in row order, so ascending rows inside every column --
and the strongly connected component of a source is what it reaches forwards that it also reaches backwards."""
import numpy as np


def transpose(rowptr, col, val, ncol):
    """(rowptr, col, val) of the ncol x M transpose of an M x ncol CSR with ascending columns: values moved, never computed."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.uint32)
    M = len(rowptr) - 1
    row = np.repeat(np.arange(M, dtype=np.uint32), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(col.astype(np.int64), minlength=ncol))]).astype(np.int64)
    return out_ptr, row[order], np.asarray(val)[order]


def passes(ncol):
    """Radix passes of the sort path: 8-bit digits over the bits of ncol - 1, at least one."""
    return max(1, (max(int(ncol) - 1, 0).bit_length() + 7) // 8)


def directed_adjacency(rows, cols, n):
    """graph.weighted_adjacency(directed=True) with unit weights: self loops dropped, duplicates merged.  CSR (rowptr, col)."""
    r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    keep = r != c
    key = np.unique(r[keep] * n + c[keep])
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int64)
    return rowptr, (key % n).astype(np.uint32)


def _relax(rowptr, col, n, sources, max_iter):
    """The rounds of graph._relax_rounds under (MIN, PLUS) with unit weights, dense: D = the distances known, F = the
    entries that changed in the last round.  Returns (D with +inf where absent, rounds)."""
    S = len(sources)
    D = np.full((S, n), np.inf)
    D[np.arange(S), sources] = 0.0
    F = np.isfinite(D)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    rounds = 0
    while F.any() and rounds < max_iter:
        rounds += 1
        P = np.full((S, n), np.inf)
        for s in range(S):
            live = F[s][row]                                  # the edges that leave the frontier
            np.minimum.at(P[s], col[live], D[s][row[live]] + 1.0)
        F = P < D                                             # new, or better than what D holds
        D = np.minimum(D, P)
    return D, rounds


def strongly_connected(rows, cols, n, sources, max_iter=None):
    """graph.strongly_connected step by step: forwards on W, backwards on its transpose, the coordinates both hold."""
    sources = np.asarray(sources, np.int64)
    rowptr, col = directed_adjacency(rows, cols, n)
    max_iter = n if max_iter is None else max_iter
    fwd, rf = _relax(rowptr, col, n, sources, max_iter)
    tptr, tcol, _ = transpose(rowptr, col, np.ones(len(col)), n)
    bwd, rb = _relax(tptr, tcol, n, sources, max_iter)
    return np.isfinite(fwd) & np.isfinite(bwd), {"rounds_forward": rf, "rounds_backward": rb,
                                                  "nnz_forward": int(np.isfinite(fwd).sum()), "nnz_backward": int(np.isfinite(bwd).sum())}


def graphs():
    """The six directed graphs the component tests share: name -> (n, rows, cols)."""
    from outerspace_amd import generators as gen
    n8, r8, c8, _ = gen.rmat_coo(8, 4, "g500", seed=11)
    return {
        "cycle with a tail": (7, [0, 1, 2, 3, 3, 4, 5], [1, 2, 3, 0, 4, 5, 6]),
        "dag": (6, [0, 0, 1, 2, 3, 1], [1, 2, 3, 3, 4, 5]),
        "two cycles joined one way": (7, [0, 1, 2, 2, 3, 4, 5], [1, 2, 0, 3, 4, 5, 3]),
        "self loop": (4, [0, 1, 1, 2], [1, 1, 2, 0]),
        "isolated vertex": (5, [0, 1, 3], [1, 0, 0]),
        "rmat8": (n8, r8.astype(np.int64), c8.astype(np.int64)),
    }
