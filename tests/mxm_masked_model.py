"""The numpy model of osp_csr_mxm_masked (include/outerspace_spgemm_mxm_masked.h) and of graph.bfs_parents.

The masked product is the header's contract, taken literally: ``semiring_model.mxm`` of the operands, then a numpy filter of
the output's (row, column) pairs against the mask's.  ``products_kept`` is counted from the UNFOLDED product list -- every
product of an admitted coordinate -- so it shares nothing with the fold.  The BFS is plain Python, level by level: the parent
of a vertex reached on level d is the smallest id among its in-neighbours on level d - 1."""
import numpy as np

from tests import semiring_model as model

ADD_OPS, MUL_OPS, SHORT_CAP, BATCH = model.ADD_OPS, model.MUL_OPS, model.SHORT_CAP, model.BATCH


def _keys(rowptr, col, ncol):
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr)) * ncol + col.astype(np.int64)


def product_columns(a, b):
    """The (row, column) of every formed product of a x b, in the library's (row, k, column) order."""
    ap, ac = np.asarray(a[0]), np.asarray(a[1]).astype(np.int64)
    bp, bc = np.asarray(b[0]), np.asarray(b[1])
    lens = (bp[ac + 1] - bp[ac]).astype(np.int64)
    arow = np.repeat(np.arange(len(ap) - 1, dtype=np.int64), np.diff(ap))
    P = int(lens.sum())
    pa = np.repeat(np.arange(len(ac), dtype=np.int64), lens)
    within = np.arange(P, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(arow, lens), bc[bp[ac[pa]] + within].astype(np.int64)


def filter_product(full, st, a, b, mask, ncol, complement=False):
    """The masked product from the plain one: ``full`` = (rowptr, col, val) and ``st`` as semiring_model.mxm returns them for
    a and b.  Returns ((rowptr int64, col uint32, val), stats): st's products, short_rows, long_rows and batches (they do not
    depend on the mask), with nnz_out of the masked result, nnz_mask and products_kept."""
    rowptr, col, val = full
    M = len(rowptr) - 1
    mkeys = _keys(mask[0], mask[1], ncol)
    keep = np.isin(_keys(rowptr, col, ncol), mkeys) != bool(complement)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr))[keep]
    out_ptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=M), out=out_ptr[1:])
    prow, pcol = product_columns(a, b)
    kept = int((np.isin(prow * ncol + pcol, mkeys) != bool(complement)).sum())
    st = dict(st, nnz_out=int(keep.sum()), nnz_mask=len(mask[1]), products_kept=kept)
    return (out_ptr, col[keep], val[keep]), st


def mxm_masked(a, b, mask, ncol, complement=False, add="plus", mul="times", cap=SHORT_CAP, budget=BATCH):
    """a, b as semiring_model.mxm takes them; mask = (rowptr, col[, anything]) of shape M x ncol: ``filter_product`` of
    ``semiring_model.mxm``."""
    full, st = model.mxm(a, b, ncol, add, mul, cap, budget)
    return filter_product(full, st, a, b, mask, ncol, complement)


def dense_masked(A, hasA, B, hasB, hasM, complement, add, mul):
    """A brute force that shares nothing with the above: dense operands with presence arrays, three loops, the fold in
    ascending k from the first product.  Returns (has, val) dense."""
    M, K = A.shape
    N = B.shape[1]
    has, out = np.zeros((M, N), bool), np.zeros((M, N), A.dtype)
    for i in range(M):
        for j in range(N):
            if bool(hasM[i, j]) == bool(complement):
                continue
            acc = None
            for k in range(K):
                if hasA[i, k] and hasB[k, j]:
                    p = model.op(mul, A[i:i + 1, k], B[k:k + 1, j])
                    acc = p if acc is None else model.op(add, acc, p)
            if acc is not None:
                has[i, j], out[i, j] = True, acc[0]
    return has, out


# ---- breadth-first parents --------------------------------------------------------------------------------------------------------
def adjacency_lists(rows, cols, n, directed=False):
    """out-neighbour sets as graph._pattern_result builds the matrix: undirected drops self loops and holds every edge in
    both directions; directed keeps the edges as given."""
    nbr = [set() for _ in range(n)]
    for u, v in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist()):
        if directed:
            nbr[u].add(v)
        elif u != v:
            nbr[u].add(v)
            nbr[v].add(u)
    return nbr


def bfs_parents(rows, cols, n, sources, directed=False, max_levels=None):
    """Returns (parent int64 [S, n], level int32 [S, n], levels): the minimum-id parent, -1 where unreached; ``levels`` is the
    deepest level reached over all sources."""
    nbr = adjacency_lists(rows, cols, n, directed)
    src = np.atleast_1d(np.asarray(sources, np.int64)).ravel()
    parent = np.full((len(src), n), -1, np.int64)
    level = np.full((len(src), n), -1, np.int32)
    deepest = 0
    for s, root in enumerate(src.tolist()):
        parent[s, root], level[s, root] = root, 0
        frontier, d = [root], 0
        while frontier and (max_levels is None or d < max_levels):
            d += 1
            found = {}
            for k in sorted(frontier):            # ascending k: the first to reach v is the smallest
                for v in nbr[k]:
                    if level[s, v] < 0 and v not in found:
                        found[v] = k
            for v, k in found.items():
                parent[s, v], level[s, v] = k, d
            frontier = list(found)
            if frontier:
                deepest = max(deepest, d)
    return parent, level, deepest
