"""Numpy models that judge osp_csr_ewise and graph.personalized_pagerank (checkers only; nothing here runs on the GPU).

``ewise`` follows include/outerspace_spgemm_ewise.h rule by rule: structural patterns (an explicit or computed zero is an
entry), one numpy operation of the operands' dtype where both hold a coordinate, and a copy of the bits everywhere else.
``ppr`` is the truncated series of ``graph.personalized_pagerank``: the same step count, the same operand values
(alpha / deg), the same ``select("ge", prune)``, with scipy's product in place of the library's."""
import numpy as np
import scipy.sparse as sp

MODES = ["union", "intersect"]
OPS = ["plus", "times", "min", "max", "first", "second", "minus", "div"]       # in the enum's order
UNION_OPS = OPS[:6]                                                            # minus and div are refused under union
COPY_OPS = ("min", "max", "first", "second")                                   # the result is a copy of one operand's bits


def _keys(rowptr, col, ncol):
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    return row * np.int64(ncol) + col.astype(np.int64)


def apply_op(op, a, b):
    """op(a, b) on arrays of one dtype: ONE operation of that dtype, or a copy of one operand."""
    with np.errstate(all="ignore"):
        if op == "plus":
            return a + b
        if op == "times":
            return a * b
        if op == "minus":
            return a - b
        if op == "div":
            return a / b
        if op == "min":
            return np.where(b < a, b, a)     # a NaN on either side: the comparison is false, a stays
        if op == "max":
            return np.where(b > a, b, a)
        if op == "first":
            return a.copy()
        if op == "second":
            return b.copy()
    raise ValueError(op)


class Plan:
    """Where the two patterns meet: computed once for a pair, then every mode and op is a gather."""

    def __init__(self, a, b, ncol):
        (self.a_ptr, self.a_col, self.a_val), (self.b_ptr, self.b_col, self.b_val) = a, b
        assert len(self.a_ptr) == len(self.b_ptr) and self.a_val.dtype == self.b_val.dtype
        self.M, self.ncol = len(self.a_ptr) - 1, ncol
        ka, kb = _keys(self.a_ptr, self.a_col, ncol), _keys(self.b_ptr, self.b_col, ncol)
        assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0), "columns must ascend strictly in every row"
        self.ka, self.kb = ka, kb
        q = np.searchsorted(kb, ka)
        self.a_hit = np.zeros(len(ka), bool)
        inside = q < len(kb)
        self.a_hit[inside] = kb[q[inside]] == ka[inside]
        self.a_q = q                                   # (meaningful where a_hit)
        self.b_hit = np.zeros(len(kb), bool)
        self.b_hit[q[self.a_hit]] = True
        self.nnz_both = int(self.a_hit.sum())
        self._patterns = {}

    def _rowptr(self, keys):
        ptr = np.zeros(self.M + 1, np.int64)
        if self.M:
            ptr[1:] = np.cumsum(np.bincount(keys // self.ncol, minlength=self.M))
        return ptr

    def _pattern(self, mode):
        """(rowptr, col) of the mode's result and, for the union, where a's entries and b's own entries go (computed once)."""
        if mode not in self._patterns:
            if mode == "intersect":
                keys, where = self.ka[self.a_hit], None
            else:
                own = self.kb[~self.b_hit]
                # an entry's place: its own position plus the other side's entries before it
                pos_a = np.arange(len(self.ka)) + np.searchsorted(own, self.ka)
                pos_b = np.arange(len(own)) + np.searchsorted(self.ka, own)
                keys = np.empty(len(self.ka) + len(own), np.int64)
                keys[pos_a], keys[pos_b] = self.ka, own
                assert np.all(np.diff(keys) > 0)
                where = (pos_a, pos_b)
            self._patterns[mode] = (self._rowptr(keys), (keys % self.ncol).astype(np.uint32), where)
        return self._patterns[mode]

    def result(self, mode, op):
        """(rowptr, col, val, computed): ``computed`` marks the entries whose value is op(a, b) and not a copy."""
        if mode not in MODES or op not in OPS or (mode == "union" and op not in UNION_OPS):
            raise ValueError((mode, op))
        both = apply_op(op, self.a_val[self.a_hit], self.b_val[self.a_q[self.a_hit]])
        rowptr, col, where = self._pattern(mode)
        if mode == "intersect":
            return rowptr, col, both, np.ones(len(col), bool)
        pos_a, pos_b = where
        val, computed = np.empty(len(col), self.a_val.dtype), np.zeros(len(col), bool)
        va = self.a_val.copy()
        va[self.a_hit] = both
        val[pos_a], val[pos_b] = va, self.b_val[~self.b_hit]
        computed[pos_a] = self.a_hit
        return rowptr, col, val, computed


def ewise(a, b, ncol, mode, op):
    """a, b: (rowptr, col, val) of one shape and dtype.  Returns (rowptr, col, val)."""
    return Plan(a, b, ncol).result(mode, op)[:3]


# ---- personalised PageRank ---------------------------------------------------------------------------------------------------
def ppr_steps(alpha, tol, max_iter=None):
    """The smallest k with alpha^(k+1) < tol, capped by max_iter."""
    k = 0
    while alpha ** (k + 1) >= tol:
        k += 1
    return k if max_iter is None else min(k, max_iter)


def _as_triple(m):
    m = m.tocsr()
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.uint32), m.data.astype(np.float64)


def ppr(adj, sources, alpha=0.85, tol=1e-6, max_iter=None, prune=0.0):
    """adj: the symmetric unit adjacency as scipy CSR (tests/bfs_model.symmetric_adjacency).  Returns (dense [S, n], info):
    info = steps (K), iterations, frontiers (every F_k, k >= 1, after the select, as scipy CSR) and products (before it)."""
    n = adj.shape[0]
    src = np.asarray(sources, np.int64).ravel()
    S = len(src)
    K = ppr_steps(alpha, tol, max_iter)
    deg = np.diff(adj.indptr).astype(np.float64)
    W = adj.astype(np.float64).tocsr(copy=True)
    with np.errstate(divide="ignore"):      # (an isolated vertex has no entry to hold its infinity)
        W.data = (alpha / deg)[np.repeat(np.arange(n), np.diff(adj.indptr))]
    F = sp.csr_matrix((np.full(S, 1.0 - alpha), src, np.arange(S + 1)), shape=(S, n))
    total = _as_triple(F)
    info = {"steps": K, "iterations": 0, "frontiers": [], "products": []}
    for _ in range(K):
        F = (F @ W).tocsr()
        F.sort_indices()
        info["products"].append(F.copy())
        if prune > 0.0:
            keep = F.data >= prune
            rows = np.repeat(np.arange(S), np.diff(F.indptr))[keep]
            F = sp.csr_matrix((F.data[keep], (rows, F.indices[keep])), shape=(S, n))
            F.sort_indices()
        info["frontiers"].append(F)
        info["iterations"] += 1
        if F.nnz == 0:
            break
        total = ewise(total, _as_triple(F), n, "union", "plus")
    dense = np.zeros((S, n))
    rows = np.repeat(np.arange(S), np.diff(total[0]))
    dense[rows, total[1].astype(np.int64)] = total[2]
    return dense, info
