"""The numpy model of osp_csr_kron (include/outerspace_spgemm_kron.h) and of the graph functions built on it
(outerspace_amd/graph.py: tensor_product, cartesian_product, strong_product, kronecker_power).  A helper, not a test file.

The model of the product works on (rowptr, col, val) triples and shares nothing with the kernel's decode of an output
position: it walks the pairs of rows (ia, ib) in the order of out's rows and writes each pair's block with an explicit
``repeat`` of a's row and ``tile`` of b's row.  The models of the graph functions work on dense 0/1 matrices with
``numpy.kron`` and never touch the CSR model."""
import numpy as np

OPS = ("times", "plus", "min", "max", "first", "second")
COPY_OPS = ("min", "max", "first", "second")   # the result is one operand's bits
LAUNCHES = 2                                   # OSP_KRON_LAUNCHES
LIMIT = (1 << 32) - 1


def apply_op(op, x, y):
    """op(x, y) element by element as the library defines it (outerspace_spgemm_ewise.h): one IEEE operation in the dtype,
    or a copy of one operand's bits; MIN and MAX take y only where the comparison says so."""
    if op == "times":
        with np.errstate(all="ignore"):
            return x * y
    if op == "plus":
        with np.errstate(all="ignore"):
            return x + y
    if op == "min":
        return np.where(y < x, y, x)
    if op == "max":
        return np.where(y > x, y, x)
    if op == "first":
        return x.copy()
    if op == "second":
        return y.copy()
    raise ValueError(f"op must be one of {' '.join(OPS)}")


def kron(a, na, b, nb, op="times"):
    """a (x) b for a = (rowptr, col, val) with na columns and b likewise.  Returns ((rowptr, col, val), (M, N), stats):
    stats holds nnz_a, nnz_b, nnz_out, launches, readbacks and no_work.  Raises ValueError for what the library refuses
    with OSP_ERR_ARG and OverflowError for OSP_ERR_CAPACITY, the argument checks first."""
    if op not in OPS:
        raise ValueError(f"op must be one of {' '.join(OPS)}")
    (rpa, ca, va), (rpb, cb, vb) = a, b
    if va.dtype != vb.dtype:
        raise ValueError("the operands' dtypes differ")
    ma, mb = len(rpa) - 1, len(rpb) - 1
    M, N = ma * mb, int(na) * int(nb)
    if M >= LIMIT or N > LIMIT:
        raise ValueError("dimension exceeds the u32 index type")
    if len(ca) * len(cb) >= LIMIT:
        raise OverflowError("the product would hold 2^32 - 1 entries or more")
    dt = va.dtype
    # row lengths: the outer product of the operands' row lengths, summed up -- no closed form of a row's beginning
    lengths = np.outer(np.diff(rpa), np.diff(rpb)).reshape(-1).astype(np.int64)
    rowptr = np.concatenate([[0], lengths]).astype(np.int64)
    cols, vals = [], []
    view = np.uint32 if dt == np.float32 else np.uint64
    rows_b = np.flatnonzero(np.diff(rpb)).tolist()
    for ia in np.flatnonzero(np.diff(rpa)).tolist():   # (a pair with an empty row writes nothing)
        a0, a1 = int(rpa[ia]), int(rpa[ia + 1])
        for ib in rows_b:
            b0, b1 = int(rpb[ib]), int(rpb[ib + 1])
            la, lb = a1 - a0, b1 - b0
            # every entry of a's row against the whole of b's row, in a's order then b's
            col_a, col_b = np.repeat(ca[a0:a1].astype(np.int64), lb), np.tile(cb[b0:b1].astype(np.int64), la)
            cols.append(col_a * int(nb) + col_b)
            x, y = np.repeat(va[a0:a1], lb), np.tile(vb[b0:b1], la)
            # (repeat and tile move bits: the special values keep their payloads)
            assert np.array_equal(x.view(view), np.repeat(va[a0:a1].view(view), lb))
            vals.append(apply_op(op, x, y))
    rowptr = np.cumsum(rowptr)
    col = np.concatenate(cols).astype(np.uint32) if cols else np.zeros(0, np.uint32)
    val = np.concatenate(vals).astype(dt) if vals else np.zeros(0, dt)
    no_work = M == 0 or len(ca) == 0 or len(cb) == 0
    stats = {"nnz_a": len(ca), "nnz_b": len(cb), "nnz_out": len(col), "launches": 0 if no_work else LAUNCHES, "readbacks": 0,
             "no_work": no_work}
    assert len(col) == len(ca) * len(cb)
    return (rowptr, col, val), (M, N), stats


def closed_form_rowptr(rpa, rpb):
    """out's row pointers as the header states them: row ia mB + ib begins at rpA[ia] nnzB + lenA[ia] rpB[ib]."""
    rpa, rpb = np.asarray(rpa, np.int64), np.asarray(rpb, np.int64)
    ma, mb = len(rpa) - 1, len(rpb) - 1
    nnzb = int(rpb[-1])
    body = (rpa[:-1, None] * nnzb + np.diff(rpa)[:, None] * rpb[None, :-1]).reshape(-1) if ma and mb else np.zeros(0, np.int64)
    return np.concatenate([body, [int(rpa[-1]) * nnzb]]).astype(np.int64)


# ---- the graph functions, on dense matrices -------------------------------------------------------------------------------------
def adjacency(rows, cols, n, directed=False, loops=False):
    """graph.adjacency_matrix with unit weights as a dense 0/1 matrix."""
    A = np.zeros((n, n), np.float64)
    for u, v in zip(np.asarray(rows, np.int64).tolist(), np.asarray(cols, np.int64).tolist()):
        if u == v and not loops:
            continue
        A[u, v] = 1.0
        if not directed:
            A[v, u] = 1.0
    return A


def _csr(D):
    """A dense matrix of non-negative values as (rowptr, col, val): its non-zeros."""
    r, c = np.nonzero(D)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=D.shape[0]))]).astype(np.int64)
    return rowptr, c.astype(np.uint32), D[r, c]


def _parts(g, h, directed):
    (r1, c1, n1), (r2, c2, n2) = g, h
    return adjacency(r1, c1, n1, directed, directed), adjacency(r2, c2, n2, directed, directed)


def tensor_product(g, h, directed=False):
    A, B = _parts(g, h, directed)
    return _csr(np.kron(A, B))


def cartesian_product(g, h, directed=False):
    A, B = _parts(g, h, directed)
    return _csr(np.kron(A, np.eye(len(B))) + np.kron(np.eye(len(A)), B))


def strong_product(g, h, directed=False):
    A, B = _parts(g, h, directed)
    return _csr(np.kron(A, B) + np.kron(A, np.eye(len(B))) + np.kron(np.eye(len(A)), B))


def kronecker_power(rows, cols, n, k, directed=False, loops=True):
    A = adjacency(rows, cols, n, directed, loops)
    out = A
    for _ in range(k - 1):
        out = np.kron(out, A)
    return _csr(out)


def triangles(csr):
    """Triangles of a loop-free symmetric pattern: trace(A^3) / 6."""
    rowptr, col, _ = csr
    n = len(rowptr) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rowptr)), col.astype(np.int64)] = 1.0
    return int(round(np.trace(A @ A @ A))) // 6
