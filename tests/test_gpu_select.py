"""osp_csr_select on the GPU against the numpy model of tests/truss_model.py: row pointers and columns exact, value BITS equal
(compared as unsigned integers), all ten predicates, with and without fill, f32 and f64, on the inputs built for every rule
of the mask filter (tests/test_gpu_apply_mask.py: the same shapes and special values), on a product's result, through the
result's other entry points, and its errors."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import test_gpu_apply_mask as am   # the input builders only
from tests import truss_model as model

pytestmark = pytest.mark.gpu

DEV = am.DEV
CHUNK = am.CHUNK
_bits, _upload = am._bits, am._upload
VALUE_OPS, POSITION_OPS = list(model.VALUE_OPS), list(model.POSITION_OPS)


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _denormal_threshold(dt):
    """Half of the positive denormal among am._special's values, exact as a double: only an unflushed comparison tells the
    denormal from 0."""
    v = am._special(dt)
    d = v[(v > 0) & (v < np.finfo(dt).tiny)].max()
    return float(d) / 2


# per input: thresholds of the value predicates, diagonals of the position predicates (every predicate must both keep and
# remove something for at least one of them: test_select_equals_model checks that)
def _params(case, dt, ncol, nrow):
    thresholds, diags = [0.25], [0, ncol // 2]
    if case == "traps":
        thresholds += [0.0, -0.0, np.nan, np.inf, -np.inf, _denormal_threshold(dt), 0.1]
        diags += [-5, 30000, ncol, 1 << 40, -(1 << 62), (1 << 63) - 1, -(1 << 63)]
    if case == "short_rows":
        diags = [0, 2000, -100000, -(nrow - 1)]
    if case == "frontier":
        diags = [1 << 20, 0]
    return thresholds, diags


CASES = ("traps", "frontier", "short_rows", "empty_in", "same_pattern", "no_rows")


def _input(case, dt):
    """The mask filter's input of that name with every third ordinary value set to 0.25, so that eq / ne (and lt against
    le) have something to tell apart; NaNs, infinities, zeros, denormals and the largest number stay where they are."""
    ncol, (rowptr, col, val), _ = am.CASES[case](dt)
    val = val.copy()
    ordinary = np.isfinite(val) & (np.abs(val) > 1e-30) & (np.abs(val) < 1e30)
    val[ordinary & (np.arange(len(val)) % 3 == 0)] = 0.25
    return ncol, (rowptr, col, val)


def _check(res, st, ncol, csr, op, threshold=0.0, diag=0, fill=None):
    want_ptr, want_col, want_val = model.select(*csr, op, threshold, diag, fill)
    assert res.shape == (len(csr[0]) - 1, ncol) and res.dtype == csr[2].dtype.type
    assert res.nnz == len(want_col) == res.info["nnz_c"]
    assert np.array_equal(res.rowptr, want_ptr)
    assert np.array_equal(res.colidx, want_col)
    assert np.array_equal(_bits(res.vals), _bits(want_val))
    assert (st["nnz_in"], st["nnz_out"]) == (len(csr[1]), len(want_col))
    assert st["ms_total"] >= 0 and (st["launches"] > 0) == (len(csr[1]) > 0)
    return len(want_col)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_select_equals_model_bit_for_bit(mctx, case, dt):
    ncol, csr = _input(case, dt)
    nnz = len(csr[1])
    src = _upload(mctx, ncol, csr)
    thresholds, diags = _params(case, dt, ncol, len(csr[0]) - 1)
    kept = {}
    try:
        for fill in (None, 2.5, 0.1):
            for op in VALUE_OPS + POSITION_OPS:
                for x in (thresholds if op in VALUE_OPS else diags):
                    kw = {"threshold": x} if op in VALUE_OPS else {"diag": x}
                    res, st = src.select(op, fill=fill, **kw)
                    try:
                        kept.setdefault(op, []).append(_check(res, st, ncol, csr, op, fill=fill, **kw))
                    finally:
                        res.close()
        # `in` stays valid and untouched
        src._host = None   # (read it again)
        rp, c, v = src.to_host()
        assert np.array_equal(rp, csr[0]) and np.array_equal(c, csr[1]) and np.array_equal(_bits(v), _bits(csr[2]))
    finally:
        src.close()
    if case in ("traps", "frontier", "short_rows"):
        for op in ("lt", "le", "gt", "ge", "eq", "ne", "tril", "triu"):     # each keeps and removes a fair share somewhere
            assert any(0.1 * nnz < k < 0.9 * nnz for k in kept[op]), (op, kept[op])
    if case == "traps":
        assert 0 in kept["eq"] and 6 in kept["eq"]      # (a NaN threshold; +-0.0 == 0.0 == -0.0: three copies of the two zeros)
        assert nnz in kept["ne"] and nnz in kept["triu"] and 0 in kept["tril"]
    if case == "short_rows":
        assert any(0 < k < nnz for k in kept["diag"])


def test_denormals_and_inexact_thresholds_are_compared_as_doubles(mctx):
    for dt in (np.float32, np.float64):
        sp_ = am._special(dt)
        val = np.concatenate([sp_, np.full(5, 0.1, dt)])
        csr = (np.array([0, len(val)], np.int64), np.arange(len(val), dtype=np.uint32), val)
        src = _upload(mctx, 64, csr)
        try:
            thr = _denormal_threshold(dt)
            n_den = {}
            for op, x in (("gt", thr), ("lt", -0.0), ("gt", 0.1), ("eq", 0.1), ("le", 0.1), ("eq", float(dt(0.1)))):
                res, st = src.select(op, x)
                n_den[(op, x)] = _check(res, st, 64, csr, op, x)
                res.close()
            # +inf, the positive denormal, the largest number, 1 and the five 0.1 are above half the denormal; the smallest
            # denormal (bits 1) is not
            assert n_den[("gt", thr)] == 9
            assert n_den[("lt", -0.0)] == 2          # -inf and the negative denormal; -0.0 is not below -0.0
            # 0.1f widened is above the double 0.1; the double 0.1 equals it
            assert n_den[("eq", 0.1)] == (0 if dt == np.float32 else 5) and n_den[("eq", float(dt(0.1)))] == 5
            assert n_den[("gt", 0.1)] == (8 if dt == np.float32 else 3)    # +inf, the largest number, 1 (and 0.1f)
        finally:
            src.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_positions_next_to_the_diagonal_of_short_rows(mctx, dt):
    """Many short rows of a square matrix, every entry within 3 columns of the diagonal: an entry whose row is off by one
    changes its verdict for diag in {-1, 0, 1}, so a row search that errs anywhere -- at a chunk boundary, in a run of
    empty rows -- shows."""
    n = 3 * CHUNK + 777
    rng = np.random.default_rng(17)
    keep = rng.random((n, 7)) < 0.6                      # columns row - 3 .. row + 3, about 4 a row
    keep[rng.random(n) < 0.1] = False                    # and runs of empty rows
    row, off = np.nonzero(keep)
    col = row + off - 3
    inside = (col >= 0) & (col < n)
    row, col = row[inside], col[inside].astype(np.uint32)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    csr = (rowptr, col, rng.standard_normal(len(col)).astype(dt))
    nnz = len(col)
    assert nnz > 5 * CHUNK and np.any(np.diff(rowptr) == 0)
    src = _upload(mctx, n, csr)
    try:
        for op in POSITION_OPS:
            for d in (-1, 0, 1):
                for fill in (None, 1.0):
                    res, st = src.select(op, diag=d, fill=fill)
                    try:
                        k = _check(res, st, n, csr, op, diag=d, fill=fill)
                    finally:
                        res.close()
                    assert 0.05 * nnz < k < 0.95 * nnz, (op, d, k)
    finally:
        src.close()


def test_fill_beyond_the_dtype_is_infinity(mctx):
    res = am._small_result(mctx)
    csr = (res.rowptr.copy(), res.colidx.copy(), res.vals.copy())
    try:
        for dt_res, big in ((res, 1e308 * 10), (res, -np.inf)):
            out, st = dt_res.select("ne", np.nan, fill=big)
            _check(out, st, 4, csr, "ne", np.nan, fill=big)
            out.close()
    finally:
        res.close()
    val = np.array([1.0, 2.0, 3.0], np.float32)
    csr = (np.array([0, 2, 3], np.int64), np.array([0, 3, 1], np.uint32), val)
    src = _upload(mctx, 4, csr)
    try:
        for big, want in ((1e39, np.inf), (-3.5e38, -np.inf), (3.4e38, np.float32(3.4e38)), (float(np.finfo(np.float32).max), np.finfo(np.float32).max)):
            out, _ = src.select("ge", 0.0, fill=big)
            assert out.nnz == 3 and np.all(out.vals == np.float32(want)), big
            out.close()
    finally:
        src.close()


def _keys(res_or_csr, ncol):
    rp, c, v = res_or_csr if isinstance(res_or_csr, tuple) else res_or_csr.to_host()
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    return row * ncol + c.astype(np.int64), _bits(v)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_predicates_partition_the_input(mctx, dt):
    ncol, csr, _ = am._traps(dt)
    clean = (csr[0], csr[1], np.where(np.isnan(csr[2]), dt(0.5), csr[2]).astype(dt))

    def union_is_input(src, a, b, of):
        ra, _ = src.select(a[0], **a[1])
        rb, _ = src.select(b[0], **b[1])
        try:
            ka, va = _keys(ra, ncol)
            kb, vb = _keys(rb, ncol)
            assert len(np.intersect1d(ka, kb, assume_unique=True)) == 0
            allk = np.concatenate([ka, kb])
            order = np.argsort(allk, kind="stable")
            wk, wv = _keys(of, ncol)
            assert np.array_equal(allk[order], wk) and np.array_equal(np.concatenate([va, vb])[order], wv)
            return ra.nnz, rb.nnz
        finally:
            ra.close()
            rb.close()

    src = _upload(mctx, ncol, csr)
    try:
        for thr in (0.0, 0.3, np.nan):
            union_is_input(src, ("eq", {"threshold": thr}), ("ne", {"threshold": thr}), csr)
        for d in (-3, 0, 1, 30000, ncol - 1, 1 << 35, -(1 << 35)):
            union_is_input(src, ("tril", {"diag": d}), ("triu", {"diag": d + 1}), csr)
            union_is_input(src, ("diag", {"diag": d}), ("offdiag", {"diag": d}), csr)
        a, b = union_is_input(src, ("tril", {"diag": 30000}), ("triu", {"diag": 30001}), csr)
        assert a > 0 and b > 0
        # with NaNs in the input lt and ge lose them
        lt, _ = src.select("lt", 0.3)
        ge, _ = src.select("ge", 0.3)
        assert lt.nnz + ge.nnz == len(csr[1]) - int(np.isnan(csr[2]).sum())
        lt.close()
        ge.close()
    finally:
        src.close()
    src = _upload(mctx, ncol, clean)
    try:
        for thr in (0.0, 0.3, -np.inf, np.inf):
            union_is_input(src, ("lt", {"threshold": thr}), ("ge", {"threshold": thr}), clean)
            union_is_input(src, ("le", {"threshold": thr}), ("gt", {"threshold": thr}), clean)
    finally:
        src.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_upper_triangle_of_a_symmetric_self_product(ctx, dt):
    n, r, c, _ = gen.rmat_coo(11, 8, "g500", seed=5)
    A = sp.coo_matrix((np.ones(len(r), dt), (r, c)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(dt).tocsr()
    A.sort_indices()
    arrs = (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data)
    prod = ctx.spgemm_csc_csr(n, n, n, *arrs, *arrs)       # A symmetric: its CSR is its CSC
    try:
        up, st = prod.select("triu", diag=1)
        low, _ = prod.select("tril", diag=-1)
        try:
            want = sp.triu(prod.to_scipy(), k=1).tocsr()
            want.sort_indices()
            assert 0.3 * prod.nnz < up.nnz < 0.5 * prod.nnz and up.nnz == low.nnz == want.nnz
            assert np.array_equal(up.rowptr, want.indptr) and np.array_equal(up.colidx, want.indices)
            assert np.array_equal(_bits(up.vals), _bits(want.data.astype(dt)))
            assert (low.to_scipy().T != up.to_scipy()).nnz == 0      # the product of a symmetric matrix with itself is symmetric
            # counts of a 0/1 matrix are whole numbers: ge 2, fill 1 is the pattern of the entries with at least two paths
            two, _ = prod.select("ge", 2.0, fill=1.0)
            P = prod.to_scipy()
            assert two.nnz == int((P.data >= 2).sum()) and np.all(two.vals == 1) and 0 < two.nnz < prod.nnz
            two.close()
        finally:
            up.close()
            low.close()
    finally:
        prod.close()


# ---- error paths ------------------------------------------------------------------------------------------------------------
def _raw(res, sel, out=True):
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    stats = _lib.SelectStats()
    stats.nnz_in = 77
    st = _lib.lib().osp_csr_select(res._h if res is not None else None, ctypes.byref(sel) if sel is not None else None,
                                   ctypes.byref(o) if out else None, ctypes.byref(stats))
    return st, o.value == sentinel and stats.nnz_in == 77


def _sel(op=0, **kw):
    s = _lib.Select()
    s.op = op
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_argument_errors(mctx):
    res = am._small_result(mctx)
    try:
        assert _raw(res, None) == (_lib.ERR_ARG, True)                       # null sel
        assert _raw(res, _sel(), out=False)[0] == _lib.ERR_ARG               # null out
        assert _raw(None, _sel()) == (_lib.ERR_ARG, True)                    # null in
        for op in (-1, 10, 1 << 20):                                         # an op outside the enum
            assert _raw(res, _sel(op)) == (_lib.ERR_ARG, True)
            assert _lib.lib().osp_last_error_string()
        for word in range(8):                                                # a reserved word that is not 0
            s = _sel(3)
            s.reserved[word] = 1
            assert _raw(res, s) == (_lib.ERR_ARG, True)
        # every op of the enum is taken, and stats may be null
        for op in range(10):
            o = ctypes.c_void_p()
            s = _sel(op)
            assert _lib.lib().osp_csr_select(res._h, ctypes.byref(s), ctypes.byref(o), None) == 0
            S.CsrResult(mctx, o).close()
        with pytest.raises(ValueError):
            res.select("between")
        with pytest.raises(ValueError):
            res.select(3)
    finally:
        res.close()


def test_partials_result_is_refused(ctx):
    mctx = ctx
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    ts = [am._dev(x) for x in (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, B.indptr.astype(np.int64),
                               B.indices.astype(np.uint32), B.data)]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        assert _raw(part, _sel(3)) == (_lib.ERR_ARG, True)
    finally:
        part.close()


# ---- composition --------------------------------------------------------------------------------------------------------------
def test_select_result_composes(mctx):
    ncol = 3000
    rowptr, col, val = am._csr_from_lengths([5, 0, 700, 2500, 64], ncol, np.float64, seed=41)
    val = np.abs(val) + 0.1
    csr = (rowptr, col, val)
    mask = am._mask_for(rowptr, col, ncol, seed=42, share=0.7)
    src = _upload(mctx, ncol, csr)
    try:
        # select of a select
        a, st = src.select("gt", 0.5)
        w1 = model.select(*csr, "gt", 0.5)
        _check(a, st, ncol, csr, "gt", 0.5)
        b, st = a.select("triu", diag=1000)
        _check(b, st, ncol, w1, "triu", diag=1000)
        assert 0 < b.nnz < a.nnz < src.nnz
        # of an apply_mask, and into one
        m, _ = src.apply_mask(mask, space="host")
        mh = (m.rowptr.copy(), m.colidx.copy(), m.vals.copy())
        c, st = m.select("le", 0.9, fill=1.0)
        _check(c, st, ncol, mh, "le", 0.9, fill=1.0)
        d, ms = a.apply_mask(mask, complement=True, space="host")
        from tests import bfs_model
        wd = bfs_model.apply_mask(*w1, *mask, ncol, True)
        assert np.array_equal(d.rowptr, wd[0]) and np.array_equal(d.colidx, wd[1]) and np.array_equal(_bits(d.vals), _bits(wd[2]))
        assert 0 < d.nnz < a.nnz and 0 < c.nnz < m.nnz
        # into an inflate_prune (power 1, no pruning: the rows divided by their sums)
        t, ps = b.inflate_prune(1.0, 0.0, 0)
        assert ps["nnz_in"] == ps["nnz_out"] == b.nnz and np.array_equal(t.rowptr, b.rowptr) and np.array_equal(t.colidx, b.colidx)
        sums = np.add.reduceat(t.vals, t.rowptr[:-1][np.diff(t.rowptr) > 0])
        assert np.allclose(sums, 1.0, rtol=1e-12)
        # of a bias_relu
        bias = np.where(np.arange(ncol) % 3 == 0, -10.0, 0.5)
        br = src.bias_relu(bias, True)
        brh = (br.rowptr.copy(), br.colidx.copy(), br.vals.copy())
        e, st = br.select("ge", 1.0)
        _check(e, st, ncol, brh, "ge", 1.0)
        assert 0 < e.nnz < br.nnz
        # the other entry points of a result
        rows = torch.empty(e.nnz, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(DEV)
        e.coo_rows_into(rows.data_ptr())
        assert np.array_equal(rows.cpu().numpy(), np.repeat(np.arange(len(rowptr) - 1), np.diff(e.rowptr)))
        assert e.to_scipy().nnz == e.nnz and e.info["M"] == len(rowptr) - 1 and e.info["N"] == ncol
        # info is in's with nnz_c and ms_total replaced
        for k, v in src.info.items():
            if k not in ("nnz_c", "ms_total"):
                assert a.info[k] == v, k
        for x in (a, b, m, c, d, t, br, e):
            x.close()
    finally:
        src.close()


def test_fifty_back_to_back_calls_give_the_same_arrays(mctx):
    """Recycled pool buffers carry nothing over from call to call."""
    ncol, csr, _ = am._traps(np.float32)
    src = _upload(mctx, ncol, csr)
    variants = [("ge", {"threshold": 0.25}, None), ("triu", {"diag": 30000}, None), ("lt", {"threshold": 0.25}, 1.0),
                ("offdiag", {"diag": 20000}, 7.0)]
    try:
        first = {}
        for i in range(50):
            op, kw, fill = variants[i % len(variants)]
            res, st = src.select(op, fill=fill, **kw)
            got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["nnz_out"])
            res.close()
            if op not in first:
                first[op] = got
                w = model.select(*csr, op, kw.get("threshold", 0.0), kw.get("diag", 0), fill)
                assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and np.array_equal(got[2], _bits(w[2]))
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, first[op])), i
        src._host = None
        assert np.array_equal(_bits(src.to_host()[2]), _bits(csr[2]))
    finally:
        src.close()


def test_select_reports_its_launches(mctx):
    """Flag, scan, row pointers and, when anything is kept, the write kernel (am.SCAN_SMALL_MAX: where the scan takes three)."""
    for (ncol, csr, scan), nnz in zip(am._launch_inputs(), (am.SCAN_SMALL_MAX, am.SCAN_SMALL_MAX + 1)):
        assert len(csr[1]) == nnz
        src = am._upload(mctx, ncol, csr)
        try:
            for op, kw, fill, kept in (("gt", {"threshold": 0.0}, None, "some"), ("gt", {"threshold": 0.0}, 1.0, "some"),
                                       ("tril", {"diag": ncol}, None, "all"), ("gt", {"threshold": 1e30}, None, "none"),
                                       ("triu", {"diag": ncol}, 1.0, "none")):
                res, st = src.select(op, fill=fill, **kw)
                try:
                    assert st["nnz_out"] == res.nnz
                    assert {"some": 0 < res.nnz < nnz, "all": res.nnz == nnz, "none": res.nnz == 0}[kept]
                    want = 1 + scan + 1 + (kept != "none")
                    assert st["launches"] == want, (nnz, op, fill, st["launches"], want)
                finally:
                    res.close()
        finally:
            src.close()
    ncol, csr = _input("empty_in", np.float32)
    src = am._upload(mctx, ncol, csr)
    try:
        res, st = src.select("ne", 0.0)
        assert st["launches"] == 0 and res.nnz == 0
        res.close()
    finally:
        src.close()
