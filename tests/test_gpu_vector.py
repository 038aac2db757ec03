"""osp_csr_reduce, osp_csr_apply_vectors and osp_csr_select_vertices on the GPU against tests/vector_model.py: row pointers and
columns exact, values and vectors equal as BITS (compared as unsigned integers); where a value came out of an arithmetic
operation (PLUS of reduce, the arithmetic ops of apply) a NaN is a NaN whatever its payload, as tests/test_gpu_ewise.py
compares them.  Inputs are tests/test_gpu_apply_mask.py's."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import bfs_model, ewise_model, mxd_model, truss_model
from tests import test_gpu_apply_mask as am   # the input builders only
from tests import vector_model as model

pytestmark = pytest.mark.gpu

DEV = am.DEV
CHUNK = am.CHUNK
_bits = am._bits
_upload = am._upload
DTYPES = [np.float32, np.float64]
CASES = ["traps", "frontier", "short_rows", "empty_in", "no_rows"]


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(name, dt):
    """(ncol, (rowptr, col, val)) of one of the mask filter's inputs, built once and never changed."""
    ncol, csr, _ = am.CASES[name](dt)
    for a in csr:
        a.setflags(write=False)
    return ncol, csr


@functools.lru_cache(maxsize=None)
def _want_reduce(name, dt, axis, op):
    ncol, csr = _case(name, dt)
    return model.reduce(*csr, ncol, axis, op)


def _assert_vector(got, want, op):
    assert got.dtype == want.dtype and got.shape == want.shape
    if op == "plus":
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all() and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))
    else:
        assert np.array_equal(_bits(got), _bits(want))


# ---- reduce ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_reduce_equals_model_bit_for_bit(mctx, case, dt):
    ncol, csr = _case(case, dt)
    M, nnz = len(csr[0]) - 1, len(csr[1])
    src = _upload(mctx, ncol, csr)
    try:
        for axis in model.AXES:
            for op in model.REDUCE_OPS:
                want, nlong = _want_reduce(case, dt, axis, op)
                got, st = src.reduce(axis, op)
                _assert_vector(got, want, op)
                assert (st["nnz_in"], st["nnz_out"], st["long_segments"]) == (nnz, M if axis == "rows" else ncol, nlong), (axis, op)
                assert st["ms_total"] >= 0 and (st["launches"] > 0) == (nnz > 0 and len(want) > 0)
        if case == "traps":
            assert _want_reduce(case, dt, "rows", "plus")[1] == 3          # 2049, 3000 and 4 * 2048
            assert np.isnan(_want_reduce(case, dt, "rows", "plus")[0]).sum() == 2 and not np.isnan(_want_reduce(case, dt, "rows", "min")[0]).any()
        if case == "frontier":
            assert _want_reduce(case, dt, "rows", "plus")[1] == 1 and _want_reduce(case, dt, "cols", "max")[1] == 0
    finally:
        src.close()


def test_reduce_third_level(mctx):
    """ONE float32 row of 2048 * 2048 + 1 entries: the blocks' results are themselves longer than a block."""
    m = model.BLOCK * model.BLOCK + 1
    rng = np.random.default_rng(21)
    val = (rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m)).astype(np.float32)
    csr = (np.array([0, 0, m, m], np.int64), np.arange(m, dtype=np.uint32), val)
    src = _upload(mctx, 1 << 23, csr)
    try:
        for op in ("plus", "min", "max", "count"):
            want, nlong = model.reduce(*csr, 1 << 23, "rows", op)
            got, st = src.reduce("rows", op)
            _assert_vector(got, want, op)
            assert nlong == st["long_segments"] == 1
        assert got.tolist() == [0.0, float(m), 0.0]
    finally:
        src.close()


# row lengths around the block of 2048: nothing can be long, nnz > 2048 without a long row, one long row of two blocks
LAUNCH_SHAPES = [[3, 0, 2000, 45], [2000, 0, 2000, 7], [2, 2049, 2]]


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_launches_follow_the_formula(mctx, dt):
    """stats.launches of plus, min and max is osp_csr_mxd's count (tests/mxd_model.py) on the segments of the axis: the short
    kernel; the zeroing and the listing of the long segments; with a long one the setup, the scan (one launch for one entry),
    the blocks and the next level's short kernel."""
    ncol = 1 << 12
    for lengths, launches in zip(LAUNCH_SHAPES, (1, 3, 7)):
        csr = am._csr_from_lengths(lengths, ncol, dt, seed=23)
        assert mxd_model.expected_launches(csr[0], scan_launches=1) == launches
        by_axis = {"rows": launches, "cols": mxd_model.expected_launches(model.column_view(*csr, ncol)[0], scan_launches=1)}
        src = _upload(mctx, ncol, csr)
        try:
            for axis in model.AXES:
                for op in ("plus", "min", "max"):
                    got, st = src.reduce(axis, op)
                    _assert_vector(got, model.reduce(*csr, ncol, axis, op)[0], op)
                    assert st["launches"] == by_axis[axis], (lengths, axis, op)
        finally:
            src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_columns_of_the_transpose_is_reduce_rows(mctx, dt):
    ncol, csr = _case("traps", dt)
    M = len(csr[0]) - 1
    T = sp.csr_matrix((csr[2], csr[1].astype(np.int64), csr[0]), shape=(M, ncol)).T.tocsr()
    T.sort_indices()
    tcsr = (T.indptr.astype(np.int64), T.indices.astype(np.uint32), T.data)
    view = model.column_view(*csr, ncol)
    assert np.array_equal(tcsr[0], view[0]) and np.array_equal(tcsr[1], view[1]) and np.array_equal(_bits(tcsr[2]), _bits(view[2]))
    src, tr = _upload(mctx, ncol, csr), _upload(mctx, M, tcsr)
    try:
        for op in model.REDUCE_OPS:
            a, sa = src.reduce("rows", op)
            b, sb = tr.reduce("cols", op)
            assert np.array_equal(_bits(a), _bits(b)), op      # (the same segments in the same order: NaN payloads included)
            assert sa["long_segments"] == sb["long_segments"]
            c, _ = tr.reduce("rows", op)
            d, _ = src.reduce("cols", op)
            assert np.array_equal(_bits(c), _bits(d)), op
    finally:
        src.close()
        tr.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_into_device_memory(mctx, dt):
    ncol, csr = _case("traps", dt)
    M = len(csr[0]) - 1
    tdt = torch.float32 if dt == np.float32 else torch.float64
    src = _upload(mctx, ncol, csr)
    try:
        for axis, n in (("rows", M), ("cols", ncol)):
            for op in model.REDUCE_OPS:
                out = torch.full((n,), 7.0, dtype=tdt, device=DEV)
                torch.cuda.synchronize(DEV)
                ret, st = src.reduce(axis, op, out=out)
                assert ret is out
                _assert_vector(out.cpu().numpy(), _want_reduce("traps", dt, axis, op)[0], op)
                raw, _ = src.reduce(axis, op, out=out.data_ptr())
                assert raw == out.data_ptr()
        with pytest.raises(S.OspError):
            src.reduce("rows", "plus", out=torch.zeros(M + 1, dtype=tdt, device=DEV))
        with pytest.raises(ValueError):
            src.reduce("diagonal", "plus")
        with pytest.raises(ValueError):
            src.reduce("rows", "times")
    finally:
        src.close()


# ---- apply ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vectors(name, dt):
    """x (M values) and y (ncol values): random numbers, with every value of am._special on rows and columns that hold
    entries (as far as there are that many)."""
    ncol, (rowptr, col, _) = _case(name, dt)
    rng = np.random.default_rng(31)
    M = len(rowptr) - 1
    x, y = rng.standard_normal(M).astype(dt), rng.standard_normal(ncol).astype(dt)
    sp_ = am._special(dt)
    rows = np.flatnonzero(np.diff(rowptr) > 0)
    rows = rows[:: max(1, len(rows) // (3 * len(sp_)))]
    x[rows] = np.resize(sp_, len(rows))
    cols = np.unique(col)
    cols = cols[rng.random(len(cols)) < 0.3]
    y[cols] = np.resize(sp_, len(cols))
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


PAIRS = [("second", "plus"), ("times", "times"), ("div", None), (None, "min")]
SIDES = [(op, None) for op in model.APPLY_OPS] + [(None, op) for op in model.APPLY_OPS]


def _assert_values(got, want, computed):
    gb, wb = _bits(got), _bits(want)
    if not computed:
        assert np.array_equal(gb, wb)
        return
    nan = np.isnan(want)
    assert np.array_equal(gb[~nan], wb[~nan]) and np.isnan(got[nan]).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["traps", "frontier", "short_rows"])
def test_apply_vectors_equals_model(mctx, case, dt):
    ncol, csr = _case(case, dt)
    x, y = _vectors(case, dt)
    if case == "traps":
        for v in (x, y):
            assert all(np.any(_bits(v) == b) for b in _bits(am._special(dt)))
    src = _upload(mctx, ncol, csr)
    dx, dy = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)   # (copies of the bytes: payloads survive)
    torch.cuda.synchronize(DEV)
    try:
        for i, (row_op, col_op) in enumerate(SIDES + PAIRS):
            want, computed = model.apply_vectors(*csr, x, row_op, y, col_op)
            if i % 2:
                res, st = src.apply_vectors(x, row_op, y, col_op, space="host")
            else:
                res, st = src.apply_vectors(dx.data_ptr(), row_op, dy.data_ptr(), col_op)
            try:
                assert res.shape == src.shape and res.dtype == dt and res.nnz == len(csr[1]) == res.info["nnz_c"]
                assert np.array_equal(res.rowptr, csr[0]) and np.array_equal(res.colidx, csr[1])
                _assert_values(res.vals, want, computed)
                assert (st["nnz_in"], st["nnz_out"], st["long_segments"]) == (len(csr[1]), len(csr[1]), 0)
                assert st["launches"] == (row_op is not None) + (col_op is not None)
            finally:
                res.close()
    finally:
        src.close()


def test_apply_vectors_ignores_the_vector_of_a_skipped_side_and_the_value_under_second(mctx):
    ncol, csr = _case("traps", np.float64)
    x, y = _vectors("traps", np.float64)
    src = _upload(mctx, ncol, csr)
    try:
        a, _ = src.apply_vectors(x, "plus", None, None, space="host")
        b, _ = src.apply_vectors(x, "plus", "not a vector", None, space="host")
        assert np.array_equal(_bits(a.vals), _bits(b.vals))
        # SECOND first: the result does not depend on in's values (the row of special values included)
        ones, _ = src.select("ne", np.nan, fill=1.0)
        c, _ = src.apply_vectors(x, "second", y, "plus", space="host")
        d, _ = ones.apply_vectors(x, "second", y, "plus", space="host")
        assert np.array_equal(_bits(c.vals), _bits(d.vals))
        for r in (a, b, c, d, ones):
            r.close()
        for bad in ("first", "pow"):
            with pytest.raises(ValueError):
                src.apply_vectors(x, bad, space="host")
        with pytest.raises(S.OspError):
            src.apply_vectors(x[:-1], "plus", space="host")
        with pytest.raises(ValueError):
            src.apply_vectors(x, "plus", space="elsewhere")
    finally:
        src.close()


def test_apply_vectors_of_empty_results(mctx):
    for case in ("empty_in", "no_rows"):
        ncol, csr = _case(case, np.float64)
        M = len(csr[0]) - 1
        src = _upload(mctx, ncol, csr)
        try:
            res, st = src.apply_vectors(np.ones(M), "times", np.ones(ncol), "plus", space="host")
            assert res.nnz == 0 and res.shape == (M, ncol) and np.array_equal(res.rowptr, csr[0]) and st["launches"] == 0
            res.close()
        finally:
            src.close()


# ---- vertex select --------------------------------------------------------------------------------------------------------
def _keeps(name, n, rowptr=None):
    rng = np.random.default_rng(41 + n % 7)
    out = {"ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "half": (rng.random(n) < 0.5).astype(np.uint8) * 3}
    if rowptr is not None:
        # the rows that begin on a chunk boundary or hold one
        some = np.diff(rowptr) > 0
        edge = some & ((rowptr[:-1] % CHUNK == 0) | (rowptr[:-1] // CHUNK < (rowptr[1:] - 1) // CHUNK))
        assert edge.sum() >= 3
        out["boundary"] = edge.astype(np.uint8)
    return out


def _check_select(res, st, csr, want):
    assert np.array_equal(res.rowptr, want[0]) and np.array_equal(res.colidx, want[1]) and np.array_equal(_bits(res.vals), _bits(want[2]))
    assert res.nnz == len(want[1]) == res.info["nnz_c"]
    assert (st["nnz_in"], st["nnz_out"], st["long_segments"]) == (len(csr[1]), len(want[1]), 0)
    assert (st["launches"] > 0) == (len(csr[1]) > 0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_select_vertices_equals_model(mctx, case, dt):
    ncol, csr = _case(case, dt)
    M = len(csr[0]) - 1
    kr, kc = _keeps(case, M, csr[0] if case == "traps" else None), _keeps(case, ncol)
    src = _upload(mctx, ncol, csr)
    try:
        for i, (rname, cname) in enumerate([(r, None) for r in kr] + [(None, c) for c in kc] + [("half", "half"), ("ones", "half"), ("half", "zeros")]
                                           + ([("boundary", "half")] if "boundary" in kr else [])):
            r, c = kr.get(rname), kc.get(cname)
            want = model.select_vertices(*csr, r, c)
            if i % 2:
                res, st = src.select_vertices(r, c, space="host")
            else:
                dr, dc = (None if v is None else torch.from_numpy(v).to(DEV) for v in (r, c))
                torch.cuda.synchronize(DEV)
                res, st = src.select_vertices(dr, dc)
            try:
                _check_select(res, st, csr, want)
                if rname == "ones" and cname is None or cname == "ones" and rname is None:
                    assert res.nnz == src.nnz
                if "zeros" in (rname, cname):
                    assert res.nnz == 0
            finally:
                res.close()
    finally:
        src.close()


@pytest.mark.parametrize("case", ["traps", "short_rows"])
def test_select_rows_then_columns_is_both_at_once(mctx, case):
    ncol, csr = _case(case, np.float64)
    M = len(csr[0]) - 1
    r, c = _keeps(case, M)["half"], _keeps(case, ncol)["half"]
    src = _upload(mctx, ncol, csr)
    try:
        a, _ = src.select_vertices(r, None, space="host")
        ab, _ = a.select_vertices(None, c, space="host")
        b, _ = src.select_vertices(None, c, space="host")
        ba, _ = b.select_vertices(r, None, space="host")
        both, st = src.select_vertices(r, c, space="host")
        for x in (ab, ba):
            assert np.array_equal(x.rowptr, both.rowptr) and np.array_equal(x.colidx, both.colidx) and np.array_equal(_bits(x.vals), _bits(both.vals))
        assert 0 < both.nnz < a.nnz < src.nnz and st["nnz_out"] == len(model.select_vertices(*csr, r, c)[1])
        for x in (a, ab, b, ba, both):
            x.close()
    finally:
        src.close()


# ---- error paths ------------------------------------------------------------------------------------------------------------
def _apply(row_op, col_op, reserved=0):
    ap = _lib.VectorApply()
    ap.row_op = _lib.VECTOR_NONE if row_op is None else row_op
    ap.col_op = _lib.VECTOR_NONE if col_op is None else col_op
    ap.reserved[5] = reserved
    return ap


def test_argument_errors(mctx):
    L = _lib.lib()
    res = am._small_result(mctx)   # 2 x 4, float64
    out = ctypes.c_void_p(0x1234)
    stats = _lib.VectorStats()
    stats.nnz_in = 77
    vec, keep = np.full(4, 5.0), np.ones(4, np.uint8)
    vp, kp, H = ctypes.c_void_p(vec.ctypes.data), ctypes.c_void_p(keep.ctypes.data), _lib.OSP_HOST
    o, s = ctypes.byref(out), ctypes.byref(stats)
    plus, first = _lib.EWISE_OPS["plus"], _lib.EWISE_OPS["first"]
    bad = [lambda: L.osp_csr_reduce(res._h, 0, 0, None, H, s),                              # null output vector
           lambda: L.osp_csr_reduce(res._h, 2, 0, vp, H, s), lambda: L.osp_csr_reduce(res._h, -1, 0, vp, H, s),      # bad axis
           lambda: L.osp_csr_reduce(res._h, 0, 4, vp, H, s), lambda: L.osp_csr_reduce(res._h, 1, -1, vp, H, s),      # bad op
           lambda: L.osp_csr_reduce(res._h, 0, 0, vp, 7, s),                                # bad space
           lambda: L.osp_csr_apply_vectors(res._h, None, vp, vp, H, o, s),                  # null ap
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(plus, None)), vp, vp, H, None, s),              # null out
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(first, None)), vp, vp, H, o, s),                # FIRST
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(None, first)), vp, vp, H, o, s),
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(None, None)), vp, vp, H, o, s),                 # both NONE
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(plus, None)), None, vp, H, o, s),               # an op without its vector
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(None, plus)), vp, None, H, o, s),
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(8, None)), vp, vp, H, o, s),                    # bad op
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(plus, -2)), vp, vp, H, o, s),
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(plus, None, reserved=1)), vp, vp, H, o, s),     # reserved word
           lambda: L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(plus, None)), vp, vp, 7, o, s),                 # bad space
           lambda: L.osp_csr_select_vertices(res._h, None, None, H, o, s),                  # both null
           lambda: L.osp_csr_select_vertices(res._h, kp, kp, H, None, s),                   # null out
           lambda: L.osp_csr_select_vertices(res._h, kp, kp, 7, o, s)]                      # bad space
    try:
        for i, call in enumerate(bad):
            assert call() == _lib.ERR_ARG, i
            assert L.osp_last_error_string()
            assert out.value == 0x1234 and stats.nnz_in == 77 and np.all(vec == 5.0), i
        # a skipped side's null vector and null stats are legal
        o2 = ctypes.c_void_p()
        assert L.osp_csr_apply_vectors(res._h, ctypes.byref(_apply(None, plus)), None, vp, H, ctypes.byref(o2), None) == 0
        r2 = S.CsrResult(mctx, o2)
        assert r2.vals.tolist() == [6.0, 7.0, 8.0]
        r2.close()
        assert L.osp_csr_reduce(res._h, 0, 0, vp, H, None) == 0 and vec.tolist() == [3.0, 3.0, 5.0, 5.0]
        o3 = ctypes.c_void_p()
        assert L.osp_csr_select_vertices(res._h, None, kp, H, ctypes.byref(o3), None) == 0
        r3 = S.CsrResult(mctx, o3)
        assert r3.nnz == 3
        r3.close()
        with pytest.raises(S.OspError):
            res.select_vertices(np.ones(3, np.uint8), None, space="host")
        with pytest.raises(ValueError):
            res.select_vertices(keep[:2], None, space="elsewhere")
    finally:
        res.close()


def test_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    ts = [am._dev(x) for x in (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, B.indptr.astype(np.int64),
                               B.indices.astype(np.uint32), B.data)]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    L = _lib.lib()
    out = ctypes.c_void_p(0x1234)
    vec, keep = np.full(n, 5.0), np.ones(n, np.uint8)
    vp, kp = ctypes.c_void_p(vec.ctypes.data), ctypes.c_void_p(keep.ctypes.data)
    try:
        assert L.osp_csr_reduce(part._h, 0, 0, vp, _lib.OSP_HOST, None) == _lib.ERR_ARG
        assert L.osp_csr_apply_vectors(part._h, ctypes.byref(_apply(0, None)), vp, vp, _lib.OSP_HOST, ctypes.byref(out), None) == _lib.ERR_ARG
        assert L.osp_csr_select_vertices(part._h, kp, kp, _lib.OSP_HOST, ctypes.byref(out), None) == _lib.ERR_ARG
        assert out.value == 0x1234 and np.all(vec == 5.0)
    finally:
        part.close()


# ---- composition --------------------------------------------------------------------------------------------------------------
def _host(res):
    return res.rowptr.copy(), res.colidx.copy(), res.vals.copy()


def _same(res, want):
    return np.array_equal(res.rowptr, want[0]) and np.array_equal(res.colidx, want[1]) and np.array_equal(_bits(res.vals), _bits(want[2]))


def test_vector_results_compose(mctx):
    from outerspace_amd.sparse_util import _result_as_input
    n = 3000
    a = am._csr_from_lengths([5, 0, 700, 2500, 64] + [0] * (n - 5), n, np.float64, seed=41)
    rng = np.random.default_rng(42)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    keep[:5] = 1
    ra = _upload(mctx, n, a)
    made = []
    try:
        ap, _ = ra.apply_vectors(x, "times", y, "plus", space="host")
        made.append(ap)
        wap = (a[0], a[1], model.apply_vectors(*a, x, "times", y, "plus")[0])
        assert _same(ap, wap)
        sv, _ = ap.select_vertices(None, keep, space="host")
        made.append(sv)
        wsv = model.select_vertices(*wap, None, keep)
        assert _same(sv, wsv) and 0 < sv.nnz < ap.nnz
        # into select, ewise and apply_mask
        s, _ = sv.select("gt", 0.0)
        made.append(s)
        assert _same(s, truss_model.select(*wsv, "gt", 0.0))
        e, _ = ap.ewise(sv, "intersect", "minus")
        made.append(e)
        assert _same(e, ewise_model.ewise(wap, wsv, n, "intersect", "minus"))
        m, _ = ap.apply_mask(sv, complement=True)
        made.append(m)
        assert _same(m, bfs_model.apply_mask(*wap, wsv[0], wsv[1], n, True)) and m.nnz == ap.nnz - sv.nnz
        # a reduce of each
        for res, w in ((ap, wap), (sv, wsv)):
            for axis in model.AXES:
                got, _ = res.reduce(axis, "plus")
                _assert_vector(got, model.reduce(*w, n, axis, "plus")[0], "plus")
        # into a product: sv @ sv by the COO entry point, against scipy
        t = _result_as_input(sv, torch.device(DEV))
        ptrs = (t.rows.data_ptr(), t.cols.data_ptr(), t.vals.data_ptr())
        p = mctx.spgemm_coo_device(np.float64, n, n, n, t.nnz, ptrs, t.nnz, ptrs)
        made.append(p)
        W = sp.csr_matrix((wsv[2], wsv[1].astype(np.int64), wsv[0]), shape=(n, n))
        ref = (W @ W).tocsr()
        ref.sort_indices()
        assert np.array_equal(p.rowptr, ref.indptr) and np.array_equal(p.colidx, ref.indices) and np.allclose(p.vals, ref.data, rtol=1e-12, atol=1e-12)
        torch.cuda.synchronize(DEV)
        del t
        # info is in's with nnz_c and ms_total replaced
        for k, v in ra.info.items():
            if k not in ("nnz_c", "ms_total"):
                assert ap.info[k] == v and sv.info[k] == v, k
    finally:
        for r in made + [ra]:
            r.close()


def test_fifty_back_to_back_calls_give_the_same_arrays(mctx):
    """Recycled pool buffers carry nothing over from call to call."""
    ncol, csr = _case("traps", np.float32)
    x, y = _vectors("traps", np.float32)
    M = len(csr[0]) - 1
    kr, kc = _keeps("traps", M, csr[0])["boundary"], _keeps("traps", ncol)["half"]
    src = _upload(mctx, ncol, csr)
    try:
        first = {}
        for i in range(50):
            kind = i % 5
            if kind == 0:
                got = (_bits(src.reduce("rows", "plus")[0]).copy(),)
            elif kind == 1:
                got = (_bits(src.reduce("cols", "min")[0]).copy(),)
            elif kind == 2:
                got = (_bits(src.reduce("cols", "plus")[0]).copy(),)
            elif kind == 3:
                res, _ = src.apply_vectors(x, "div", y, "max", space="host")
                got = (_bits(res.vals).copy(),)
                res.close()
            else:
                res, st = src.select_vertices(kr, kc, space="host")
                got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["nnz_out"])
                res.close()
            if kind not in first:
                first[kind] = got
            else:
                assert all(np.array_equal(a, b) for a, b in zip(got, first[kind])), i
    finally:
        src.close()
