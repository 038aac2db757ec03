"""osp_csr_mxd on the GPU against tests/mxd_model.py (mxv's model column by column) AND against the device's own osp_csr_mxv of
each column: matrices equal as BITS (compared as unsigned integers); where the value came out of an addition (add = plus) a
NaN is a NaN whatever its payload, as tests/test_gpu_mxv.py compares them.  Input builders are tests/test_gpu_apply_mask.py's."""
import ctypes
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import mxd_model as model
from tests import mxv_model
from tests import test_gpu_apply_mask as am   # the input builders only
from tests import test_gpu_vector as tv       # its cached inputs only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
DTYPES = [np.float32, np.float64]
IDENTITY = {"plus": 0.0, "min": np.inf, "max": -np.inf}
ALL_SEMIRINGS = [(add, mul) for add in model.ADD_OPS for mul in model.MUL_OPS]
LONG_ROW_LAUNCHES = 3 + 1 + 1 + 2   # rows, zeroing, classify; setup; the scan of a few long rows is one kernel; blocks, upper


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _tdt(dt):
    return torch.float32 if dt == np.float32 else torch.float64


def _to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy()).to(DEV)


def _assert_matrix(got, want, add):
    assert got.dtype == want.dtype and got.shape == want.shape
    tv._assert_vector(got.ravel(), want.ravel(), add)


def _mxv_columns(src, X, add, mul):
    """The device's osp_csr_mxv of every column of X, side by side."""
    cols = [src.mxv(np.ascontiguousarray(X[:, c]), add, mul, space="host")[0] for c in range(X.shape[1])]
    return np.stack(cols, axis=1) if cols else np.empty((src.shape[0], 0), X.dtype)


# ---- the shape matrix -------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 128, 129, 2047, 2048, 2, 2049, 2, 2, 4097, 2] + [0] * 100 + [3, 4, 5]


@functools.lru_cache(maxsize=None)
def _shapes(dt):
    """(ncol, csr, X with max(KS) columns): every row length at which the one-lane order changes, a row of 2049 and one of 4097
    between rows of 2, 100 empty rows; M = 124 is no multiple of 64 (nor of 64 / lanes for any packing but one lane)."""
    assert len(LENGTHS) % 64 != 0
    ncol = 1 << 13
    rowptr, col, val = am._csr_from_lengths(LENGTHS, ncol, dt, seed=51)
    X = np.random.default_rng(52).standard_normal((ncol, max(model.KS))).astype(dt)
    for a in (rowptr, col, val, X):
        a.setflags(write=False)
    return ncol, (rowptr, col, val), X


@functools.lru_cache(maxsize=None)
def _shapes_want(dt, add, mul):
    """The model at the widest k, once: a narrower X is its first columns, and a column's result depends on that column alone."""
    ncol, csr, X = _shapes(dt)
    return model.mxd(*csr, X, add, mul)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", model.KS)
def test_every_packing_equals_the_model_and_mxv(mctx, k, dt):
    ncol, csr, Xall = _shapes(dt)
    M, nnz = len(csr[0]) - 1, len(csr[1])
    X = np.ascontiguousarray(Xall[:, :k])
    src = _upload(mctx, ncol, csr)
    try:
        for add, mul in [("plus", "times"), ("min", "plus")]:
            want, nlong = _shapes_want(dt, add, mul)
            assert nlong == 2
            got, st = src.mxd(X, add, mul, space="host")
            _assert_matrix(got, np.ascontiguousarray(want[:, :k]), add)
            _assert_matrix(got, _mxv_columns(src, X, add, mul), add)   # the device's own mxv, column by column
            assert (st["nnz_in"], st["nnz_out"], st["cols"], st["long_segments"]) == (nnz, M * k, k, 2), (add, mul)
            assert st["lanes_per_row"] == model.lanes_per_row(k)
            assert st["launches"] == LONG_ROW_LAUNCHES == model.expected_launches(csr[0], scan_launches=1)
            assert st["ms_total"] >= 0
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_launches_follow_the_formula_without_long_rows(mctx, dt):
    ncol = 1 << 12
    for lengths, launches in (([3, 0, 2000, 45], 1), ([2000, 0, 2000, 7], 3)):
        csr = am._csr_from_lengths(lengths, ncol, dt, seed=53)
        X = np.random.default_rng(54).standard_normal((ncol, 3)).astype(dt)
        src = _upload(mctx, ncol, csr)
        try:
            got, st = src.mxd(X, space="host")
            _assert_matrix(got, model.mxd(*csr, X, "plus", "times")[0], "plus")
            assert st["launches"] == launches == model.expected_launches(csr[0]) and st["long_segments"] == 0
        finally:
            src.close()


# ---- operators and special values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_all_eighteen_semirings_on_special_values(mctx, dt):
    """tests/test_gpu_vector.py's "traps" (special values among the entries, three long rows) times an X of 5 columns that hold
    every special value."""
    ncol, csr = tv._case("traps", dt)
    special = am._special(dt)
    rng = np.random.default_rng(61)
    X = rng.standard_normal((ncol, 5)).astype(dt)
    used = np.unique(csr[1]).astype(np.int64)
    for c in range(5):
        where = rng.choice(used, size=2 * len(special), replace=False)
        X[where, c] = np.resize(special, len(where))
        assert all(np.any(_bits(X[:, c]) == b) for b in _bits(special))
    src = _upload(mctx, ncol, csr)
    dX = _to_dev(X)
    torch.cuda.synchronize(DEV)
    try:
        for add, mul in ALL_SEMIRINGS:
            want, nlong = model.mxd(*csr, X, add, mul)
            got, st = src.mxd(dX, add, mul)
            got = got.cpu().numpy()
            _assert_matrix(got, want, add)
            _assert_matrix(got, _mxv_columns(src, X, add, mul), add)
            assert st["long_segments"] == nlong == 3 and st["launches"] == LONG_ROW_LAUNCHES
            if add != "plus":
                assert not np.isnan(got).any()
        assert np.isnan(model.mxd(*csr, X, "plus", "times")[0]).any()
    finally:
        src.close()


def test_a_product_and_its_addition_are_two_roundings(mctx):
    ncol, csr, x = mxv_model.fma_telling_input()
    X = np.ascontiguousarray(np.stack([x, x[::-1], np.float32(3.0) * x, np.roll(x, 7)], axis=1))
    want, _ = model.mxd(*csr, X, "plus", "times")
    fused = mxv_model.fma_mxv_plus_times(*csr, x)
    src = _upload(mctx, ncol, csr)
    try:
        got, _ = src.mxd(X, space="host")
        assert np.array_equal(_bits(got), _bits(want))
        assert (_bits(np.ascontiguousarray(got[:, 0])) != _bits(fused)).any()
    finally:
        src.close()


# ---- the second upper level ---------------------------------------------------------------------------------------------------------------
def test_a_row_of_more_than_2048_blocks(mctx):
    """One row of 2048 * 2048 + 1 entries (2049 blocks: the row's partials are a long segment themselves), float32, k = 2,
    built on the device and checked against the device's mxv of each column -- whose upper levels are osp_csr_reduce's."""
    n = 2048 * 2048 + 1
    g = torch.Generator(device=DEV).manual_seed(71)
    vals = torch.randn(n, dtype=torch.float32, device=DEV, generator=g)
    X = torch.randn((n, 2), dtype=torch.float32, device=DEV, generator=g)
    rows = torch.zeros(n, dtype=torch.int32, device=DEV)
    cols = torch.arange(n, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize(DEV)
    src, _ = mctx.build(1, n, rows, cols, vals, dup="error", dtype=np.float32, space="device")
    try:
        for add, mul in [("plus", "times"), ("max", "plus")]:
            got, st = src.mxd(X, add, mul)
            assert (st["long_segments"], st["launches"], st["nnz_out"]) == (1, LONG_ROW_LAUNCHES, 2)
            for c in range(2):
                xc = X[:, c].contiguous()
                torch.cuda.synchronize(DEV)
                want, _ = src.mxv(xc, add, mul)
                assert np.array_equal(_bits(got[:, c].cpu().numpy()), _bits(want.cpu().numpy())), (add, mul, c)
        # (not a sum that happens to be exact: the serial sum of the products differs from R's)
        assert float((vals.double() * X[:, 0].double()).sum()) != float(got[0, 0])
    finally:
        src.close()


# ---- calling conventions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_x_and_out_on_the_host_and_on_the_device(mctx, dt):
    ncol, csr, Xall = _shapes(dt)
    M, k = len(csr[0]) - 1, 5
    X = np.ascontiguousarray(Xall[:, :k])
    want = np.ascontiguousarray(_shapes_want(dt, "min", "plus")[0][:, :k])
    src = _upload(mctx, ncol, csr)
    try:
        h, _ = src.mxd(X, "min", "plus", space="host")
        assert isinstance(h, np.ndarray) and h.shape == (M, k) and np.array_equal(_bits(h), _bits(want))
        buf = np.full((M, k), 7.0, dt)
        ret, _ = src.mxd(X.tolist(), "min", "plus", out=buf, space="host")
        assert ret is buf and np.array_equal(_bits(buf), _bits(want))
        dX = _to_dev(X)
        out = torch.full((M, k), 7.0, dtype=_tdt(dt), device=DEV)
        torch.cuda.synchronize(DEV)
        ret, _ = src.mxd(dX, "min", "plus", out=out)
        assert ret is out and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        out.fill_(7.0)
        torch.cuda.synchronize(DEV)
        raw, _ = src.mxd(dX.data_ptr(), "min", "plus", out=out.data_ptr(), k=k)
        assert raw == out.data_ptr() and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        fresh, _ = src.mxd(dX, "min", "plus")
        assert torch.is_tensor(fresh) and tuple(fresh.shape) == (M, k) and np.array_equal(_bits(fresh.cpu().numpy()), _bits(want))
        for call in (lambda: src.mxd(dX, out=torch.zeros((M + 1, k), dtype=_tdt(dt), device=DEV)),
                     lambda: src.mxd(dX, out=torch.zeros((M, k + 1), dtype=_tdt(dt), device=DEV)),
                     lambda: src.mxd(X[:-1], space="host"), lambda: src.mxd(None), lambda: src.mxd(dX.data_ptr())):
            with pytest.raises(S.OspError):
                call()
        with pytest.raises(ValueError):
            src.mxd(dX, add="first")
        with pytest.raises(ValueError):
            src.mxd(dX, mul="div")
    finally:
        src.close()


@pytest.mark.parametrize("space", ["host", "device"])
def test_out_is_x_on_a_square_input(mctx, space):
    n, k = 3000, 6
    rng = np.random.default_rng(17)
    csr = am._csr_from_lengths(rng.integers(0, 40, n), n, np.float64, seed=18, lo=0)
    X = rng.standard_normal((n, k))
    want = model.mxd(*csr, X, "plus", "times")[0]
    src = _upload(mctx, n, csr)
    try:
        if space == "host":
            v = X.copy()
            ret, _ = src.mxd(v, out=v, space="host")
            assert ret is v and np.array_equal(_bits(v), _bits(want))
        else:
            v = _to_dev(X)
            torch.cuda.synchronize(DEV)
            ret, _ = src.mxd(v, out=v)
            assert ret is v and np.array_equal(_bits(v.cpu().numpy()), _bits(want))
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_first_reads_no_x(mctx, dt):
    ncol, csr = tv._case("traps", dt)
    src = _upload(mctx, ncol, csr)
    try:
        for add in model.ADD_OPS:
            column = tv._want_reduce("traps", dt, "rows", add)[0]
            got, st = src.mxd(None, add, "first", space="host", k=3)
            assert st["cols"] == 3
            _assert_matrix(got, np.ascontiguousarray(np.stack([column] * 3, axis=1)), add)
            dev, _ = src.mxd(None, add, "first", k=3)
            assert np.array_equal(_bits(dev.cpu().numpy()), _bits(got))
    finally:
        src.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _semiring(add, mul, reserved=0):
    sr = _lib.Semiring()
    sr.add, sr.mul = add, mul
    sr.reserved[3] = reserved
    return sr


def test_argument_errors_leave_y_and_stats_alone(mctx):
    ncol, csr = tv._case("traps", np.float64)
    M, k = len(csr[0]) - 1, 2
    src = _upload(mctx, ncol, csr)
    L = _lib.lib()
    E = _lib.EWISE_OPS
    x, y = np.ones((ncol, k)), np.full((M, k), 7.0)
    xp, yp = ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data)
    stats = _lib.MxdStats()
    stats.nnz_in = 77
    good = _semiring(E["plus"], E["times"])
    H, st = _lib.OSP_HOST, ctypes.byref(stats)
    calls = [lambda: L.osp_csr_mxd(None, ctypes.byref(good), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, None, xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(good), xp, k, None, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(good), None, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["min"], E["second"])), None, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["first"], E["times"])), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["times"], E["times"])), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["plus"], E["minus"])), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["plus"], E["div"])), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(-1, E["times"])), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["plus"], 99)), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["plus"], E["times"], reserved=1)), xp, k, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(good), xp, k, yp, 99, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(good), xp, model.MAX_COLS + 1, yp, H, st),
             lambda: L.osp_csr_mxd(src._h, ctypes.byref(_semiring(E["max"], E["first"])), None, model.MAX_COLS + 1, yp, H, st)]
    try:
        for i, call in enumerate(calls):
            assert call() == _lib.ERR_ARG, i
            assert L.osp_last_error_string()
            assert stats.nnz_in == 77 and (y == 7.0).all(), i
        # the same call with nothing wrong, and without stats
        assert L.osp_csr_mxd(src._h, ctypes.byref(good), xp, k, yp, H, None) == _lib.OSP_OK
        _assert_matrix(y, model.mxd(*csr, x, "plus", "times")[0], "plus")
    finally:
        src.close()


def test_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    ts = [am._dev(a) for a in (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, B.indptr.astype(np.int64),
                               B.indices.astype(np.uint32), B.data)]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    X, y = np.ones((n, 2)), np.full((n, 2), 5.0)
    E = _lib.EWISE_OPS
    try:
        assert _lib.lib().osp_csr_mxd(part._h, ctypes.byref(_semiring(E["plus"], E["times"])), ctypes.c_void_p(X.ctypes.data), 2,
                                      ctypes.c_void_p(y.ctypes.data), _lib.OSP_HOST, None) == _lib.ERR_ARG
        assert (y == 5.0).all()
    finally:
        part.close()


# ---- empty shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["empty_in", "no_rows"])
def test_empty_inputs_launch_nothing(mctx, case, dt):
    ncol, csr = tv._case(case, dt)
    M, k = len(csr[0]) - 1, 3
    src = _upload(mctx, ncol, csr)
    dX = _to_dev(np.ones((ncol, k), dt))
    torch.cuda.synchronize(DEV)
    try:
        for add in model.ADD_OPS:
            want = np.full((M, k), IDENTITY[add], dt)
            got, st = src.mxd(np.ones((ncol, k), dt), add, "times", space="host")
            assert got.shape == (M, k) and np.array_equal(_bits(got), _bits(want))
            assert (st["launches"], st["nnz_in"], st["nnz_out"], st["cols"], st["long_segments"]) == (0, 0, M * k, k, 0)
            dev, st = src.mxd(dX, add, "second")
            assert st["launches"] == 0 and tuple(dev.shape) == (M, k) and np.array_equal(_bits(dev.cpu().numpy()), _bits(want))
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_no_columns_launch_nothing(mctx, dt):
    ncol, csr, _ = _shapes(dt)
    M = len(csr[0]) - 1
    src = _upload(mctx, ncol, csr)
    try:
        got, st = src.mxd(np.empty((ncol, 0), dt), space="host")
        assert got.shape == (M, 0) and (st["launches"], st["nnz_out"], st["cols"], st["nnz_in"]) == (0, 0, 0, len(csr[1]))
        dev, st = src.mxd(torch.empty((ncol, 0), dtype=_tdt(dt), device=DEV))
        assert tuple(dev.shape) == (M, 0) and st["launches"] == 0
        buf = np.full((M, 0), 7.0, dt)
        assert src.mxd(None, "max", "first", out=buf, space="host", k=0)[0] is buf
    finally:
        src.close()


# ---- chaining and repetition ------------------------------------------------------------------------------------------------------------------
def test_mxd_of_other_operations_results(mctx):
    n, r, c, v = gen.rmat_coo(10, 8, "g500", seed=5)
    A = sp.csr_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    csr = (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(np.float64))
    X = np.random.default_rng(3).standard_normal((n, 7))
    src = _upload(mctx, n, csr)
    made = []
    try:
        made.append(src.transpose()[0])
        made.append(src.select("triu")[0])
        made.append(src.mxm(src, "min", "plus")[0])
        for res in made:
            host = (res.rowptr.copy(), res.colidx.copy(), res.vals.copy())
            for add, mul in [("plus", "times"), ("min", "plus")]:
                got, st = res.mxd(X, add, mul, space="host")
                assert np.array_equal(_bits(got), _bits(model.mxd(*host, X, add, mul)[0])) and st["nnz_in"] == res.nnz
        # the transpose's product is scipy's A^T X up to the order of summation
        assert np.allclose(made[0].mxd(X, space="host")[0], A.T @ X, rtol=1e-12, atol=1e-12)
    finally:
        for res in made:
            res.close()
        src.close()


def test_fifty_back_to_back_calls_give_the_same_bits_and_the_pool_does_not_grow(mctx, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call, and after the first call no call allocates device memory:
    the library's own count of pool misses (hipMalloc calls of the context, printed under OSP_VERBOSE) stays where the first
    call left it."""
    ncol, csr, Xall = _shapes(np.float64)
    k = 17
    src = _upload(mctx, ncol, csr)
    dX = _to_dev(Xall[:, :k])
    out = torch.empty((len(csr[0]) - 1, k), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    monkeypatch.setenv("OSP_VERBOSE", "1")
    misses, first = [], None
    try:
        for i in range(50):
            capfd.readouterr()
            src.mxd(dX, "plus", "times", out=out)
            err = capfd.readouterr().err
            found = re.findall(r"\[osp\] mxd .*pool misses so far: (\d+) hipMalloc calls", err)
            assert len(found) == 1, err
            misses.append(int(found[0]))
            got = _bits(out.cpu().numpy()).copy()
            if first is None:
                first = got
            assert np.array_equal(got, first), i
    finally:
        src.close()
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses
    assert np.array_equal(first, _bits(np.ascontiguousarray(_shapes_want(np.float64, "plus", "times")[0][:, :k])))
