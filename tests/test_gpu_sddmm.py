"""osp_csr_sddmm on the GPU against tests/sddmm_model.py (vector_model's R on the k products of every entry) AND against the
device's own osp_csr_mxv of the one-row CSR of X[i, :] with Y[j, :]: values equal as BITS (compared as unsigned integers);
where a value came out of an arithmetic operation a NaN is a NaN whatever its payload, as tests/test_gpu_mxv.py compares
them.  Input builders are tests/test_gpu_apply_mask.py's."""
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
from tests import mxd_model
from tests import sddmm_model as model
from tests import test_gpu_apply_mask as am   # the input builders only
from tests import test_gpu_vector as tv       # its cached inputs only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
DTYPES = [np.float32, np.float64]
ALL_SEMIRINGS = [(add, mul) for add in model.ADD_OPS for mul in model.MUL_OPS]


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _assert_values(got, want, computed):
    assert got.dtype == want.dtype and got.shape == want.shape
    if computed:
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all() and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))
    else:
        assert np.array_equal(_bits(got), _bits(want))


def _sddmm(src, X, Y, add="plus", mul="times", accum="second", **kw):
    """The call, the result's values on the host, its pattern checked against the input's; the result is closed."""
    res, st = src.sddmm(X, Y, add, mul, accum, **kw)
    try:
        assert res.shape == src.shape and res.nnz == src.nnz == st["nnz_in"] == st["nnz_out"] and res.dtype == src.dtype
        assert np.array_equal(res.rowptr, src.rowptr) and np.array_equal(res.colidx, src.colidx)
        return res.vals.copy(), st
    finally:
        res.close()


# ---- the main pattern: every packing ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _main(dt):
    ncol, csr = model.main_pattern(dt)
    rng = np.random.default_rng(92)
    X = rng.standard_normal((len(csr[0]) - 1, max(model.KS))).astype(dt)
    Y = rng.standard_normal((ncol, max(model.KS))).astype(dt)
    for a in (*csr, X, Y):
        a.setflags(write=False)
    return ncol, csr, X, Y


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", model.KS)
def test_every_packing_equals_the_model(mctx, k, dt):
    ncol, csr, Xall, Yall = _main(dt)
    assert (len(csr[0]) - 1, ncol) == (70, 4200) and np.diff(csr[0]).max() == 4097
    X, Y = np.ascontiguousarray(Xall[:, :k]), np.ascontiguousarray(Yall[:, :k])
    src = _upload(mctx, ncol, csr)
    try:
        for add, mul, accum in [("plus", "times", "second"), ("min", "plus", "second"), ("plus", "times", "minus")]:
            want, computed = model.sddmm(*csr, X, Y, add, mul, accum)
            got, st = _sddmm(src, X, Y, add, mul, accum, space="host")
            _assert_values(got, want, computed)
            assert (st["nnz_out"], st["cols"], st["lanes_per_entry"]) == (len(csr[1]), k, model.lanes_per_entry(k))
            assert st["launches"] == model.expected_launches(len(csr[1])) == 1 and st["ms_total"] >= 0
        if k == 0:   # d is the identity
            assert np.array_equal(_bits(_sddmm(src, X, Y, "max", "times", space="host")[0]), _bits(np.full(len(csr[1]), -np.inf, dt)))
    finally:
        src.close()


# ---- large k: the blocks of 2048 and the second level ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", [2047, 2048, 2049, 4097])
def test_k_around_the_block_of_2048(mctx, k, dt):
    rng = np.random.default_rng(93)
    csr = am._csr_from_lengths([3, 0, 5, 4], 9, dt, seed=94, lo=0)
    assert len(csr[1]) == 12
    X, Y = rng.standard_normal((4, k)).astype(dt), rng.standard_normal((9, k)).astype(dt)
    src = _upload(mctx, 9, csr)
    try:
        for add, mul in [("plus", "times"), ("max", "plus")]:
            got, st = _sddmm(src, X, Y, add, mul, space="host")
            _assert_values(got, model.sddmm(*csr, X, Y, add, mul)[0], add == "plus")
            assert st["lanes_per_entry"] == 64 and st["launches"] == 1
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_largest_k_takes_the_second_level_with_32_blocks(mctx, dt):
    k = model.MAX_COLS
    rng = np.random.default_rng(95)
    csr = (np.array([0, 1, 1, 3, 3], np.int64), np.array([4, 0, 2], np.uint32), rng.standard_normal(3).astype(dt))
    X, Y = rng.standard_normal((4, k)).astype(dt), rng.standard_normal((5, k)).astype(dt)
    src = _upload(mctx, 5, csr)
    try:
        for add, mul, accum in [("plus", "times", "second"), ("min", "plus", "plus")]:
            want, computed = model.sddmm(*csr, X, Y, add, mul, accum)
            _assert_values(_sddmm(src, X, Y, add, mul, accum, space="host")[0], want, computed)
        # (not a sum that happens to be exact: the serial sum of the products differs from R's somewhere)
        serial = np.array([np.cumsum((X[i] * Y[j]).astype(dt), dtype=dt)[-1] for i, j in ((0, 4), (2, 0), (2, 2))], dt)
        assert (_bits(serial) != _bits(model.sddmm(*csr, X, Y)[0])).any()
    finally:
        src.close()


# ---- the independent device path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", [5, 100, 2100])
def test_a_dozen_entries_equal_the_devices_own_mxv_of_the_one_row_csr(mctx, k, dt):
    ncol, csr, _, _ = _main(dt)
    rng = np.random.default_rng(96)
    X, Y = rng.standard_normal((70, k)).astype(dt), rng.standard_normal((ncol, k)).astype(dt)
    rows = np.repeat(np.arange(70), np.diff(csr[0]))
    entries = np.concatenate([[0, 1, 2, len(csr[1]) - 1], rng.choice(len(csr[1]), size=8, replace=False)])
    src = _upload(mctx, ncol, csr)
    try:
        for add, mul in [("plus", "times"), ("min", "plus"), ("max", "second")]:
            got, _ = _sddmm(src, X, Y, add, mul, space="host")
            for p in entries:
                one, _ = mctx.build(1, k, np.zeros(k, np.int64), np.arange(k), X[rows[p]], dup="error", dtype=dt, space="host")
                try:
                    want, _ = one.mxv(np.ascontiguousarray(Y[int(csr[1][p])]), add, mul, space="host")
                finally:
                    one.close()
                _assert_values(got[p:p + 1], want, add == "plus")
    finally:
        src.close()


# ---- operators and special values ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _special_case(dt):
    """A 40 x 50 pattern of every row length from 0 to 12 whose X and Y hold every special value (NaNs with payloads, both
    infinities, both zeros, denormals) in every column of k = 5, and whose own values hold them too."""
    rng = np.random.default_rng(97)
    M, N, k = 40, 50, 5
    csr = am._csr_from_lengths(rng.integers(0, 13, M), N, dt, seed=98, lo=0)
    special = am._special(dt)
    X, Y = rng.standard_normal((M, k)).astype(dt), rng.standard_normal((N, k)).astype(dt)
    for c in range(k):
        X[rng.choice(M, size=len(special), replace=False), c] = special
        Y[rng.choice(N, size=len(special), replace=False), c] = special
    val = csr[2].copy()
    val[rng.choice(len(val), size=len(special), replace=False)] = special
    return M, N, (csr[0], csr[1], val), X, Y


@pytest.mark.parametrize("dt", DTYPES)
def test_all_eighteen_semirings_and_three_accums_on_special_values(mctx, dt):
    M, N, csr, X, Y = _special_case(dt)
    src = _upload(mctx, N, csr)
    dX, dY = _to_dev(X), _to_dev(Y)
    torch.cuda.synchronize(DEV)
    seen_nan = False
    try:
        for add, mul in ALL_SEMIRINGS:
            for accum in ("second", "times", "minus"):
                want, computed = model.sddmm(*csr, X, Y, add, mul, accum)
                got, st = _sddmm(src, dX, dY, add, mul, accum)
                _assert_values(got, want, computed)
                assert st["launches"] == 1 and st["cols"] == 5 and st["lanes_per_entry"] == 8
                seen_nan |= bool(np.isnan(want).any())
                if add != "plus" and accum == "second":
                    assert not np.isnan(got).any()
        assert seen_nan
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_every_accum_operator_under_plus_times(mctx, dt):
    M, N, csr, X, Y = _special_case(dt)
    src = _upload(mctx, N, csr)
    try:
        for accum in model.ACCUM_OPS + [None]:
            want, computed = model.sddmm(*csr, X, Y, "plus", "times", accum)
            _assert_values(_sddmm(src, X, Y, accum=accum, space="host")[0], want, True)
        with pytest.raises(ValueError):
            src.sddmm(X, Y, accum="first", space="host")
        # second and None read no value of `in`: the same bits on a pattern whose values are all NaN
        nan = _upload(mctx, N, (csr[0], csr[1], np.full(len(csr[1]), np.nan, dt)))
        try:
            for accum in ("second", None):
                _assert_values(_sddmm(nan, X, Y, accum=accum, space="host")[0], model.sddmm(*csr, X, Y)[0], True)
        finally:
            nan.close()
    finally:
        src.close()


def test_a_product_and_its_addition_are_two_roundings(mctx):
    X, Y = model.fma_telling_dense()
    n = len(X)
    csr = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.uint32), np.ones(n, np.float32))
    src = _upload(mctx, n, csr)
    try:
        got, _ = _sddmm(src, X, Y, space="host")
        assert np.array_equal(_bits(got), _bits(model.sddmm(*csr, X, Y)[0]))
        assert (_bits(got) != _bits(model.fma_diagonal(X, Y))).any()
    finally:
        src.close()


# ---- calling conventions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_x_and_y_on_the_host_and_on_the_device(mctx, dt):
    ncol, csr, Xall, Yall = _main(dt)
    k = 17
    X, Y = np.ascontiguousarray(Xall[:, :k]), np.ascontiguousarray(Yall[:, :k])
    want = model.sddmm(*csr, X, Y, "min", "plus", "max")[0]
    src = _upload(mctx, ncol, csr)
    try:
        assert np.array_equal(_bits(_sddmm(src, X, Y, "min", "plus", "max", space="host")[0]), _bits(want))
        assert np.array_equal(_bits(_sddmm(src, X.tolist(), Y.tolist(), "min", "plus", "max", space="host")[0]), _bits(want))
        dX, dY = _to_dev(X), _to_dev(Y)
        torch.cuda.synchronize(DEV)
        assert np.array_equal(_bits(_sddmm(src, dX, dY, "min", "plus", "max")[0]), _bits(want))
        assert np.array_equal(_bits(_sddmm(src, dX.data_ptr(), dY.data_ptr(), "min", "plus", "max", k=k)[0]), _bits(want))
        for call in (lambda: src.sddmm(dX[:-1].contiguous(), dY), lambda: src.sddmm(dX, dY[:, :-1].contiguous()), lambda: src.sddmm(None, dY),
                     lambda: src.sddmm(dX, None), lambda: src.sddmm(dX.data_ptr(), dY.data_ptr()), lambda: src.sddmm(X[:-1], Y, space="host")):
            with pytest.raises(S.OspError):
                call()
        with pytest.raises(ValueError):
            src.sddmm(dX, dY, add="first")
        with pytest.raises(ValueError):
            src.sddmm(dX, dY, mul="div")
    finally:
        src.close()


@pytest.mark.parametrize("space", ["host", "device"])
def test_y_is_x_on_a_square_pattern(mctx, space):
    n, k = 300, 6
    rng = np.random.default_rng(17)
    csr = am._csr_from_lengths(rng.integers(0, 40, n), n, np.float64, seed=18, lo=0)
    X = rng.standard_normal((n, k))
    want = model.sddmm(*csr, X, X, accum="plus")[0]
    src = _upload(mctx, n, csr)
    try:
        v = X if space == "host" else _to_dev(X)
        torch.cuda.synchronize(DEV)
        got, _ = _sddmm(src, v, v, accum="plus", space=space)
        assert np.array_equal(_bits(got), _bits(want))
        if space == "device":   # the same address twice, given as addresses
            assert np.array_equal(_bits(_sddmm(src, v.data_ptr(), v.data_ptr(), accum="plus", k=k)[0]), _bits(want))
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_first_reads_no_y_and_second_no_x(mctx, dt):
    M, N, csr, X, Y = _special_case(dt)
    src = _upload(mctx, N, csr)
    dX, dY = _to_dev(X), _to_dev(Y)
    torch.cuda.synchronize(DEV)
    try:
        for add in model.ADD_OPS:
            for args, mul in (((X, None), "first"), ((None, Y), "second")):
                want, computed = model.sddmm(*csr, *args, add, mul)
                got, st = _sddmm(src, *args, add, mul, space="host")
                _assert_values(got, want, computed)
                assert st["cols"] == 5
                dargs = tuple(None if a is None else d for a, d in zip(args, (dX, dY)))
                _assert_values(_sddmm(src, *dargs, add, mul)[0], want, computed)
                # an operand that is given but not read is not looked at either
                other = (X, np.zeros((1, 1))) if mul == "first" else (np.zeros((1, 1)), Y)
                _assert_values(_sddmm(src, *other, add, mul, space="host")[0], want, computed)
    finally:
        src.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _semiring(add, mul, reserved=0):
    sr = _lib.Semiring()
    sr.add, sr.mul = add, mul
    sr.reserved[3] = reserved
    return sr


def test_argument_errors_leave_out_and_stats_alone(mctx):
    M, N, csr, X, Y = _special_case(np.float64)
    k = 5
    src = _upload(mctx, N, csr)
    L = _lib.lib()
    E = _lib.EWISE_OPS
    xp, yp = ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(Y.ctypes.data)
    stats = _lib.SddmmStats()
    stats.nnz_in = 77
    out = ctypes.c_void_p(0x5555)
    good = _semiring(E["plus"], E["times"])
    H, st, op, SEC = _lib.OSP_HOST, ctypes.byref(stats), ctypes.byref(out), E["second"]
    g = ctypes.byref(good)
    calls = [lambda: L.osp_csr_sddmm(None, g, SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, None, SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, SEC, xp, yp, k, H, None, st),
             lambda: L.osp_csr_sddmm(src._h, g, SEC, None, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, SEC, xp, None, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["min"], E["first"])), SEC, None, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["min"], E["second"])), SEC, xp, None, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["first"], E["times"])), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["times"], E["times"])), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["plus"], E["minus"])), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["plus"], E["div"])), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(-1, E["times"])), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["plus"], 99)), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, ctypes.byref(_semiring(E["plus"], E["times"], reserved=1)), SEC, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, E["first"], xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, 8, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, -2, xp, yp, k, H, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, SEC, xp, yp, k, 99, op, st),
             lambda: L.osp_csr_sddmm(src._h, g, SEC, xp, yp, model.MAX_COLS + 1, H, op, st)]
    try:
        for i, call in enumerate(calls):
            assert call() == _lib.ERR_ARG, i
            assert L.osp_last_error_string()
            assert stats.nnz_in == 77 and out.value == 0x5555, i
        # the same call with nothing wrong, and without stats; OSP_VECTOR_NONE is SECOND
        assert L.osp_csr_sddmm(src._h, g, _lib.VECTOR_NONE, xp, yp, k, H, op, None) == _lib.OSP_OK
        res = S.CsrResult(mctx, out)
        try:
            _assert_values(res.vals, model.sddmm(*csr, X, Y)[0], True)
        finally:
            res.close()
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
    X = np.ones((n, 2))
    E = _lib.EWISE_OPS
    out = ctypes.c_void_p(0x5555)
    try:
        assert _lib.lib().osp_csr_sddmm(part._h, ctypes.byref(_semiring(E["plus"], E["times"])), E["second"], ctypes.c_void_p(X.ctypes.data),
                                        ctypes.c_void_p(X.ctypes.data), 2, _lib.OSP_HOST, ctypes.byref(out), None) == _lib.ERR_ARG
        assert out.value == 0x5555
    finally:
        part.close()


# ---- empty shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["empty_in", "no_rows"])
def test_an_empty_in_launches_nothing(mctx, case, dt):
    ncol, csr = tv._case(case, dt)
    M, k = len(csr[0]) - 1, 3
    src = _upload(mctx, ncol, csr)
    dX, dY = _to_dev(np.ones((M, k), dt)), _to_dev(np.ones((ncol, k), dt))
    torch.cuda.synchronize(DEV)
    try:
        for args, space in (((np.ones((M, k), dt), np.ones((ncol, k), dt)), "host"), ((dX, dY), "device")):
            res, st = src.sddmm(*args, accum="plus", space=space)
            try:
                assert res.shape == (M, ncol) and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(M + 1, np.int64))
                assert (st["launches"], st["nnz_in"], st["nnz_out"], st["cols"], st["lanes_per_entry"]) == (0, 0, 0, k, 4)
            finally:
                res.close()
    finally:
        src.close()


# ---- chaining and repetition ------------------------------------------------------------------------------------------------------------------
def test_sddmm_of_other_operations_results_fed_on_into_mxd(mctx):
    n, r, c, v = gen.rmat_coo(9, 8, "g500", seed=5)
    A = sp.csr_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    csr = (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(np.float64))
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((n, 7)), rng.standard_normal((n, 7))
    src = _upload(mctx, n, csr)
    made = []
    try:
        made.append(src.transpose()[0])
        made.append(src.select("triu")[0])
        made.append(src.mxm(src, "min", "plus")[0])
        for res in made:
            host = (res.rowptr.copy(), res.colidx.copy(), res.vals.copy())
            for add, mul, accum in [("plus", "times", "times"), ("min", "plus", "second")]:
                E, st = res.sddmm(X, Y, add, mul, accum, space="host")
                try:
                    want, computed = model.sddmm(*host, X, Y, add, mul, accum)
                    _assert_values(E.vals, want, computed)
                    assert st["nnz_in"] == res.nnz
                    Z, _ = E.mxd(Y, space="host")   # the forward of an attention layer: scores, then the weighted sum
                    assert np.array_equal(_bits(Z), _bits(mxd_model.mxd(host[0], host[1], want, Y, "plus", "times")[0]))
                finally:
                    E.close()
    finally:
        for res in made:
            res.close()
        src.close()


def test_fifty_back_to_back_calls_give_the_same_bits_and_the_pool_does_not_grow(mctx, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call, and after the first call no call allocates device memory:
    the library's own count of pool misses (hipMalloc calls of the context, printed under OSP_VERBOSE) stays where the first
    call left it."""
    ncol, csr, Xall, Yall = _main(np.float64)
    k = 17
    src = _upload(mctx, ncol, csr)
    dX, dY = _to_dev(Xall[:, :k]), _to_dev(Yall[:, :k])
    torch.cuda.synchronize(DEV)
    monkeypatch.setenv("OSP_VERBOSE", "1")
    misses, first = [], None
    try:
        for i in range(50):
            capfd.readouterr()
            res, _ = src.sddmm(dX, dY, accum="minus")
            err = capfd.readouterr().err
            found = re.findall(r"\[osp\] sddmm .*pool misses so far: (\d+) hipMalloc calls", err)
            assert len(found) == 1, err
            misses.append(int(found[0]))
            got = _bits(res.vals).copy()
            res.close()
            if first is None:
                first = got
            assert np.array_equal(got, first), i
    finally:
        src.close()
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses
    want = model.sddmm(*csr, np.ascontiguousarray(Xall[:, :k]), np.ascontiguousarray(Yall[:, :k]), accum="minus")[0]
    assert np.array_equal(first, _bits(want))
