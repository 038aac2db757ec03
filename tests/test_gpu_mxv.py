"""osp_csr_mxv on the GPU against tests/mxv_model.py AND against the device composition it fuses (osp_csr_apply_vectors on the
column side, then osp_csr_reduce over the rows): vectors equal as BITS (compared as unsigned integers); where the value came
out of an addition (add = plus) a NaN is a NaN whatever its payload, as tests/test_gpu_vector.py compares them.  Inputs are
tests/test_gpu_apply_mask.py's, the vectors tests/test_gpu_vector.py's."""
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
from tests import mxv_model as model
from tests import test_gpu_apply_mask as am   # the input builders only
from tests import test_gpu_vector as tv       # its cached inputs and vectors only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
_assert_vector = tv._assert_vector
DTYPES = [np.float32, np.float64]
# every add, and TIMES, PLUS, SECOND, FIRST and (MAX, MIN) among the muls
SEMIRINGS = [("plus", "times"), ("min", "times"), ("max", "times"), ("plus", "plus"), ("min", "plus"), ("min", "second"), ("plus", "second"),
             ("max", "first"), ("plus", "first"), ("max", "min")]
IDENTITY = {"plus": 0.0, "min": np.inf, "max": -np.inf}


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _tdt(dt):
    return torch.float32 if dt == np.float32 else torch.float64


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV) if len(a) else torch.empty(1, dtype=_tdt(a.dtype.type), device=DEV)


@functools.lru_cache(maxsize=None)
def _want(case, dt, add, mul):
    ncol, csr = tv._case(case, dt)
    return model.mxv(*csr, _x(case, dt), add, mul)


def _x(case, dt):
    """N values with every special value on columns that hold entries (tests/test_gpu_vector.py's column vector)."""
    return tv._vectors(case, dt)[1]


def _composition(src, dx, add, mul):
    """reduce(rows, add) of apply_vectors(cols = x, col_op = mul) on the device; mul = first: reduce of the result itself."""
    if mul == "first":
        return src.reduce("rows", add)[0]
    prod, _ = src.apply_vectors(cols=dx, col_op=mul)
    try:
        return prod.reduce("rows", add)[0]
    finally:
        prod.close()


# ---- against the model and the composition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["traps", "frontier", "short_rows"])
def test_mxv_equals_model_and_composition(mctx, case, dt):
    ncol, csr = tv._case(case, dt)
    M, nnz = len(csr[0]) - 1, len(csr[1])
    x = _x(case, dt)
    if case == "traps":
        assert all(np.any(_bits(x) == b) for b in _bits(am._special(dt)))
    src = _upload(mctx, ncol, csr)
    dx = _to_dev(x)
    torch.cuda.synchronize(DEV)
    try:
        for add, mul in SEMIRINGS:
            want, nlong = _want(case, dt, add, mul)
            got, st = src.mxv(dx, add, mul, space="device")
            got = got.cpu().numpy()
            _assert_vector(got, want, add)
            _assert_vector(got, _composition(src, dx, add, mul), add)
            assert (st["nnz_in"], st["nnz_out"], st["long_segments"]) == (nnz, M, nlong), (add, mul)
            assert st["group"] in model.GROUPS and st["launches"] > 0 and st["ms_total"] >= 0
            if add != "plus":
                assert not np.isnan(got).any()
        assert _want(case, dt, "plus", "times")[1] == {"traps": 3, "frontier": 1, "short_rows": 0}[case]
        if case == "traps":
            assert np.isnan(_want(case, dt, "plus", "times")[0]).any()
    finally:
        src.close()


# ---- the packing edges ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packing(dt):
    """Row lengths 0, 1, g - 1, g, g + 1 for every g, a row of 2049 between rows of 2, 100 empty rows; M = 128 + 3: the last
    wave is partial under every g.  Special values among the entries and in x."""
    lengths = []
    for g in model.GROUPS:
        lengths += [0, 1, g - 1, g, g + 1]
    lengths += [2, 2049, 2] + [0] * 100 + [3, 4, 5]
    assert len(lengths) % 16 != 0
    ncol = 1 << 12
    rowptr, col, val = am._csr_from_lengths(lengths, ncol, dt, seed=41)
    sp_ = am._special(dt)
    rng = np.random.default_rng(42)
    val[rng.choice(len(val), 4 * len(sp_), replace=False)] = np.resize(sp_, 4 * len(sp_))
    x = rng.standard_normal(ncol).astype(dt)
    x[rng.choice(ncol, 8 * len(sp_), replace=False)] = np.resize(sp_, 8 * len(sp_))
    for a in (rowptr, col, val, x):
        a.setflags(write=False)
    return ncol, (rowptr, col, val), x


@pytest.mark.parametrize("dt", DTYPES)
def test_every_group_gives_the_same_bits(mctx, dt, monkeypatch):
    ncol, csr, x = _packing(dt)
    src = _upload(mctx, ncol, csr)
    try:
        for add, mul in [("plus", "times"), ("min", "plus"), ("max", "second"), ("plus", "first")]:
            want, nlong = model.mxv(*csr, x, add, mul)
            assert nlong == 1
            got = {}
            for g in model.GROUPS + [None]:
                if g is None:
                    monkeypatch.delenv("OSP_MXV_GROUP", raising=False)
                else:
                    monkeypatch.setenv("OSP_MXV_GROUP", str(g))
                got[g], st = src.mxv(x, add, mul, space="host")
                assert st["group"] == g if g else st["group"] in model.GROUPS
                assert st["long_segments"] == 1
                _assert_vector(got[g], want, add)
            for g in model.GROUPS:
                assert np.array_equal(_bits(got[g]), _bits(got[None])), (add, mul, g)
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_launches_follow_the_formula(mctx, dt):
    """stats.launches is osp_csr_mxd's count (tests/mxd_model.py): the rows kernel; the zeroing and the listing of the long
    rows; with a long row the setup, the scan (one launch for one entry), the blocks and the next level's short kernel."""
    ncol = 1 << 12
    x = np.random.default_rng(44).standard_normal(ncol).astype(dt)
    for lengths, launches in zip(tv.LAUNCH_SHAPES, (1, 3, 7)):
        csr = am._csr_from_lengths(lengths, ncol, dt, seed=43)
        src = _upload(mctx, ncol, csr)
        try:
            for add, mul in [("plus", "times"), ("min", "plus")]:
                got, st = src.mxv(x, add, mul, space="host")
                _assert_vector(got, model.mxv(*csr, x, add, mul)[0], add)
                assert st["launches"] == launches == mxd_model.expected_launches(csr[0], scan_launches=1), (lengths, add, mul)
        finally:
            src.close()


def test_a_product_and_its_addition_are_two_roundings(mctx):
    ncol, csr, x = model.fma_telling_input()
    want, _ = model.mxv(*csr, x, "plus", "times")
    fused = model.fma_mxv_plus_times(*csr, x)
    src = _upload(mctx, ncol, csr)
    try:
        got, _ = src.mxv(x, space="host")
        assert np.array_equal(_bits(got), _bits(want))
        assert (_bits(got) != _bits(fused)).any()
    finally:
        src.close()


# ---- shapes and argument forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_one_column(mctx, dt):
    rng = np.random.default_rng(7)
    lengths = rng.integers(0, 2, 1000)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    csr = (rowptr, np.zeros(int(rowptr[-1]), np.uint32), rng.standard_normal(int(rowptr[-1])).astype(dt))
    x = np.array([-2.5], dt)
    src = _upload(mctx, 1, csr)
    try:
        for add, mul in [("plus", "times"), ("min", "plus"), ("max", "second")]:
            got, st = src.mxv(x, add, mul, space="host")
            assert np.array_equal(_bits(got), _bits(model.mxv(*csr, x, add, mul)[0]))
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_x_and_out_on_the_host_and_on_the_device(mctx, dt):
    ncol, csr = tv._case("traps", dt)
    M = len(csr[0]) - 1
    x = _x("traps", dt)
    want = _want("traps", dt, "min", "plus")[0]
    src = _upload(mctx, ncol, csr)
    try:
        h, _ = src.mxv(x, "min", "plus", space="host")
        assert isinstance(h, np.ndarray) and np.array_equal(_bits(h), _bits(want))
        buf = np.full(M, 7.0, dt)
        ret, _ = src.mxv(list(x), "min", "plus", out=buf, space="host")
        assert ret is buf and np.array_equal(_bits(buf), _bits(want))
        dx = _to_dev(x)
        out = torch.full((M,), 7.0, dtype=_tdt(dt), device=DEV)
        torch.cuda.synchronize(DEV)
        ret, _ = src.mxv(dx, "min", "plus", out=out)
        assert ret is out and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        out.fill_(7.0)
        torch.cuda.synchronize(DEV)
        raw, _ = src.mxv(dx.data_ptr(), "min", "plus", out=out.data_ptr())
        assert raw == out.data_ptr() and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        fresh, _ = src.mxv(dx, "min", "plus")
        assert torch.is_tensor(fresh) and fresh.shape == (M,) and np.array_equal(_bits(fresh.cpu().numpy()), _bits(want))
        with pytest.raises(S.OspError):
            src.mxv(dx, out=torch.zeros(M + 1, dtype=_tdt(dt), device=DEV))
        with pytest.raises(S.OspError):
            src.mxv(x[:-1], space="host")
        with pytest.raises(S.OspError):
            src.mxv(None)
        with pytest.raises(ValueError):
            src.mxv(dx, add="first")
        with pytest.raises(ValueError):
            src.mxv(dx, mul="div")
    finally:
        src.close()


@pytest.mark.parametrize("space", ["host", "device"])
def test_out_is_x_on_a_square_input(mctx, space):
    n = 3000
    rng = np.random.default_rng(17)
    csr = am._csr_from_lengths(rng.integers(0, 40, n), n, np.float64, seed=18, lo=0)
    x = rng.standard_normal(n)
    want = model.mxv(*csr, x, "plus", "times")[0]
    src = _upload(mctx, n, csr)
    try:
        if space == "host":
            v = x.copy()
            ret, _ = src.mxv(v, out=v, space="host")
            assert ret is v and np.array_equal(_bits(v), _bits(want))
        else:
            v = _to_dev(x)
            torch.cuda.synchronize(DEV)
            ret, _ = src.mxv(v, out=v)
            assert ret is v and np.array_equal(_bits(v.cpu().numpy()), _bits(want))
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_first_reads_no_x(mctx, dt):
    ncol, csr = tv._case("traps", dt)
    src = _upload(mctx, ncol, csr)
    try:
        for add in model.ADD_OPS:
            got, st = src.mxv(None, add, "first", space="host")
            _assert_vector(got, tv._want_reduce("traps", dt, "rows", add)[0], add)
            dev, _ = src.mxv(None, add, "first")
            assert np.array_equal(_bits(dev.cpu().numpy()), _bits(got))
    finally:
        src.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _semiring(add, mul, reserved=0):
    sr = _lib.Semiring()
    sr.add, sr.mul = add, mul
    sr.reserved[3] = reserved
    return sr


def test_argument_errors_leave_y_and_stats_alone(mctx):
    ncol, csr = tv._case("traps", np.float64)
    M = len(csr[0]) - 1
    src = _upload(mctx, ncol, csr)
    L = _lib.lib()
    E = _lib.EWISE_OPS
    x, y = np.ones(ncol), np.full(M, 7.0)
    xp, yp = ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data)
    stats = _lib.MxvStats()
    stats.nnz_in = 77
    good = _semiring(E["plus"], E["times"])
    H = _lib.OSP_HOST
    calls = [lambda: L.osp_csr_mxv(None, ctypes.byref(good), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, None, xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(good), xp, None, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(good), None, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["min"], E["second"])), None, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["first"], E["times"])), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["times"], E["times"])), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["plus"], E["minus"])), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["plus"], E["div"])), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(-1, E["times"])), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["plus"], 99)), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(_semiring(E["plus"], E["times"], reserved=1)), xp, yp, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(src._h, ctypes.byref(good), xp, yp, 99, ctypes.byref(stats))]
    try:
        for i, call in enumerate(calls):
            assert call() == _lib.ERR_ARG, i
            assert L.osp_last_error_string()
            assert stats.nnz_in == 77 and (y == 7.0).all(), i
        # the same call with nothing wrong, and without stats
        assert L.osp_csr_mxv(src._h, ctypes.byref(good), xp, yp, H, None) == _lib.OSP_OK
        _assert_vector(y, model.mxv(*csr, x, "plus", "times")[0], "plus")
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
    vec, y = np.ones(n), np.full(n, 5.0)
    E = _lib.EWISE_OPS
    try:
        assert _lib.lib().osp_csr_mxv(part._h, ctypes.byref(_semiring(E["plus"], E["times"])), ctypes.c_void_p(vec.ctypes.data),
                                      ctypes.c_void_p(y.ctypes.data), _lib.OSP_HOST, None) == _lib.ERR_ARG
        assert (y == 5.0).all()
    finally:
        part.close()


# ---- empty shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["empty_in", "no_rows"])
def test_empty_shapes_launch_nothing(mctx, case, dt):
    ncol, csr = tv._case(case, dt)
    M = len(csr[0]) - 1
    src = _upload(mctx, ncol, csr)
    dx = _to_dev(np.ones(ncol, dt))
    torch.cuda.synchronize(DEV)
    try:
        for add in model.ADD_OPS:
            want = np.full(M, IDENTITY[add], dt)
            got, st = src.mxv(np.ones(ncol, dt), add, "times", space="host")
            assert got.shape == (M,) and np.array_equal(_bits(got), _bits(want))
            assert (st["launches"], st["nnz_in"], st["nnz_out"], st["long_segments"]) == (0, 0, M, 0)
            dev, st = src.mxv(dx, add, "second")
            assert st["launches"] == 0 and np.array_equal(_bits(dev.cpu().numpy()), _bits(want))
    finally:
        src.close()


# ---- chaining ---------------------------------------------------------------------------------------------------------------------
def test_mxv_of_other_operations_results(mctx):
    n, r, c, v = gen.rmat_coo(10, 8, "g500", seed=5)
    A = sp.csr_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    csr = (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(np.float64))
    x = np.random.default_rng(3).standard_normal(n)
    src = _upload(mctx, n, csr)
    made = []
    try:
        made.append(src.transpose()[0])
        made.append(src.select("triu")[0])
        made.append(src.mxm(src, "min", "plus")[0])
        for res in made:
            host = (res.rowptr.copy(), res.colidx.copy(), res.vals.copy())
            for add, mul in [("plus", "times"), ("min", "plus")]:
                got, st = res.mxv(x, add, mul, space="host")
                assert np.array_equal(_bits(got), _bits(model.mxv(*host, x, add, mul)[0])) and st["nnz_in"] == res.nnz
        # the transpose's product is scipy's A^T x up to the order of summation
        assert np.allclose(made[0].mxv(x, space="host")[0], A.T @ x, rtol=1e-12, atol=1e-12)
    finally:
        for res in made:
            res.close()
        src.close()


def test_fifty_back_to_back_calls_give_the_same_bits_and_the_pool_does_not_grow(mctx, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call, and after the first call no call allocates device memory:
    the library's own count of pool misses (hipMalloc calls of the context, printed under OSP_VERBOSE) stays where the first
    call left it."""
    ncol, csr = tv._case("traps", np.float64)
    src = _upload(mctx, ncol, csr)
    dx = _to_dev(_x("traps", np.float64))
    out = torch.empty(len(csr[0]) - 1, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    monkeypatch.setenv("OSP_VERBOSE", "1")
    misses, first = [], None
    try:
        for i in range(50):
            capfd.readouterr()
            src.mxv(dx, "plus", "times", out=out)
            err = capfd.readouterr().err
            found = re.findall(r"\[osp\] mxv .*pool misses so far: (\d+) hipMalloc calls", err)
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
