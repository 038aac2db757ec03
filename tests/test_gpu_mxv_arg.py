"""osp_csr_mxv_arg on the GPU against tests/mxv_arg_model.py AND against osp_csr_mxv: arg equal as integers, y equal to mxv's
y as BITS (compared as unsigned integers).  Inputs are tests/test_gpu_apply_mask.py's, the vectors tests/test_gpu_vector.py's,
the packing shape tests/test_gpu_mxv.py's; the rows with ties are written out by hand."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import mxd_model
from tests import mxv_arg_model as model
from tests import test_gpu_apply_mask as am   # the input builders only
from tests import test_gpu_vector as tv       # its cached inputs and vectors only
from tests import test_gpu_mxv as tm          # its packing shape only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
_to_dev = tm._to_dev
_tdt = tm._tdt
DTYPES = [np.float32, np.float64]
SEMIRINGS = [(add, mul) for add in model.ADD_OPS for mul in model.MUL_OPS]
IDENTITY = {"min": np.inf, "max": -np.inf}


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _want_arg(case, dt, add, mul):
    ncol, csr = tv._case(case, dt)
    return model.arg_rows(csr[0], csr[1], _products(case, dt, mul), add)


@functools.lru_cache(maxsize=None)
def _products(case, dt, mul):
    ncol, csr = tv._case(case, dt)
    return model.products(*csr, tm._x(case, dt), mul)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- against the model and against mxv --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["traps", "frontier", "short_rows"])
def test_mxv_arg_equals_model_and_mxv(mctx, case, dt):
    ncol, csr = tv._case(case, dt)
    M, nnz = len(csr[0]) - 1, len(csr[1])
    src = _upload(mctx, ncol, csr)
    dx = _to_dev(tm._x(case, dt))
    torch.cuda.synchronize(DEV)
    try:
        for add, mul in SEMIRINGS:
            want = _want_arg(case, dt, add, mul)
            y, arg, st = src.mxv_arg(dx, add, mul)
            assert arg.dtype == torch.int64 and arg.shape == (M,)
            arg = arg.cpu().numpy()
            assert np.array_equal(arg, want), (add, mul, np.flatnonzero(arg != want)[:5])
            ref, sr = src.mxv(dx, add, mul)
            assert _same_bits(y.cpu().numpy(), ref.cpu().numpy()), (add, mul)
            assert (st["nnz_in"], st["nnz_out"], st["long_segments"], st["group"]) == (nnz, M, sr["long_segments"], sr["group"])
            assert st["rows_without"] == int((want < 0).sum()) and st["launches"] > 0 and st["ms_total"] >= 0
            none, only, _ = src.mxv_arg(dx, add, mul, values=False)
            assert none is None and np.array_equal(only.cpu().numpy(), want), (add, mul)
    finally:
        src.close()


# ---- the packing edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_every_group_gives_the_same_arg_and_the_same_bits(mctx, dt, monkeypatch):
    ncol, csr, x = tm._packing(dt)
    src = _upload(mctx, ncol, csr)
    try:
        for add, mul in [("min", "times"), ("min", "plus"), ("max", "second"), ("max", "first")]:
            want = model.arg_rows(csr[0], csr[1], model.products(*csr, x, mul), add)
            monkeypatch.delenv("OSP_MXV_GROUP", raising=False)
            ref, _ = src.mxv(x, add, mul, space="host")
            for g in model.GROUPS + [None]:
                if g is None:
                    monkeypatch.delenv("OSP_MXV_GROUP", raising=False)
                else:
                    monkeypatch.setenv("OSP_MXV_GROUP", str(g))
                y, arg, st = src.mxv_arg(x, add, mul, space="host")
                assert st["group"] == g if g else st["group"] in model.GROUPS
                assert st["long_segments"] == 1
                assert isinstance(arg, np.ndarray) and arg.dtype == np.int64
                assert np.array_equal(arg, want), (add, mul, g, np.flatnonzero(arg != want)[:5])
                assert _same_bits(y, ref), (add, mul, g)
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_launches_follow_the_formula(mctx, dt):
    """stats.launches is osp_csr_mxv's count (tests/test_gpu_mxv.py) plus the two of the stats' rows_without."""
    ncol = 1 << 12
    x = np.random.default_rng(46).standard_normal(ncol).astype(dt)
    for lengths, launches in zip(tv.LAUNCH_SHAPES, (1 + 2, 3 + 2, 7 + 2)):
        csr = am._csr_from_lengths(lengths, ncol, dt, seed=45)
        src = _upload(mctx, ncol, csr)
        try:
            for add, mul in [("min", "times"), ("max", "plus")]:
                y, arg, st = src.mxv_arg(x, add, mul, space="host")
                assert np.array_equal(arg, model.arg_rows(csr[0], csr[1], model.products(*csr, x, mul), add)), (lengths, add, mul)
                assert st["launches"] == launches == mxd_model.expected_launches(csr[0], scan_launches=1) + 2, (lengths, add, mul)
        finally:
            src.close()


# ---- rows with ties, written out by hand ------------------------------------------------------------------------------------------
def _tie_rows(dt):
    """(ncol, csr, expected arg under min, expected arg under max) with mul = first.  Column of position t of a row is
    10 + 3 t, so "the column of position t" is a number one can read."""
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(51)

    def noise(k):                        # values in [2, 3): never a minimum below 1 nor a maximum above 4
        return 2.0 + rng.random(k)

    def planted(k, positions, lo=1.0, hi=4.0):
        """A row of k entries with `lo` (the minimum) at `positions` and `hi` (the maximum) one position before each."""
        v = noise(k)
        for t in positions:
            v[t], v[t - 1] = lo, hi
        return v

    rows, amin, amax = [], [], []

    def add(v, lo_pos, hi_pos):
        rows.append(np.asarray(v, np.float64))
        amin.append(-1 if lo_pos is None else 10 + 3 * lo_pos)
        amax.append(-1 if hi_pos is None else 10 + 3 * hi_pos)

    for _ in range(16):                                      # a whole batch of short rows under every g: the packed path
        add([5.0, 7.0, 5.0, 7.0], 0, 1)
    add(planted(200, [3, 70, 130]), 3, 2)                    # the extreme three times, in lanes 3, 6 and 2
    add(planted(200, [70, 130]), 70, 69)                     # the smaller column in the HIGHER lane (6 against 2)
    add([], None, None)
    add(planted(4100, [4099, 2050, 5]), 5, 4)                # three blocks: the extreme in the last, the second and the first
    add(planted(4100, [4099, 2050]), 2050, 2049)             # ... and in the last two only
    add([], None, None)
    add([2.0, 0.0, 1.0, -0.0, 3.0], 1, 4)                    # min: +0.0 before -0.0
    add([2.0, -0.0, 1.0, 0.0, 3.0], 1, 4)                    # min: -0.0 before +0.0
    add([-2.0, 0.0, -1.0, -0.0, -3.0], 4, 1)                 # max: +0.0 before -0.0
    add([-2.0, -0.0, -1.0, 0.0, -3.0], 4, 1)                 # max: -0.0 before +0.0
    add([nan, nan, nan], None, None)                         # all NaN: no position, the identity
    add([], None, None)
    add([nan, inf, nan], 1, 1)                               # the only number is min's identity
    add([nan, -inf], 1, 1)                                   # the only number is max's identity
    add([nan] * 70 + [1.5] + [nan] * 9, 70, 70)              # one number among NaNs, beyond the first 64 lanes' first step
    add([], None, None)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([10 + 3 * np.arange(len(r), dtype=np.int64) for r in rows]).astype(np.uint32)
    val = np.concatenate(rows).astype(dt)
    return 10 + 3 * 4100, (rowptr, col, val), np.array(amin, np.int64), np.array(amax, np.int64)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("group", [None, 4, 64])
def test_ties_nans_zeros_and_identities(mctx, dt, group, monkeypatch):
    ncol, csr, amin, amax = _tie_rows(dt)
    if group is None:
        monkeypatch.delenv("OSP_MXV_GROUP", raising=False)
    else:
        monkeypatch.setenv("OSP_MXV_GROUP", str(group))
    src = _upload(mctx, ncol, csr)
    ones = np.ones(ncol, dt)
    try:
        for add, want in (("min", amin), ("max", amax)):
            assert np.array_equal(model.arg_rows(csr[0], csr[1], csr[2], add), want)     # the model reads the rows as their author did
            for mul, x in (("first", None), ("times", ones)):                            # (v * 1.0 is v, zeros' signs and NaNs included)
                y, arg, st = src.mxv_arg(x, add, mul, space="host")
                assert np.array_equal(arg, want), (add, mul, np.flatnonzero(arg != want))
                ref, _ = src.mxv(x, add, mul, space="host")
                assert _same_bits(y, ref), (add, mul)
                assert st["rows_without"] == int((want < 0).sum()) == 5 and st["long_segments"] == 2
                assert (y[want < 0] == IDENTITY[add]).all() and not np.isnan(y).any()
    finally:
        src.close()


def test_second_level_longer_than_a_block(mctx):
    """ONE float32 row of 2048 * 2048 + 5 entries: the blocks' pairs are themselves longer than a block.  The minimum sits in
    the last block (the second segment of the second level) and at position 3000; the maximum only in the last block."""
    m = 2048 * 2048 + 5
    rng = np.random.default_rng(22)
    val = (2.0 + rng.random(m)).astype(np.float32)
    val[[3000, m - 2]] = 1.0
    val[m - 1] = 4.0
    csr = (np.array([0, 0, m, m], np.int64), np.arange(m, dtype=np.uint32), val)
    src = _upload(mctx, 1 << 23, csr)
    try:
        for add, where in (("min", 3000), ("max", m - 1)):
            y, arg, st = src.mxv_arg(None, add, "first", space="host")
            ref, _ = src.mxv(None, add, "first", space="host")
            assert arg.tolist() == [-1, where, -1] and _same_bits(y, ref)
            assert (st["long_segments"], st["rows_without"]) == (1, 2)
    finally:
        src.close()


# ---- aliasing, argument forms, failure ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["host", "device"])
def test_out_is_x_on_a_square_input(mctx, space):
    n = 3000
    rng = np.random.default_rng(17)
    csr = am._csr_from_lengths(rng.integers(0, 40, n), n, np.float64, seed=18, lo=0)
    x = rng.standard_normal(n)
    want_y, want_arg, _, _ = model.mxv_arg(*csr, x, "min", "times")
    src = _upload(mctx, n, csr)
    try:
        if space == "host":
            v, a = x.copy(), np.full(n, 7, np.int64)
            y, arg, _ = src.mxv_arg(v, "min", "times", out=v, out_arg=a, space="host")
            assert y is v and arg is a and _same_bits(v, want_y) and np.array_equal(a, want_arg)
        else:
            v, a = _to_dev(x), torch.full((n,), 7, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize(DEV)
            y, arg, _ = src.mxv_arg(v, "min", "times", out=v, out_arg=a)
            assert y is v and arg is a and _same_bits(v.cpu().numpy(), want_y) and np.array_equal(a.cpu().numpy(), want_arg)
            with pytest.raises(S.OspError):
                src.mxv_arg(v, out_arg=torch.zeros(n, dtype=torch.float64, device=DEV))
            with pytest.raises(S.OspError):
                src.mxv_arg(v, out_arg=torch.zeros(n + 1, dtype=torch.int64, device=DEV))
    finally:
        src.close()


def _semiring(add, mul, reserved=0):
    sr = _lib.Semiring()
    sr.add, sr.mul = add, mul
    sr.reserved[3] = reserved
    return sr


def test_argument_errors_leave_y_arg_and_stats_alone(mctx):
    ncol, csr = tv._case("traps", np.float64)
    M = len(csr[0]) - 1
    src = _upload(mctx, ncol, csr)
    L = _lib.lib()
    E = _lib.EWISE_OPS
    x, y, arg = np.ones(ncol), np.full(M, 7.0), np.full(M, 7, np.int64)
    xp, yp, ap = (ctypes.c_void_p(a.ctypes.data) for a in (x, y, arg))
    stats = _lib.MxvArgStats()
    stats.nnz_in = 77
    good = _semiring(E["min"], E["times"])
    H = _lib.OSP_HOST

    def call(in_=src._h, sr=good, x_=xp, y_=yp, a_=ap, space=H):
        return L.osp_csr_mxv_arg(in_, None if sr is None else ctypes.byref(sr), x_, y_, a_, space, ctypes.byref(stats))

    calls = [lambda: call(in_=None), lambda: call(sr=None), lambda: call(a_=None), lambda: call(x_=None),
             lambda: call(sr=_semiring(E["max"], E["second"]), x_=None),
             lambda: call(sr=_semiring(E["plus"], E["times"])), lambda: call(sr=_semiring(E["first"], E["times"])),
             lambda: call(sr=_semiring(E["times"], E["times"])), lambda: call(sr=_semiring(E["min"], E["minus"])),
             lambda: call(sr=_semiring(E["min"], E["div"])), lambda: call(sr=_semiring(-1, E["times"])),
             lambda: call(sr=_semiring(E["min"], 99)), lambda: call(sr=_semiring(E["min"], E["times"], reserved=1)),
             lambda: call(space=99)]
    try:
        for i, c in enumerate(calls):
            assert c() == _lib.ERR_ARG, i
            assert L.osp_last_error_string()
            assert stats.nnz_in == 77 and (y == 7.0).all() and (arg == 7).all(), i
        # the same call with nothing wrong and without stats, then without y
        want_y, want_arg, _, _ = model.mxv_arg(*csr, x, "min", "times")
        assert L.osp_csr_mxv_arg(src._h, ctypes.byref(good), xp, yp, ap, H, None) == _lib.OSP_OK
        assert _same_bits(y, want_y) and np.array_equal(arg, want_arg)
        arg[:] = 7
        assert call(y_=None) == _lib.OSP_OK and np.array_equal(arg, want_arg) and stats.nnz_in == len(csr[1])
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
    vec, y, arg = np.ones(n), np.full(n, 5.0), np.full(n, 5, np.int64)
    E = _lib.EWISE_OPS
    try:
        assert _lib.lib().osp_csr_mxv_arg(part._h, ctypes.byref(_semiring(E["min"], E["times"])), ctypes.c_void_p(vec.ctypes.data),
                                          ctypes.c_void_p(y.ctypes.data), ctypes.c_void_p(arg.ctypes.data), _lib.OSP_HOST,
                                          None) == _lib.ERR_ARG
        assert (y == 5.0).all() and (arg == 5).all()
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
            y, arg, st = src.mxv_arg(np.ones(ncol, dt), add, "times", space="host")
            assert _same_bits(y, want) and arg.dtype == np.int64 and arg.shape == (M,) and (arg == -1).all()
            assert (st["launches"], st["nnz_in"], st["nnz_out"], st["long_segments"], st["rows_without"]) == (0, 0, M, 0, M)
            y, arg, st = src.mxv_arg(dx, add, "second")
            assert st["launches"] == 0 and _same_bits(y.cpu().numpy(), want) and (arg.cpu().numpy() == -1).all() and arg.shape == (M,)
            none, arg, st = src.mxv_arg(None, add, "first", values=False)
            assert none is None and st["launches"] == 0 and (arg.cpu().numpy() == -1).all()
    finally:
        src.close()


# ---- the column axis ----------------------------------------------------------------------------------------------------------------
def test_the_column_axis_is_the_transpose_first(mctx):
    n, r, c, v = gen.rmat_coo(10, 8, "g500", seed=5)
    A = sp.csr_matrix((np.round(v * 8), (r, c)), shape=(n + 7, n)); A.sort_indices()     # (rounded: ties)
    csr = (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data.astype(np.float64))
    At = A.T.tocsr(); At.sort_indices()
    tcsr = (At.indptr.astype(np.int64), At.indices.astype(np.uint32), At.data.astype(np.float64))
    x = np.random.default_rng(3).integers(1, 4, n + 7).astype(np.float64)
    src = _upload(mctx, n, csr)
    T = None
    try:
        T = src.transpose()[0]
        for add, mul in [("min", "times"), ("max", "plus"), ("max", "first")]:
            want_y, want_arg, _, without = model.mxv_arg(*tcsr, x, add, mul)
            y, arg, st = T.mxv_arg(x, add, mul, space="host")
            assert np.array_equal(arg, want_arg) and _same_bits(y, want_y) and st["rows_without"] == without
    finally:
        if T is not None:
            T.close()
        src.close()
