"""osp_csr_mxm on the GPU: (PLUS, TIMES) against the library's own product bit for bit, and all 24 semirings against
tests/semiring_model.py -- row pointers and columns exact, values equal as BITS (compared as unsigned integers; a NaN that
came out of an arithmetic operation is a NaN whatever its payload, as tests/test_gpu_ewise.py compares them)."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from outerspace_amd.sparse_util import _result_as_input
from tests import semiring_model as model
from tests import test_gpu_apply_mask as am   # _upload, _dev, _bits only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
CAP = model.SHORT_CAP
DTYPES = [np.float32, np.float64]
SEMIRINGS = [(a, m) for a in model.ADD_OPS for m in model.MUL_OPS]


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _assert_same(res, want, what=""):
    rowptr, col, val = want
    assert res.nnz == len(col) == res.info["nnz_c"], what
    assert np.array_equal(res.rowptr, rowptr), what
    assert np.array_equal(res.colidx, col), what
    got = res.vals
    assert got.dtype == val.dtype
    nan = np.isnan(val)
    assert np.isnan(got[nan]).all() and np.array_equal(_bits(got[~nan]), _bits(val[~nan])), what


# ---- the built pair ---------------------------------------------------------------------------------------------------------------
# B (K x N): rows 0..5999 hold ONE entry each, all at column 7 (a PILE: an A row that points at m of them has one output entry
# fed by m products, in ascending k); rows 6000..6099 one entry each at distinct columns; row 6100 is EMPTY; rows 6101..6110
# hold 200 entries each at random columns (they overlap: runs of 2 and more); row 6111 holds columns 0..63, row 6112 0..62.
K, N = 6113, 3000
PILE, SINGLE, EMPTY, WIDE, R64, R63 = 0, 6000, 6100, 6101, 6111, 6112
# the rows of A: (the rows of B it points at) -> its products
A_ROWS = [
    [],                                                                   # 0: an empty row of A
    [EMPTY],                                                              # 1: no product, though the row has an entry
    [SINGLE],                                                             # 2: 1
    [R63],                                                                # 3: 63
    [R64],                                                                # 4: 64
    [SINGLE, R64],                                                        # 5: 65
    list(range(23)) + [EMPTY] + list(range(WIDE, WIDE + 5)),              # 6: cap - 1
    list(range(24)) + list(range(WIDE, WIDE + 5)),                        # 7: cap
    list(range(25)) + list(range(WIDE, WIDE + 5)),                        # 8: cap + 1 (the first long row)
    list(range(1077)) + list(range(WIDE, WIDE + 10)),                     # 9: 3 cap + 5; an entry fed by 1077 products
    list(range(5000)) + [SINGLE + 1],                                     # 10: an entry fed by 5000 products, one fed by 1
    list(range(100, 165)),                                                # 11: short, ONE entry fed by 65 products
    [0, 1, SINGLE + 2, WIDE, WIDE + 1],                                   # 12: an entry fed by 2
    [5990, 5991, 5992],                                                   # 13: 1e16, 1, -1e16 under PLUS: the order is visible
    [5993, 5994, 5995, 5996, 5997],                                       # 14: NaN, -0.0, +0.0, +inf, -inf under MIN, MAX, FIRST
    [5998],                                                               # 15: a lone -0.0
    [],                                                                   # 16
    list(range(2000, 2000 + 3 * CAP)) + list(range(WIDE, WIDE + 10)),     # 17: a long row after short ones
    [],                                                                   # 18: empty rows at the end
    [],
]
PRODUCTS = [0, 0, 1, 63, 64, 65, CAP - 1, CAP, CAP + 1, 3 * CAP + 5, 5001, 65, 403, 3, 5, 1, 0, 3 * CAP + 2000, 0, 0]


@functools.lru_cache(maxsize=None)
def _pair(dt):
    rng = np.random.default_rng(77)
    lens = np.ones(K, np.int64)
    lens[EMPTY] = 0
    lens[WIDE:WIDE + 10] = 200
    lens[R64], lens[R63] = 64, 63
    bp = np.concatenate([[0], np.cumsum(lens)])
    bc = np.empty(bp[-1], np.uint32)
    bc[bp[:6000]] = 7
    bc[bp[6000:6100]] = 100 + np.arange(100)
    for r in range(WIDE, WIDE + 10):
        bc[bp[r]:bp[r + 1]] = np.sort(rng.choice(400, 200, replace=False)) * 7     # (columns 0, 7, 14, ...: the pile's 7 among them)
    bc[bp[R64]:bp[R64 + 1]] = np.arange(64)
    bc[bp[R63]:bp[R63 + 1]] = np.arange(63)
    bv = (rng.standard_normal(bp[-1]) * 10.0 ** rng.integers(-2, 3, bp[-1])).astype(dt)
    bv[bp[5990:5993]] = [1e16, 1.0, -1e16]
    bv[bp[5993:5998]] = [np.nan, -0.0, 0.0, np.inf, -np.inf]
    bv[bp[5998]] = -0.0
    bv[bp[3]], bv[bp[40]], bv[bp[700]] = np.nan, np.inf, -np.inf             # inside the long piles
    ap = np.concatenate([[0], np.cumsum([len(r) for r in A_ROWS])]).astype(np.int64)
    ac = np.array([k for r in A_ROWS for k in sorted(r)], np.uint32)
    av = rng.standard_normal(len(ac)).astype(dt)
    av[ap[13]:ap[16]] = 1.0                                                    # the special rows see B's values as they are
    av[ap[9] + 5] = 0.0                                                        # an explicit zero of A is an entry
    a, b = (ap, ac, av), (bp.astype(np.int64), bc, bv)
    for x in a + b:
        x.setflags(write=False)
    U = np.array([int(lens[sorted(r)].sum()) for r in A_ROWS])
    assert U.tolist() == PRODUCTS
    return a, b


@functools.lru_cache(maxsize=None)
def _want(dt, add, mul, cap=CAP, budget=model.BATCH):
    a, b = _pair(dt)
    return model.mxm(a, b, N, add, mul, cap, budget)


@pytest.fixture(scope="module")
def operands(mctx):
    made = {}
    for dt in DTYPES:
        a, b = _pair(dt)
        made[dt] = (_upload(mctx, K, a), _upload(mctx, N, b))
    yield made
    for ra, rb in made.values():
        ra.close()
        rb.close()


def _check_stats(st, res, wst, a, b):
    assert (st["nnz_a"], st["nnz_b"]) == (len(a[1]), len(b[1]))
    assert st["products"] == wst["products"] == res.info["partials"]
    assert (st["short_rows"], st["long_rows"], st["nnz_out"], st["batches"]) == \
        (wst["short_rows"], wst["long_rows"], wst["nnz_out"], wst["batches"])
    assert st["ms_total"] >= 0 and st["launches"] > 0
    info = res.info
    assert (info["M"], info["K"], info["N"], info["row_begin"], info["row_end"]) == (len(a[0]) - 1, len(b[0]) - 1, res.shape[1], 0, len(a[0]) - 1)
    assert (info["nnz_a"], info["nnz_b"], info["nnz_c"]) == (len(a[1]), len(b[1]), wst["nnz_out"])
    named = {"M", "K", "N", "row_begin", "row_end", "nnz_a", "nnz_b", "nnz_c", "partials", "dtype", "ms_total"}
    assert all(v == 0 for k, v in info.items() if k not in named), info


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("add,mul", SEMIRINGS)
def test_every_semiring_equals_the_model(operands, add, mul, dt):
    a, b = _pair(dt)
    ra, rb = operands[dt]
    want, wst = _want(dt, add, mul)
    res, st = ra.mxm(rb, add, mul)
    try:
        assert res.shape == (len(A_ROWS), N) and res.dtype == dt
        _assert_same(res, want, (add, mul))
        _check_stats(st, res, wst, a, b)
        assert (st["short_rows"], st["long_rows"], st["batches"]) == (11, 4, 1)
    finally:
        res.close()


def test_the_built_pair_makes_the_order_visible():
    """The model's values on the special rows are what section 1 says, and another order would give something else."""
    for dt in DTYPES:
        (rowptr, col, val), _ = _want(dt, "plus", "times")
        assert val[rowptr[13]] == 0.0 and val[rowptr[15]] == 0.0 and np.signbit(val[rowptr[15]])    # (1e16 + 1) - 1e16; a lone -0.0
        (rowptr, col, val), _ = _want(dt, "min", "second")
        assert np.isnan(val[rowptr[14]])                                       # MIN keeps p_0 = NaN
        (rowptr, col, val), _ = _want(dt, "first", "second")
        assert np.isnan(val[rowptr[14]])
        (rowptr, col, val), _ = _want(dt, "max", "second")
        assert np.isnan(val[rowptr[14]])


@pytest.mark.parametrize("dt", DTYPES)
def test_batches_give_the_unbatched_result(operands, monkeypatch, dt):
    a, b = _pair(dt)
    ra, rb = operands[dt]
    for add, mul in (("plus", "times"), ("min", "plus"), ("first", "second")):
        want, _ = _want(dt, add, mul)
        for budget in (1000, 1, 6000):
            monkeypatch.setenv("OSP_MXM_BATCH", str(budget))
            wst = _want(dt, add, mul, CAP, budget)[1]
            res, st = ra.mxm(rb, add, mul)
            monkeypatch.delenv("OSP_MXM_BATCH")
            try:
                _assert_same(res, want, (add, mul, budget))
                _check_stats(st, res, wst, a, b)
                assert st["batches"] == len(model.cut_batches(np.array(PRODUCTS), budget)) > 1
            finally:
                res.close()
    assert len(model.cut_batches(np.array(PRODUCTS), 1000)) == 9      # (0,6) (6,7) (7,8) (8,9) (9,10) (10,11) (11,17) (17,18) (18,20)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_short_cap_knob_moves_rows_between_the_classes(operands, monkeypatch, dt):
    a, b = _pair(dt)
    ra, rb = operands[dt]
    for cap in (64, 63, 1):
        monkeypatch.setenv("OSP_MXM_SHORT_CAP", str(cap))
        for add, mul in (("plus", "times"), ("max", "min")):
            want, wst = _want(dt, add, mul, cap)
            res, st = ra.mxm(rb, add, mul)
            try:
                _assert_same(res, want, (add, mul, cap))
                _check_stats(st, res, wst, a, b)
            finally:
                res.close()
        monkeypatch.delenv("OSP_MXM_SHORT_CAP")
    assert _want(dt, "plus", "times", 64)[1]["long_rows"] == 9 and _want(dt, "plus", "times", 63)[1]["long_rows"] == 10


# ---- the launch count -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_pair():
    """40 x 40 times 40 x 40, about 200 entries each, built by arithmetic: five entries a row, 25 products a row of a; row 7
    of a is empty, and its row 9 holds one entry, at the one entry of b's row 3: one product."""
    i, j = np.divmod(np.arange(1600), 40)

    def csr(keep):
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(i[keep], minlength=40))]).astype(np.int64)
        return rowptr, j[keep].astype(np.uint32), (1.0 + (np.flatnonzero(keep) % 7)).astype(np.float64)

    ka = (7 * i + 3 * j) % 8 == 0
    ka &= (i != 7) & ((i != 9) | (j < 8))
    return csr(ka), csr(((3 * i + 7 * j) % 8 == 0) & ((i != 3) | (j < 8)))


# st["launches"] of the three settings as commit acee2bd ("Test the product's summation paths on IEEE edge values, bit for
# bit") reports them on an MI355X, before the sorts counted their own launches: short rows only; every row of more than one
# product long (the sorted-runs path); that in several batches
MXM_LAUNCHES = {(None, None): 8, ("1", None): 24, ("1", "50"): 326}


@pytest.mark.parametrize("cap,batch", list(MXM_LAUNCHES))
def test_mxm_reports_its_launches(mctx, monkeypatch, cap, batch):
    for name, value in (("OSP_MXM_SHORT_CAP", cap), ("OSP_MXM_BATCH", batch)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    a, b = _small_pair()
    assert (len(a[1]), len(b[1])) == (191, 196)
    want, wst = model.mxm(a, b, 40, "plus", "times", int(cap or CAP), int(batch or model.BATCH))
    ra, rb = _upload(mctx, 40, a), _upload(mctx, 40, b)
    try:
        res, st = ra.mxm(rb)
        try:
            print("mxm launches", (cap, batch), st["launches"], st["short_rows"], st["long_rows"], st["batches"])
            _assert_same(res, want, (cap, batch))
            _check_stats(st, res, wst, a, b)
            assert (st["long_rows"] > 0) == (cap is not None) and (st["batches"] > 1) == (batch is not None)
            assert st["launches"] == MXM_LAUNCHES[cap, batch], (cap, batch, st)
        finally:
            res.close()
    finally:
        ra.close()
        rb.close()


# ---- (PLUS, TIMES) is the library's own product ---------------------------------------------------------------------------------
def _library_product(mctx, ra, rb):
    a, b = _result_as_input(ra, DEV), _result_as_input(rb, DEV)
    torch.cuda.synchronize(DEV)
    dt = ra.dtype
    return mctx.spgemm_coo_device(dt, ra.shape[0], ra.shape[1], rb.shape[1], a.nnz, (a.rows.data_ptr(), a.cols.data_ptr(), a.vals.data_ptr()),
                                  b.nnz, (b.rows.data_ptr(), b.cols.data_ptr(), b.vals.data_ptr()))


def _rmat_csr(scale, dt, seed=1):
    n, r, c, v = gen.rmat_coo(scale, 16, "g500", seed=seed, dtype=dt)
    return n, gen.coo_to_csr(n, r, c, v)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ["rmat10_self", "frontier64_rmat12"])
def test_plus_times_is_the_librarys_product_bit_for_bit(mctx, shape, dt):
    if shape == "rmat10_self":
        n, g = _rmat_csr(10, dt)
        ra = rb = _upload(mctx, n, g)
    else:
        n, g = _rmat_csr(12, dt)
        rng = np.random.default_rng(9)
        lens = rng.integers(0, 400, 64)
        lens[5] = 0
        fp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        fc = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]).astype(np.uint32)
        ra, rb = _upload(mctx, n, (fp, fc, rng.standard_normal(len(fc)).astype(dt))), _upload(mctx, n, g)
    lib = res = None
    try:
        lib = _library_product(mctx, ra, rb)
        res, st = ra.mxm(rb)            # the defaults are (plus, times)
        assert res.shape == lib.shape and res.nnz == lib.nnz > 0
        assert np.array_equal(res.rowptr, lib.rowptr) and np.array_equal(res.colidx, lib.colidx)
        assert np.array_equal(_bits(res.vals), _bits(lib.vals))
        assert st["products"] == lib.info["partials"] == res.info["partials"]
        assert st["long_rows"] > 0 and st["short_rows"] > 0
    finally:
        for x in {id(x): x for x in (lib, res, ra, rb) if x is not None}.values():
            x.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_same_handle_on_both_sides(mctx, dt):
    n, g = _rmat_csr(8, dt, seed=4)
    r = _upload(mctx, n, g)
    try:
        for add, mul in (("min", "plus"), ("max", "times"), ("first", "first")):
            res, st = r.mxm(r, add, mul)
            try:
                want, wst = model.mxm(g, g, n, add, mul)
                _assert_same(res, want, (add, mul))
                assert st["products"] == wst["products"]
            finally:
                res.close()
        assert np.array_equal(r.rowptr, g[0]) and np.array_equal(_bits(r.vals), _bits(g[2]))     # the operand stays valid
    finally:
        r.close()


def test_a_rectangular_chain(mctx):
    rng = np.random.default_rng(2)
    A = sp.random(3, 7, 0.6, random_state=1, format="csr", data_rvs=lambda k: rng.integers(1, 9, k).astype(np.float64))
    B = sp.random(7, 2, 0.6, random_state=2, format="csr", data_rvs=lambda k: rng.integers(1, 9, k).astype(np.float64))
    C = sp.random(2, 5, 0.8, random_state=3, format="csr", data_rvs=lambda k: rng.integers(1, 9, k).astype(np.float64))
    for m in (A, B, C):
        m.sort_indices()
    csr = lambda m: (m.indptr.astype(np.int64), m.indices.astype(np.uint32), m.data)   # noqa: E731
    ra, rb, rc = _upload(mctx, 7, csr(A)), _upload(mctx, 2, csr(B)), _upload(mctx, 5, csr(C))
    ab = abc = None
    try:
        ab, _ = ra.mxm(rb)
        assert ab.shape == (3, 2)
        abc, _ = ab.mxm(rc)
        want = (A @ B @ C).tocsr()
        want.sort_indices()
        assert abc.shape == (3, 5) and np.array_equal(abc.rowptr, want.indptr) and np.array_equal(abc.colidx, want.indices)
        assert np.array_equal(abc.vals, want.data)
        mp, _ = ra.mxm(rb, "min", "plus")
        _assert_same(mp, model.mxm(csr(A), csr(B), 2, "min", "plus")[0])
        mp.close()
    finally:
        for x in (ab, abc, ra, rb, rc):
            if x is not None:
                x.close()


# ---- errors and empty cases -----------------------------------------------------------------------------------------------------
def _raw(a, b, sr, out=True):
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    stats = _lib.MxmStats()
    stats.products = 77
    h = lambda r: r._h if r is not None else None   # noqa: E731
    st = _lib.lib().osp_csr_mxm(h(a), h(b), ctypes.byref(sr) if sr is not None else None, ctypes.byref(o) if out else None,
                                ctypes.byref(stats))
    return st, o.value == sentinel and stats.products == 77


def _sr(add=0, mul=1):
    s = _lib.Semiring()
    s.add, s.mul = add, mul
    return s


def test_argument_errors(mctx):
    rowptr = np.array([0, 2, 3, 3, 3], np.int64)
    col, val = np.array([0, 3, 1], np.uint32), np.array([1.0, 2.0, 3.0])
    res = mctx.merge_csr_parts(4, 4, [(rowptr, col, val)])
    f32 = mctx.merge_csr_parts(4, 4, [(rowptr, col, val.astype(np.float32))])
    wide = mctx.merge_csr_parts(4, 5, [(rowptr, col, val)])
    other = S.Context(0)
    try:
        foreign = other.merge_csr_parts(4, 4, [(rowptr, col, val)])
        assert _raw(res, res, None) == (_lib.ERR_ARG, True)
        assert _raw(res, res, _sr(), out=False)[0] == _lib.ERR_ARG
        assert _raw(None, res, _sr()) == (_lib.ERR_ARG, True)
        assert _raw(res, None, _sr()) == (_lib.ERR_ARG, True)
        E = _lib.EWISE_OPS
        for add in (-1, E["times"], E["second"], E["minus"], E["div"], 8, 1 << 20):
            assert _raw(res, res, _sr(add, E["times"])) == (_lib.ERR_ARG, True)
        for mul in (-1, E["minus"], E["div"], 8, 1 << 20):
            assert _raw(res, res, _sr(E["plus"], mul)) == (_lib.ERR_ARG, True)
            assert _lib.lib().osp_last_error_string()
        for word in range(8):
            s = _sr()
            s.reserved[word] = 1
            assert _raw(res, res, s) == (_lib.ERR_ARG, True)
        for bad in (f32, foreign):
            assert _raw(res, bad, _sr()) == (_lib.ERR_ARG, True)
            assert _raw(bad, res, _sr()) == (_lib.ERR_ARG, True)
        assert _raw(wide, res, _sr()) == (_lib.ERR_DIM, True)                      # 4 x 5 times 4 x 4
        # every legal pair is taken, and stats may be null
        for add in model.ADD_OPS:
            for mul in model.MUL_OPS:
                o = ctypes.c_void_p()
                s = _sr(E[add], E[mul])
                assert _lib.lib().osp_csr_mxm(res._h, res._h, ctypes.byref(s), ctypes.byref(o), None) == 0
                S.CsrResult(mctx, o).close()
        # the Python surface: names first, then the context and the dtype, before the call is made
        for call in (lambda: res.mxm(res, "times", "plus"), lambda: res.mxm(res, "plus", "minus"), lambda: res.mxm(res, add=0)):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(TypeError):
            res.mxm(val)
        for bad in (f32, foreign):
            with pytest.raises(S.OspError) as ei:
                res.mxm(bad)
            assert ei.value.status == _lib.ERR_ARG
        with pytest.raises(S.OspError) as ei:
            wide.mxm(res)
        assert ei.value.status == _lib.ERR_DIM
        foreign.close()
    finally:
        other.close()
        for x in (res, f32, wide):
            x.close()


def test_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    ts = [am._dev(x) for x in (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, B.indptr.astype(np.int64),
                               B.indices.astype(np.uint32), B.data)]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    full = mctx.spgemm_csc_csr_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        assert _raw(part, full, _sr()) == (_lib.ERR_ARG, True)
        assert _raw(full, part, _sr()) == (_lib.ERR_ARG, True)
        assert _raw(part, part, _sr()) == (_lib.ERR_ARG, True)
    finally:
        part.close()
        full.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_cases_give_an_empty_result(mctx, dt):
    z = lambda m: np.zeros(m + 1, np.int64)   # noqa: E731
    none_c, none_v = np.zeros(0, np.uint32), np.zeros(0, dt)
    full = (np.array([0, 2, 3, 3], np.int64), np.array([0, 2, 1], np.uint32), np.array([1, 2, 3], dt))       # 3 x 3
    meets_empty = (np.array([0, 1, 2, 2], np.int64), np.array([1, 1], np.uint32), np.array([4, 5], dt))     # points at row 1 only
    b_row1_empty = (np.array([0, 2, 2, 3], np.int64), np.array([0, 1, 2], np.uint32), np.array([1, 2, 3], dt))
    cases = {"empty a": ((z(3), none_c, none_v), 3, full, 3), "empty b": (full, 3, (z(3), none_c, none_v), 3),
             "M == 0": ((z(0), none_c, none_v), 3, full, 3), "every k meets an empty row": (meets_empty, 3, b_row1_empty, 3)}
    for name, (a, ka, b, nb) in cases.items():
        ra, rb = _upload(mctx, ka, a), _upload(mctx, nb, b)
        try:
            for add, mul in (("plus", "times"), ("min", "plus")):
                res, st = ra.mxm(rb, add, mul)
                try:
                    M = len(a[0]) - 1
                    assert res.shape == (M, nb) and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(M + 1, np.int64)), name
                    assert (st["products"], st["nnz_out"], st["short_rows"], st["long_rows"], st["batches"]) == (0, 0, 0, 0, 0), name
                    assert (st["nnz_a"], st["nnz_b"]) == (len(a[1]), len(b[1]))
                    if name != "every k meets an empty row":
                        assert st["launches"] == 0, name
                    nxt, _ = res.mxm(rb) if M else (None, None)      # an empty result is an operand like any other
                    if nxt is not None:
                        assert nxt.nnz == 0
                        nxt.close()
                finally:
                    res.close()
        finally:
            ra.close()
            rb.close()


# ---- composition ------------------------------------------------------------------------------------------------------------------
def test_mxm_results_compose(mctx):
    n, g = _rmat_csr(8, np.float64, seed=6)
    r = _upload(mctx, n, g)
    made = []
    try:
        P, _ = r.mxm(r, "min", "plus")
        made.append(P)
        want = model.mxm(g, g, n, "min", "plus")[0]
        _assert_same(P, want)
        sel, _ = P.select("lt", 1.5)
        made.append(sel)
        keep = want[2] < 1.5
        assert sel.nnz == int(keep.sum()) and np.array_equal(_bits(sel.vals), _bits(want[2][keep]))
        un, _ = P.union(r, "min")
        made.append(un)
        assert un.nnz >= P.nnz
        msk, _ = P.apply_mask(r)
        made.append(msk)
        assert 0 < msk.nnz <= r.nnz
        sums, _ = P.reduce("rows", "count")
        assert np.array_equal(sums, np.diff(want[0]).astype(np.float64))
        again, _ = sel.mxm(P, "max", "min")
        made.append(again)
        selcsr = (np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(want[0]))[keep], minlength=n))]).astype(np.int64),
                  want[1][keep], want[2][keep])
        _assert_same(again, model.mxm(selcsr, want, n, "max", "min")[0])
    finally:
        for x in made:
            x.close()
        r.close()


def test_fifty_back_to_back_calls_give_the_same_arrays_and_the_pool_does_not_grow(operands, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call, and after the first call no call allocates device memory:
    the library's own count of pool misses (hipMalloc calls of the context, printed under OSP_VERBOSE) stays where the first
    call left it.  (Which block a call gets is the pool's business: equal-sized blocks change places.)"""
    import re
    ra, rb = operands[np.float64]
    monkeypatch.setenv("OSP_VERBOSE", "1")
    first, misses = {}, []
    for i in range(50):
        sr = [("plus", "times"), ("min", "plus"), ("max", "min"), ("first", "second"), ("plus", "first")][i % 5]
        capfd.readouterr()
        res, st = ra.mxm(rb, *sr)
        err = capfd.readouterr().err
        got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["nnz_out"], st["products"])
        res.close()
        found = re.findall(r"\[osp\] mxm .*pool misses so far: (\d+) hipMalloc calls", err)
        assert len(found) == 1, err
        misses.append(int(found[0]))
        if sr not in first:
            first[sr] = got
        else:
            assert all(np.array_equal(x, y) for x, y in zip(got, first[sr])), i
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses
