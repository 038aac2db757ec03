"""osp_csr_ewise on the GPU against the numpy model of tests/ewise_model.py: row pointers and columns exact, value BITS equal
(compared as unsigned integers) for every copied value and for MIN, MAX, FIRST and SECOND; for PLUS, TIMES, MINUS and DIV the
bits are equal where the model's result is no NaN, and the result is a NaN where it is (a computed NaN's payload is the
hardware's).  A single correctly rounded IEEE operation has one result: bit equality is the expectation, not a tolerance.
Both modes, every legal op, f32 and f64, both operand orders, on the inputs built for every rule of the mask filter
(tests/test_gpu_apply_mask.py) and on patterns of this op's own; the identities that tie it to the merge and the mask
filter; its errors; chaining; its launches."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import ewise_model as model
from tests import test_gpu_apply_mask as am   # the input builders only

pytestmark = pytest.mark.gpu

DEV = am.DEV
CHUNK = am.CHUNK
_bits, _upload = am._bits, am._upload


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _with_values(pattern, dt, seed):
    """Random values on a (rowptr, col) pattern."""
    rng = np.random.default_rng(seed)
    return pattern[0], pattern[1], rng.standard_normal(len(pattern[1])).astype(dt)


def _rows_of(lists, dt, seed):
    """A CSR from one ascending column array per row."""
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32)
    return _with_values((rowptr, col), dt, seed)


def _traps(dt):
    """The mask filter's trap input as a (rows of 0, 1, 63, 64, 65, 2047, 2048 and 2049 entries, runs of empty rows, chunk
    boundaries between rows and inside one) against b = half of a's coordinates, as many others, and columns below every
    row's first and above its last entry.  The special values sit in a's rows 12 and 17; b gets them, rotated, on every
    entry of those rows, so that they meet on two-sided coordinates and stand alone on one-sided ones."""
    ncol, a, m = am._traps(dt)
    b_ptr, b_col, b_val = _with_values(m, dt, seed=21)
    sp_ = am._special(dt)
    for r in (12, 17):
        k = b_ptr[r + 1] - b_ptr[r]
        b_val[b_ptr[r]:b_ptr[r + 1]] = np.resize(np.roll(sp_, 3 + r), k)
    return ncol, a, (b_ptr, b_col, b_val)


def _from_mask_case(name, seed):
    def build(dt):
        ncol, a, m = am.CASES[name](dt)
        return ncol, a, _with_values(m, dt, seed)
    return build


def _interleaved(dt):
    """Strictly interleaved columns (a the even ones, b the odd ones), rows across several chunks and short ones."""
    lengths = [0, 3 * CHUNK + 7, 1, 64, 0, CHUNK, 65]
    a = _rows_of([2 * np.arange(k) for k in lengths], dt, 31)
    b = _rows_of([2 * np.arange(k) + 1 for k in lengths], dt, 32)
    return 8 * CHUNK, a, b


def _below_above(dt):
    """Per row all of b's columns below all of a's (even rows) or above them (odd rows); row lengths differ per side."""
    la = [5, 2049, 0, 64, CHUNK + 1, 1, 700, 63]
    lb = [2049, 5, 9, 0, 64, CHUNK + 1, 1, 65]
    ncol = 4 * CHUNK
    a_rows, b_rows = [], []
    for i, (ka, kb) in enumerate(zip(la, lb)):
        low, high = np.arange(kb if i % 2 == 0 else ka), 2 * CHUNK + np.arange(ka if i % 2 == 0 else kb)
        a_rows.append(high if i % 2 == 0 else low)
        b_rows.append(low if i % 2 == 0 else high)
    return ncol, _rows_of(a_rows, dt, 33), _rows_of(b_rows, dt, 34)


def _simple(kind):
    def build(dt):
        ncol = 5000
        a = am._csr_from_lengths([0, 40, 3000, 0, 1, 200], ncol, dt, seed=12)
        b = am._csr_from_lengths([7, 0, 2500, 0, 1, 300], ncol, dt, seed=35)
        empty = (np.zeros(len(a[0]), np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))
        none = (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))
        return {"empty_a": (ncol, empty, b), "empty_b": (ncol, a, empty), "both_empty": (ncol, empty, empty),
                "no_rows": (ncol, none, none)}[kind]
    return build


CASES = {"traps": _traps, "frontier": _from_mask_case("frontier", 22), "short_rows": _from_mask_case("short_rows", 23),
         "same_pattern": _from_mask_case("same_pattern", 24), "disjoint": _from_mask_case("disjoint", 25),
         "interleaved": _interleaved, "below_above": _below_above}
CASES.update({k: _simple(k) for k in ("empty_a", "empty_b", "both_empty", "no_rows")})


def _legal(mode):
    return model.UNION_OPS if mode == "union" else model.OPS


def _assert_values(got, want, computed, op):
    """Bits equal; for the four arithmetic ops a computed NaN is a NaN, whatever its payload."""
    gb, wb = _bits(got), _bits(want)
    if op in model.COPY_OPS:
        assert np.array_equal(gb, wb)
        return
    nan = computed & np.isnan(want)
    assert np.array_equal(gb[~nan], wb[~nan])
    assert np.isnan(got[nan]).all()


def _check(res, st, plan, mode, op):
    want_ptr, want_col, want_val, computed = plan.result(mode, op)
    assert res.shape == (plan.M, plan.ncol) and res.dtype == plan.a_val.dtype.type
    assert res.nnz == len(want_col) == res.info["nnz_c"]
    assert np.array_equal(res.rowptr, want_ptr)
    assert np.array_equal(res.colidx, want_col)
    _assert_values(res.vals, want_val, computed, op)
    nnz_a, nnz_b = len(plan.a_col), len(plan.b_col)
    assert (st["nnz_a"], st["nnz_b"], st["nnz_both"], st["nnz_out"]) == (nnz_a, nnz_b, plan.nnz_both, len(want_col))
    assert st["ms_total"] >= 0 and (st["launches"] > 0) == (nnz_a > 0 and nnz_b > 0)
    return len(want_col)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_ewise_equals_model(mctx, case, dt):
    ncol, a, b = CASES[case](dt)
    ra, rb = _upload(mctx, ncol, a), _upload(mctx, ncol, b)
    try:
        for (x, y), (rx, ry) in (((a, b), (ra, rb)), ((b, a), (rb, ra))):
            plan = model.Plan(x, y, ncol)
            nnz = {}
            for mode in model.MODES:
                for op in _legal(mode):
                    res, st = rx.ewise(ry, mode, op)
                    try:
                        nnz[mode] = _check(res, st, plan, mode, op)
                    finally:
                        res.close()
            assert nnz["union"] + nnz["intersect"] == len(x[1]) + len(y[1])
            if case in ("traps", "frontier", "short_rows"):     # the patterns overlap in part
                assert 0.2 * len(a[1]) < nnz["intersect"] < 0.8 * len(a[1])
            if case in ("disjoint", "interleaved", "below_above"):
                assert nnz["intersect"] == 0 and nnz["union"] > 0
            if case == "same_pattern":
                assert nnz["intersect"] == nnz["union"] == len(x[1]) > 0
        # the operands stay valid and untouched
        for r, t in ((ra, a), (rb, b)):
            r._host = None   # (read it again)
            rp, c, v = r.to_host()
            assert np.array_equal(rp, t[0]) and np.array_equal(c, t[1]) and np.array_equal(_bits(v), _bits(t[2]))
    finally:
        ra.close()
        rb.close()


def test_the_trap_input_meets_every_rule():
    for dt in (np.float32, np.float64):
        ncol, a, b = _traps(dt)
        assert {0, 1, 63, 64, 65, 2047, 2048, 2049} <= set(np.diff(a[0]).tolist())
        starts = a[0][:-1][np.diff(a[0]) > 0]
        assert np.any((starts % CHUNK == 0) & (starts > 0))                                            # a boundary between rows
        for x in (a, b):                                                                               # and inside a row
            assert np.any((x[0][:-1] // CHUNK < (x[0][1:] - 1) // CHUNK) & (np.diff(x[0]) > 0))
            assert np.any((np.diff(x[0])[:-1] == 0) & (np.diff(x[0])[1:] == 0)) or x is b             # a run of empty rows
            assert np.isnan(x[2]).any() and np.isinf(x[2]).any()
        # b's chunks are cut elsewhere than a's: its row starts differ from a's from the third row on
        assert np.all(a[0][3:] != b[0][3:])


def test_special_values_meet_in_every_combination(mctx):
    """Every special value against every special value on two-sided coordinates, and each alone on a one-sided one."""
    for dt in (np.float32, np.float64):
        sp_ = am._special(dt)
        k = len(sp_)
        # row 0: the k x k pairs; row 1: a alone; row 2: b alone
        a = (np.array([0, k * k, k * k + k, k * k + k], np.int64),
             np.concatenate([np.arange(k * k), 2 * np.arange(k)]).astype(np.uint32), np.concatenate([np.repeat(sp_, k), sp_]))
        b = (np.array([0, k * k, k * k, k * k + k], np.int64),
             np.concatenate([np.arange(k * k), 3 * np.arange(k)]).astype(np.uint32), np.concatenate([np.tile(sp_, k), sp_]))
        ra, rb = _upload(mctx, 1024, a), _upload(mctx, 1024, b)
        plan = model.Plan(a, b, 1024)
        assert plan.nnz_both == k * k
        try:
            for mode in model.MODES:
                for op in _legal(mode):
                    res, st = ra.ewise(rb, mode, op)
                    try:
                        _check(res, st, plan, mode, op)
                    finally:
                        res.close()
            # denormals are kept, not flushed: the smallest denormal plus itself is twice it
            res, _ = ra.ewise(ra, "intersect", "plus")
            tiny = _bits(res.vals)[6 * k + 6]        # (the pair (sp_[6], sp_[6]): bits 1)
            assert _bits(a[2])[6 * k + 6] == 1 and tiny == 2
            res.close()
        finally:
            ra.close()
            rb.close()


def test_an_operand_with_itself(mctx):
    for dt in (np.float32, np.float64):
        ncol, a, _ = _traps(dt)
        ra = _upload(mctx, ncol, a)
        plan = model.Plan(a, a, ncol)
        try:
            for mode in model.MODES:
                for op in _legal(mode):
                    res, st = ra.ewise(ra, mode, op)
                    try:
                        assert _check(res, st, plan, mode, op) == len(a[1]) == st["nnz_both"]
                    finally:
                        res.close()
        finally:
            ra.close()


# ---- identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_union_first_of_disjoint_parts_is_their_merge(mctx, dt):
    """The visited set plus the new frontier of a traversal: what graph.bfs_levels relies on."""
    for name in ("interleaved", "below_above", "disjoint"):
        ncol, a, b = CASES[name](dt)
        ra, rb = _upload(mctx, ncol, a), _upload(mctx, ncol, b)
        try:
            u, st = ra.ewise(rb, "union", "first")
            m = mctx.merge_csr_parts_device(dt, len(a[0]) - 1, ncol, [ra.device_ptrs(), rb.device_ptrs()])
            try:
                assert st["nnz_both"] == 0 and u.nnz == m.nnz == len(a[1]) + len(b[1])
                assert np.array_equal(u.rowptr, m.rowptr) and np.array_equal(u.colidx, m.colidx)
                assert np.array_equal(_bits(u.vals), _bits(m.vals))
            finally:
                u.close()
                m.close()
        finally:
            ra.close()
            rb.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_intersect_first_is_the_mask_filter(mctx, dt):
    for name in ("traps", "short_rows"):
        ncol, a, b = CASES[name](dt)
        ra, rb = _upload(mctx, ncol, a), _upload(mctx, ncol, b)
        try:
            i, st = ra.ewise(rb, "intersect", "first")
            f, fs = ra.apply_mask(rb)
            u, us = ra.ewise(rb, "union", "second")
            try:
                assert 0 < i.nnz == f.nnz == st["nnz_both"] == fs["nnz_out"]
                assert np.array_equal(i.rowptr, f.rowptr) and np.array_equal(i.colidx, f.colidx)
                assert np.array_equal(_bits(i.vals), _bits(f.vals))
                assert us["nnz_out"] + st["nnz_out"] == len(a[1]) + len(b[1]) and us["nnz_both"] == st["nnz_both"]
            finally:
                for x in (i, f, u):
                    x.close()
        finally:
            ra.close()
            rb.close()


# ---- error paths ------------------------------------------------------------------------------------------------------------
def _raw(a, b, ew, out=True):
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    stats = _lib.EwiseStats()
    stats.nnz_a = 77
    h = lambda r: r._h if r is not None else None   # noqa: E731
    st = _lib.lib().osp_csr_ewise(h(a), h(b), ctypes.byref(ew) if ew is not None else None, ctypes.byref(o) if out else None,
                                  ctypes.byref(stats))
    return st, o.value == sentinel and stats.nnz_a == 77


def _ew(mode=0, op=0):
    e = _lib.Ewise()
    e.mode, e.op = mode, op
    return e


def test_argument_errors(mctx):
    res = am._small_result(mctx)
    rowptr = np.array([0, 2, 3], np.int64)
    col, val = np.array([0, 3, 1], np.uint32), np.array([1.0, 2.0, 3.0])
    f32 = mctx.merge_csr_parts(2, 4, [(rowptr, col, val.astype(np.float32))])
    wide = mctx.merge_csr_parts(2, 5, [(rowptr, col, val)])
    tall = mctx.merge_csr_parts(3, 4, [(np.array([0, 2, 3, 3], np.int64), col, val)])
    other = S.Context(0)
    try:
        foreign = other.merge_csr_parts(2, 4, [(rowptr, col, val)])
        assert _raw(res, res, None) == (_lib.ERR_ARG, True)                       # null ew
        assert _raw(res, res, _ew(), out=False)[0] == _lib.ERR_ARG                # null out
        assert _raw(None, res, _ew()) == (_lib.ERR_ARG, True)                     # null a
        assert _raw(res, None, _ew()) == (_lib.ERR_ARG, True)                     # null b
        for mode in (-1, 2, 1 << 20):                                             # a mode outside the enum
            assert _raw(res, res, _ew(mode, 0)) == (_lib.ERR_ARG, True)
        for op in (-1, 8, 1 << 20):                                               # an op outside the enum
            for mode in (0, 1):
                assert _raw(res, res, _ew(mode, op)) == (_lib.ERR_ARG, True)
                assert _lib.lib().osp_last_error_string()
        for op in (_lib.EWISE_OPS["minus"], _lib.EWISE_OPS["div"]):               # a union has no minus and no div
            assert _raw(res, res, _ew(0, op)) == (_lib.ERR_ARG, True)
        for word in range(8):                                                     # a reserved word that is not 0
            e = _ew(1, 1)
            e.reserved[word] = 1
            assert _raw(res, res, e) == (_lib.ERR_ARG, True)
        for bad in (f32, wide, tall, foreign):                                    # dtype, N, M, context: on either side
            assert _raw(res, bad, _ew()) == (_lib.ERR_ARG, True)
            assert _raw(bad, res, _ew(1, 1)) == (_lib.ERR_ARG, True)
        # every legal pair is taken, and stats may be null
        for mode in (0, 1):
            for op in range(6 if mode == 0 else 8):
                o = ctypes.c_void_p()
                e = _ew(mode, op)
                assert _lib.lib().osp_csr_ewise(res._h, res._h, ctypes.byref(e), ctypes.byref(o), None) == 0
                S.CsrResult(mctx, o).close()
        # the Python surface: names are checked first, then shape and dtype as apply_mask does
        for call in (lambda: res.ewise(res, "both", "plus"), lambda: res.ewise(res, "union", "pow"), lambda: res.union(res, op=0)):
            with pytest.raises(ValueError):
                call()
        for bad in (f32, wide, tall):
            with pytest.raises(S.OspError) as ei:
                res.intersect(bad)
            assert ei.value.status == _lib.ERR_ARG
        with pytest.raises(S.OspError) as ei:
            res.union(foreign)
        assert ei.value.status == _lib.ERR_ARG
        with pytest.raises(S.OspError) as ei:
            res.union(res, "minus")
        assert ei.value.status == _lib.ERR_ARG
        foreign.close()
    finally:
        other.close()
        for x in (res, f32, wide, tall):
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
        assert _raw(part, full, _ew()) == (_lib.ERR_ARG, True)
        assert _raw(full, part, _ew(1, 1)) == (_lib.ERR_ARG, True)
        assert _raw(part, part, _ew()) == (_lib.ERR_ARG, True)
    finally:
        part.close()
        full.close()


# ---- composition --------------------------------------------------------------------------------------------------------------
def _host(res):
    return res.rowptr.copy(), res.colidx.copy(), res.vals.copy()


def test_ewise_result_composes(mctx):
    from tests import bfs_model, truss_model
    ncol = 3000
    a = am._csr_from_lengths([5, 0, 700, 2500, 64], ncol, np.float64, seed=41)
    b = am._csr_from_lengths([0, 9, 900, 2100, 64], ncol, np.float64, seed=43)
    c = am._csr_from_lengths([1, 1, 100, 2700, 0], ncol, np.float64, seed=44)
    ra, rb, rc = (_upload(mctx, ncol, t) for t in (a, b, c))
    made = []
    try:
        # of a product's result with itself and its thinning: into select, apply_mask and ewise again
        u, st = ra.union(rb)
        made.append(u)
        wu = model.ewise(a, b, ncol, "union", "plus")
        _check(u, st, model.Plan(a, b, ncol), "union", "plus")
        s, _ = u.select("gt", 0.0)
        made.append(s)
        ws = truss_model.select(*wu, "gt", 0.0)
        assert np.array_equal(s.rowptr, ws[0]) and np.array_equal(s.colidx, ws[1]) and np.array_equal(_bits(s.vals), _bits(ws[2]))
        m, _ = u.apply_mask(rc, complement=True)
        made.append(m)
        wm = bfs_model.apply_mask(*wu, c[0], c[1], ncol, True)
        assert np.array_equal(m.rowptr, wm[0]) and np.array_equal(m.colidx, wm[1]) and np.array_equal(_bits(m.vals), _bits(wm[2]))
        i, st = u.intersect(rc, "div")
        made.append(i)
        _check(i, st, model.Plan(wu, c, ncol), "intersect", "div")
        uu, st = s.ewise(i, "union", "max")
        made.append(uu)
        _check(uu, st, model.Plan(ws, _host(i), ncol), "union", "max")
        assert 0 < i.nnz < u.nnz and 0 < s.nnz < u.nnz and 0 < m.nnz < u.nnz and uu.nnz >= s.nnz
        # of a select and of an apply_mask
        sa, _ = ra.select("lt", 0.5)
        ma, _ = rb.apply_mask(rc)
        made += [sa, ma]
        x, st = sa.ewise(ma, "union", "min")
        made.append(x)
        _check(x, st, model.Plan(_host(sa), _host(ma), ncol), "union", "min")
        # the other entry points of a result
        rows = torch.empty(u.nnz, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(DEV)
        u.coo_rows_into(rows.data_ptr())
        assert np.array_equal(rows.cpu().numpy(), np.repeat(np.arange(len(a[0]) - 1), np.diff(u.rowptr)))
        assert u.to_scipy().nnz == u.nnz
        # info is a's with nnz_c and ms_total replaced
        for k, v in ra.info.items():
            if k not in ("nnz_c", "ms_total"):
                assert u.info[k] == v, k
    finally:
        for x in made + [ra, rb, rc]:
            x.close()


def test_ewise_of_a_product(ctx):
    """A self-product against its every-second-entry thinning: the shape of tools/time_ewise.py, small."""
    n, r, c, v = gen.rmat_coo(9, 8, "uniform", seed=5)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    prod = ctx.spgemm_csc_csr(n, n, n, A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data,
                              B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data)
    p = _host(prod)
    thin = ((p[0] + 1) // 2, p[1][::2].copy(), p[2][::2] * 3.0)
    rt = _upload(ctx, n, thin)
    plan = model.Plan(p, thin, n)
    try:
        for mode, op in (("union", "plus"), ("intersect", "times"), ("union", "first"), ("intersect", "minus")):
            res, st = prod.ewise(rt, mode, op)
            try:
                _check(res, st, plan, mode, op)
                assert st["nnz_both"] == len(thin[1]) > 0
            finally:
                res.close()
    finally:
        prod.close()
        rt.close()


def test_fifty_back_to_back_calls_give_the_same_arrays(mctx):
    """Recycled pool buffers carry nothing over from call to call."""
    ncol, a, b = _traps(np.float32)
    ra, rb = _upload(mctx, ncol, a), _upload(mctx, ncol, b)
    plan = model.Plan(a, b, ncol)
    variants = [("union", "plus"), ("intersect", "times"), ("union", "first"), ("intersect", "second"), ("union", "max")]
    try:
        first = {}
        for i in range(50):
            mode, op = variants[i % len(variants)]
            res, st = ra.ewise(rb, mode, op)
            got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["nnz_out"])
            if (mode, op) not in first:
                first[(mode, op)] = got
                _check(res, st, plan, mode, op)
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, first[(mode, op)])), i
            res.close()
        ra._host = None
        assert np.array_equal(_bits(ra.to_host()[2]), _bits(a[2]))
    finally:
        ra.close()
        rb.close()


@functools.lru_cache(maxsize=None)
def _launch_pairs():
    """(ncol, big, small, kernels of the scan): ``big`` has the most entries the one-kernel scan takes, or one more; ``small``
    holds ten coordinates, five of them big's."""
    out = []
    for nnz, scan in ((am.SCAN_SMALL_MAX, 1), (am.SCAN_SMALL_MAX + 1, 3)):
        ncol = 1 << 22
        big = (np.array([0, nnz - 5, nnz], np.int64), np.concatenate([2 * np.arange(nnz - 5), np.arange(5)]).astype(np.uint32),
               np.ones(nnz, np.float32))
        small = (np.array([0, 10, 10], np.int64), np.arange(10, dtype=np.uint32) * 3 + 3, np.full(10, 2.0, np.float32))
        out.append((ncol, big, small, scan))
    return tuple(out)


def test_ewise_reports_its_launches(mctx):
    """Union: the flag over b, the scan, the row pointer, a's side and -- when b has entries of its own -- b's side.
    Intersect: the flag over a, the scan, the row pointer and -- when anything is common -- the write.  am.SCAN_SMALL_MAX is
    where the scan of the flagged operand's words takes three kernels instead of one."""
    for ncol, big, small, scan in _launch_pairs():
        rbig, rsmall = _upload(mctx, ncol, big), _upload(mctx, ncol, small)
        plan = model.Plan(small, big, ncol)
        assert plan.nnz_both == 5
        try:
            for a, b, mode, op, want in ((rsmall, rbig, "union", "plus", 1 + scan + 1 + 1 + 1),      # the flag runs over big
                                         (rbig, rsmall, "union", "plus", 1 + 1 + 1 + 1 + 1),         # over small
                                         (rbig, rbig, "union", "first", 1 + scan + 1 + 1),            # b has nothing of its own
                                         (rbig, rsmall, "intersect", "times", 1 + scan + 1 + 1),
                                         (rsmall, rbig, "intersect", "times", 1 + 1 + 1 + 1)):
                res, st = a.ewise(b, mode, op)
                try:
                    assert st["nnz_out"] == res.nnz
                    assert st["launches"] == want, (len(big[1]), mode, st["launches"], want)
                finally:
                    res.close()
            res, st = rsmall.ewise(rbig, "union", "plus")
            try:
                _check(res, st, plan, "union", "plus")
            finally:
                res.close()
        finally:
            rbig.close()
            rsmall.close()
    # nothing in common: no write kernel; an empty operand: no kernel at all
    ncol, a, b = _interleaved(np.float32)
    ra, rb = _upload(mctx, ncol, a), _upload(mctx, ncol, b)
    try:
        res, st = ra.ewise(rb, "intersect", "plus")
        assert st["launches"] == 1 + 1 + 1 and res.nnz == 0
        res.close()
    finally:
        ra.close()
        rb.close()
    ncol, a, b = _simple("empty_b")(np.float32)
    ra, rb = _upload(mctx, ncol, a), _upload(mctx, ncol, b)
    try:
        for x, y, mode, nnz in ((ra, rb, "union", len(a[1])), (rb, ra, "union", len(a[1])), (ra, rb, "intersect", 0), (rb, rb, "union", 0)):
            res, st = x.ewise(y, mode, "plus")
            assert st["launches"] == 0 and res.nnz == nnz == st["nnz_out"]
            res.close()
    finally:
        ra.close()
        rb.close()
