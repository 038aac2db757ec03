"""osp_csr_apply_mask on the GPU against the numpy model of tests/bfs_model.py: row pointers and columns exact, value BITS
equal (compared as unsigned integers), both senses, f32 and f64, host and device masks, on inputs built for every rule of
the filter, on a product's result, against the masked product, through the result's other entry points, and its errors."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import bfs_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_compact.h")).read()
# the filter's unit of work: kCompactThreads * kCompactRounds consecutive entries of `in`
CHUNK = int(re.search(r"kCompactThreads\s*=\s*(\d+)", _SRC).group(1)) * int(re.search(r"kCompactRounds\s*=\s*(\d+)", _SRC).group(1))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _dev(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(DEV) if x.size else torch.empty(1, dtype=torch.from_numpy(x[:0]).dtype, device=DEV)


def _special(dt):
    """NaNs with payloads (a quiet and a signalling one), infinities, both zeros, denormals, the largest number and 1."""
    if dt == np.float32:
        return np.array([0x7fc00123, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0, 1, 0x80000001, 0x00400000, 0x7f7fffff,
                         0x3f800000], np.uint32).view(np.float32)
    return np.array([0x7ff8000000abcdef, 0xfff4000000000001, 0x7ff0000000000000, 0xfff0000000000000, 0x8000000000000000, 0, 1,
                     0x8000000000000001, 0x0008000000000000, 0x7fefffffffffffff, 0x3ff0000000000000], np.uint64).view(np.float64)


def _csr_from_lengths(lengths, ncol, dt, seed, lo=100):
    """Rows of the given lengths with random ascending columns in [lo, ncol - lo) and random values."""
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cols = [np.sort(rng.choice(ncol - 2 * lo, size=int(k), replace=False)).astype(np.uint32) + np.uint32(lo) for k in lengths]
    col = np.concatenate(cols) if cols else np.zeros(0, np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    return rowptr, col, val


def _mask_for(rowptr, col, ncol, seed, share=0.5, extra=0.5, edges=True):
    """Per row: a random `share` of the row's own columns, `extra` times the row's length of other columns, and (edges)
    columns below the row's first and above its last entry."""
    rng = np.random.default_rng(seed)
    M = len(rowptr) - 1
    row = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr))
    key = row * ncol + col.astype(np.int64)
    own = key[rng.random(len(key)) < share]
    other = rng.integers(0, M, int(extra * len(key))) * ncol + rng.integers(0, ncol, int(extra * len(key))) if M else np.zeros(0, np.int64)
    parts = [own, other]
    if edges and M:
        r = np.arange(M, dtype=np.int64)
        parts += [r * ncol + c for c in (0, 1, 3, ncol - 1)]
    mkey = np.unique(np.concatenate(parts))
    m_rowptr = np.zeros(M + 1, np.int64)
    m_rowptr[1:] = np.cumsum(np.bincount(mkey // ncol, minlength=M))
    return m_rowptr, (mkey % ncol).astype(np.uint32)


def _traps(dt):
    ncol = 1 << 16
    lengths = [0, 0, 1, 63, 64, 65, 0, 0, 0, 2047, 2048, 2049, 11, 5, 0, 700]
    lengths.append(CHUNK - sum(lengths) % CHUNK)   # the next row begins ON a chunk boundary
    lengths += [3000, 17, 0, 4 * CHUNK, 1, 0, 0]     # boundaries inside a row; the last rows are empty
    rowptr, col, val = _csr_from_lengths(lengths, ncol, dt, seed=3)
    sp_ = _special(dt)
    val[rowptr[12]:rowptr[12] + 11] = sp_          # the row of 11 entries holds the special values
    val[rowptr[17]:rowptr[17] + 22] = np.concatenate([sp_, sp_])
    starts = rowptr[:-1][np.diff(rowptr) > 0]
    assert np.any((starts % CHUNK == 0) & (starts > 0))                                    # a boundary between rows
    assert np.any((rowptr[:-1] // CHUNK < (rowptr[1:] - 1) // CHUNK) & (np.diff(rowptr) > 0))   # and one inside a row
    m_rowptr, m_col = _mask_for(rowptr, col, ncol, seed=4)
    return ncol, (rowptr, col, val), (m_rowptr, m_col)


def _frontier(dt):
    """ONE row of 2^20 entries against a mask row of 2^20 - 1: the shape of a BFS level."""
    ncol = 1 << 21
    rowptr, col, val = _csr_from_lengths([1 << 20], ncol, dt, seed=5, lo=0)
    rng = np.random.default_rng(6)
    m_col = np.sort(rng.choice(ncol, size=(1 << 20) - 1, replace=False)).astype(np.uint32)
    return ncol, (rowptr, col, val), (np.array([0, len(m_col)], np.int64), m_col)


def _short_rows(dt):
    """2^18 rows of at most 4 entries."""
    ncol = 1 << 12
    rng = np.random.default_rng(8)
    rowptr, col, val = _csr_from_lengths(rng.integers(0, 5, 1 << 18), ncol, dt, seed=9, lo=0)
    return ncol, (rowptr, col, val), _mask_for(rowptr, col, ncol, seed=10, edges=False)


def _simple(kind):
    def build(dt):
        ncol = 5000
        rowptr, col, val = _csr_from_lengths([0, 40, 3000, 0, 1, 200], ncol, dt, seed=12)
        empty = (np.zeros(len(rowptr), np.int64), np.zeros(0, np.uint32))
        if kind == "empty_in":
            m = _mask_for(rowptr, col, ncol, seed=13)
            return ncol, (np.zeros(len(rowptr), np.int64), np.zeros(0, np.uint32), np.zeros(0, dt)), m
        if kind == "empty_mask":
            return ncol, (rowptr, col, val), empty
        if kind == "same_pattern":
            return ncol, (rowptr, col, val), (rowptr.copy(), col.copy())
        if kind == "disjoint":
            return ncol, (rowptr, col, val), _mask_for(rowptr, col, ncol, seed=14, share=0.0, extra=0.0)
        if kind == "no_rows":
            return ncol, (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt)), (np.zeros(1, np.int64), np.zeros(0, np.uint32))
        raise KeyError(kind)
    return build


CASES = {"traps": _traps, "frontier": _frontier, "short_rows": _short_rows}
CASES.update({k: _simple(k) for k in ("empty_in", "empty_mask", "same_pattern", "disjoint", "no_rows")})


def _upload(mctx, ncol, csr):
    """The CSR as a library result: the merge of ONE part is the part itself, bit for bit."""
    rowptr, col, val = csr
    src = mctx.merge_csr_parts(len(rowptr) - 1, ncol, [csr])
    assert np.array_equal(src.rowptr, rowptr) and np.array_equal(src.colidx, col) and np.array_equal(_bits(src.vals), _bits(val))
    return src


def _check(res, st, ncol, csr, mask, complement):
    want_ptr, want_col, want_val = model.apply_mask(*csr, *mask, ncol, complement)
    assert res.shape == (len(csr[0]) - 1, ncol) and res.dtype == csr[2].dtype.type
    assert res.nnz == len(want_col) == res.info["nnz_c"]
    assert np.array_equal(res.rowptr, want_ptr)
    assert np.array_equal(res.colidx, want_col)
    assert np.array_equal(_bits(res.vals), _bits(want_val))
    assert (st["nnz_in"], st["nnz_mask"], st["nnz_out"]) == (len(csr[1]), len(mask[1]), len(want_col))
    assert st["ms_total"] >= 0
    return len(want_col)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_apply_mask_equals_model_bit_for_bit(mctx, case, dt):
    ncol, csr, mask = CASES[case](dt)
    src = _upload(mctx, ncol, csr)
    dmask = [_dev(mask[0]), _dev(mask[1])]
    torch.cuda.synchronize(DEV)
    kept = {}
    try:
        for complement in (False, True):
            for space in ("host", "device"):
                m = mask if space == "host" else (dmask[0].data_ptr(), dmask[1].data_ptr())
                res, st = src.apply_mask(m, complement=complement, space=space)
                try:
                    kept[complement] = _check(res, st, ncol, csr, mask, complement)
                finally:
                    res.close()
        # `in` stays valid and untouched
        assert np.array_equal(_bits(src.to_host()[2]), _bits(csr[2]))
    finally:
        src.close()
    nnz = len(csr[1])
    assert kept[False] + kept[True] == nnz
    if case in ("traps", "frontier", "short_rows"):     # both senses keep and remove something
        assert 0.2 * nnz < kept[False] < 0.8 * nnz
    if case == "same_pattern":
        assert kept[False] == nnz and kept[True] == 0
    if case in ("disjoint", "empty_mask"):
        assert kept[False] == 0 and kept[True] == nnz


def test_special_values_are_in_the_trap_input():
    for dt in (np.float32, np.float64):
        _, (rowptr, col, val), _ = _traps(dt)
        assert np.isnan(val).sum() == 6 and np.isinf(val).sum() == 6 and np.any(np.signbit(val) & (val == 0))
        assert np.any((val != 0) & (np.abs(val) < np.finfo(dt).tiny))


def test_mask_given_as_a_result(mctx):
    ncol, csr, mask = _traps(np.float64)
    src = _upload(mctx, ncol, csr)
    msk = mctx.merge_csr_parts(len(mask[0]) - 1, ncol, [(mask[0], mask[1], np.ones(len(mask[1])))])
    try:
        for complement in (False, True):
            res, st = src.apply_mask(msk, complement=complement, validate=True)
            _check(res, st, ncol, csr, mask, complement)
            res.close()
    finally:
        src.close()
        msk.close()


def test_senses_partition_a_product(mctx):
    """keep ∪ complement = in and keep ∩ complement = ∅ on an R-MAT self-product, each side 20-80 % of it."""
    n, r, c, v = gen.rmat_coo(14, 8, "g500", seed=2)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    prod = mctx.spgemm_csc_csr(n, n, n, A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data,
                               B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data)
    try:
        rowptr, col, val = prod.to_host()
        mask = _mask_for(rowptr, col, n, seed=21, share=0.5, extra=0.25, edges=False)
        keep, _ = prod.apply_mask(mask, space="host", validate=True)
        comp, _ = prod.apply_mask(mask, complement=True, space="host")
        try:
            assert 0.2 * prod.nnz <= keep.nnz <= 0.8 * prod.nnz and 0.2 * prod.nnz <= comp.nnz <= 0.8 * prod.nnz
            assert keep.nnz + comp.nnz == prod.nnz
            row = lambda rp: np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
            kk = row(keep.rowptr) * n + keep.colidx
            ck = row(comp.rowptr) * n + comp.colidx
            assert len(np.intersect1d(kk, ck, assume_unique=True)) == 0
            allk = np.concatenate([kk, ck])
            order = np.argsort(allk, kind="stable")
            assert np.array_equal(allk[order], row(rowptr) * n + col)
            assert np.array_equal(np.concatenate([_bits(keep.vals), _bits(comp.vals)])[order], _bits(val))
            # the union on the device is the product again
            back = mctx.merge_csr_parts_device(np.float64, n, n, [keep.device_ptrs(), comp.device_ptrs()])
            assert np.array_equal(back.rowptr, rowptr) and np.array_equal(back.colidx, col) and np.array_equal(_bits(back.vals), _bits(val))
            back.close()
        finally:
            keep.close()
            comp.close()
    finally:
        prod.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_filtered_product_equals_masked_product(ctx, dt):
    """DESIGN.md section 9 defines the masked product as the product with the entries outside the mask removed."""
    for (M, K, N, a, b) in _product_operands(dt):
        full = ctx.spgemm_csc_csr(M, K, N, *a, *b)
        try:
            thin = (full.rowptr.copy(), full.colidx.copy())
            masks = [_mask_for(full.rowptr, full.colidx, N, seed=31, edges=False), thin,
                     (np.zeros(M + 1, np.int64), np.zeros(0, np.uint32))]
            for m_rowptr, m_col in masks:
                want = ctx.spgemm_masked(M, K, N, *a, *b, m_rowptr, m_col)
                got, _ = full.apply_mask((m_rowptr, m_col), space="host")
                try:
                    assert np.array_equal(got.rowptr, want.rowptr)
                    assert np.array_equal(got.colidx, want.colidx)
                    assert np.array_equal(_bits(got.vals), _bits(want.vals))
                finally:
                    want.close()
                    got.close()
            assert 0 < len(masks[0][1]) and full.nnz > 0
        finally:
            full.close()


def _product_operands(dt):
    def csc(M, K, r, c, v):
        A = sp.csc_matrix((v, (r, c)), shape=(M, K)); A.sort_indices()
        return A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data
    def csr(K, N, r, c, v):
        B = sp.csr_matrix((v, (r, c)), shape=(K, N)); B.sort_indices()
        return B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data
    M, K, N = 150, 90, 170
    ar, ac, av = gen.random_coo(M, K, 0.05, seed=11, dtype=dt)
    br, bc, bv = gen.random_coo(K, N, 0.06, seed=12, dtype=dt)
    yield M, K, N, csc(M, K, ar, ac, (av - dt(0.5)).astype(dt)), csr(K, N, br, bc, (bv - dt(0.5)).astype(dt))
    n, r, c, v = gen.rmat_coo(10, 8, "g500", seed=4, dtype=dt)
    yield n, n, n, csc(n, n, r, c, v), csr(n, n, c, r, v)


# ---- error paths ------------------------------------------------------------------------------------------------------------
def _small_result(mctx):
    rowptr = np.array([0, 2, 3], np.int64)
    return mctx.merge_csr_parts(2, 4, [(rowptr, np.array([0, 3, 1], np.uint32), np.array([1.0, 2.0, 3.0]))])


def _raw(res, M, N, m_rowptr, m_col, space=_lib.OSP_HOST, complement=0, validate=1, out=True):
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    stats = _lib.ApplyMaskStats()
    stats.nnz_in = 77
    rp = None if m_rowptr is None else ctypes.c_void_p(m_rowptr.ctypes.data)
    ci = None if m_col is None else ctypes.c_void_p(m_col.ctypes.data)
    st = _lib.lib().osp_csr_apply_mask(res._h, M, N, rp, ci, space, complement, validate, ctypes.byref(o) if out else None,
                                       ctypes.byref(stats))
    return st, o.value == sentinel and stats.nnz_in == 77


_BAD_MASKS = {
    "unsorted": (np.array([0, 2, 3], np.int64), np.array([3, 1, 0], np.uint32), _lib.ERR_UNSORTED),
    "duplicate": (np.array([0, 2, 3], np.int64), np.array([1, 1, 0], np.uint32), _lib.ERR_DUPLICATE),
    "out_of_range": (np.array([0, 2, 3], np.int64), np.array([1, 4, 0], np.uint32), _lib.ERR_RANGE),
    "non_monotone_rowptr": (np.array([0, 3, 2], np.int64), np.array([0, 1, 2], np.uint32), _lib.ERR_ARG),
    "rowptr_not_from_zero": (np.array([1, 2, 3], np.int64), np.array([0, 1, 2], np.uint32), _lib.ERR_ARG),
}


@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("case", sorted(_BAD_MASKS))
def test_bad_mask_statuses(mctx, case, space):
    m_rowptr, m_col, want = _BAD_MASKS[case]
    res = _small_result(mctx)
    try:
        for complement in (0, 1):
            if space == "host":
                st, untouched = _raw(res, 2, 4, m_rowptr, m_col, complement=complement)
            else:
                d = [_dev(m_rowptr), _dev(m_col)]
                torch.cuda.synchronize(DEV)
                sentinel = 0x1234
                o = ctypes.c_void_p(sentinel)
                st = _lib.lib().osp_csr_apply_mask(res._h, 2, 4, ctypes.c_void_p(d[0].data_ptr()), ctypes.c_void_p(d[1].data_ptr()),
                                                   _lib.OSP_DEVICE, complement, 1, ctypes.byref(o), None)
                untouched = o.value == sentinel
            assert st == want, (case, st, _lib.lib().osp_last_error_string())
            assert untouched and _lib.lib().osp_last_error_string()
        if space == "host":
            with pytest.raises(S.OspError) as ei:
                res.apply_mask((m_rowptr, m_col), validate=True, space="host")
            assert ei.value.status == want
    finally:
        res.close()


def test_argument_errors(mctx):
    res = _small_result(mctx)
    good = (np.array([0, 1, 2], np.int64), np.array([3, 1], np.uint32))
    try:
        for M, N in ((3, 4), (2, 5), (1, 4), (2, 3)):                    # shape mismatch
            assert _raw(res, M, N, np.array([0, 1, 2, 2], np.int64), good[1]) == (_lib.ERR_ARG, True)
        assert _raw(res, 2, 4, None, good[1]) == (_lib.ERR_ARG, True)                       # null row pointers
        assert _raw(res, 2, 4, good[0], None, validate=0) == (_lib.ERR_ARG, True)           # null columns, nnzM > 0 (host)
        assert _raw(res, 2, 4, good[0], good[1], out=False)[0] == _lib.ERR_ARG              # null out
        assert _raw(res, 2, 4, good[0], good[1], space=7) == (_lib.ERR_ARG, True)           # bad space
        d = _dev(good[0])
        torch.cuda.synchronize(DEV)
        o = ctypes.c_void_p(0x1234)
        st = _lib.lib().osp_csr_apply_mask(res._h, 2, 4, ctypes.c_void_p(d.data_ptr()), None, _lib.OSP_DEVICE, 1, 0, ctypes.byref(o), None)
        assert st == _lib.ERR_ARG and o.value == 0x1234                                     # null columns, nnzM > 0 (device)
        # a null column array with an EMPTY mask is legal, and stats may be null
        z = np.zeros(3, np.int64)
        o = ctypes.c_void_p()
        assert _lib.lib().osp_csr_apply_mask(res._h, 2, 4, ctypes.c_void_p(z.ctypes.data), None, _lib.OSP_HOST, 1, 1, ctypes.byref(o), None) == 0
        out = S.CsrResult(mctx, o)
        assert out.nnz == 3 and np.array_equal(out.colidx, [0, 3, 1])
        out.close()
        other = mctx.merge_csr_parts(3, 4, [(np.array([0, 0, 0, 1], np.int64), np.array([2], np.uint32), np.array([1.0]))])
        with pytest.raises(S.OspError) as ei:
            res.apply_mask(other)
        assert ei.value.status == _lib.ERR_ARG
        other.close()
        with pytest.raises(ValueError):
            res.apply_mask(good, space="elsewhere")
    finally:
        res.close()


def test_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    ts = [_dev(x) for x in (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, B.indptr.astype(np.int64),
                            B.indices.astype(np.uint32), B.data)]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        st, untouched = _raw(part, n, n, np.zeros(n + 1, np.int64), np.zeros(0, np.uint32))
        assert st == _lib.ERR_ARG and untouched
    finally:
        part.close()


# ---- composition --------------------------------------------------------------------------------------------------------------
def test_apply_mask_result_composes(mctx):
    ncol = 3000
    rowptr, col, val = _csr_from_lengths([5, 0, 700, 2500, 64], ncol, np.float64, seed=41)
    val = np.abs(val) + 0.1
    csr = (rowptr, col, val)
    m1, m2 = _mask_for(rowptr, col, ncol, seed=42, share=0.7), _mask_for(rowptr, col, ncol, seed=43, share=0.6)
    src = _upload(mctx, ncol, csr)
    try:
        # apply_mask of an apply_mask
        a, _ = src.apply_mask(m1, space="host")
        b, st = a.apply_mask(m2, complement=True, space="host")
        w1 = model.apply_mask(*csr, *m1, ncol)
        _check(b, st, ncol, w1, m2, True)
        assert 0 < b.nnz < a.nnz < src.nnz
        # into an inflate_prune (power 1, no pruning: the rows divided by their sums)
        t, ps = b.inflate_prune(1.0, 0.0, 0)
        assert ps["nnz_in"] == ps["nnz_out"] == b.nnz and np.array_equal(t.rowptr, b.rowptr) and np.array_equal(t.colidx, b.colidx)
        sums = np.add.reduceat(t.vals, t.rowptr[:-1][np.diff(t.rowptr) > 0])
        assert np.allclose(sums, 1.0, rtol=1e-12)
        # of a bias_relu
        bias = np.where(np.arange(ncol) % 3 == 0, -10.0, 0.5)
        br = src.bias_relu(bias, True)
        brh = (br.rowptr.copy(), br.colidx.copy(), br.vals.copy())
        c, st = br.apply_mask(m1, space="host", validate=True)
        _check(c, st, ncol, brh, m1, False)
        assert 0 < c.nnz < br.nnz   # (the bias fills every column it does not push below zero)
        # the other entry points of a result
        rows = torch.empty(c.nnz, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(DEV)
        c.coo_rows_into(rows.data_ptr())
        assert np.array_equal(rows.cpu().numpy(), np.repeat(np.arange(len(rowptr) - 1), np.diff(c.rowptr)))
        assert c.to_scipy().nnz == c.nnz and c.info["M"] == len(rowptr) - 1 and c.info["N"] == ncol
        for x in (a, b, t, br, c):
            x.close()
    finally:
        src.close()


def test_fifty_back_to_back_calls_give_the_same_arrays(mctx):
    """Recycled pool buffers carry nothing over from call to call (also run under OSP_POISON=1, see MEASUREMENTS.md 0d)."""
    ncol, csr, mask = _traps(np.float32)
    src = _upload(mctx, ncol, csr)
    try:
        first = None
        for i in range(50):
            complement = bool(i & 1)
            res, st = src.apply_mask(mask, complement=complement, space="host")
            got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["nnz_out"])
            res.close()
            if i < 2:
                first = (first or {}) | {complement: got}
                _ = model.apply_mask(*csr, *mask, ncol, complement)
                assert np.array_equal(got[0], _[0]) and np.array_equal(got[1], _[1]) and np.array_equal(got[2], _bits(_[2]))
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, first[complement])), i
    finally:
        src.close()


# ---- the launches a call reports ------------------------------------------------------------------------------------------------
# A filter of a non-empty `in` launches its flag kernel, the scan over the verdict words, the row-pointer kernel and, when
# anything is kept, the write kernel.  The scan is one kernel up to 16 tiles of 2048 words of 64 entries and three above.
SCAN_SMALL_MAX = 16 * 2048 * 64


@functools.lru_cache(maxsize=None)
def _launch_inputs():
    """(ncol, csr, kernels of the scan) for the largest input of the one-kernel scan and the smallest of the three-kernel one."""
    ncol = 1 << 20
    lengths = [700000, 0, SCAN_SMALL_MAX - 1400000, 700000]
    return tuple((ncol, _csr_from_lengths(lengths + extra, ncol, np.float32, seed=51, lo=0), scan) for extra, scan in (([], 1), ([1], 3)))


def test_apply_mask_reports_its_launches(mctx):
    for (ncol, csr, scan), nnz in zip(_launch_inputs(), (SCAN_SMALL_MAX, SCAN_SMALL_MAX + 1)):
        assert len(csr[1]) == nnz
        src = _upload(mctx, ncol, csr)
        try:
            # the mask is `in`'s own pattern: everything is kept, or (complement) nothing
            for complement, validate, want in ((False, False, 1 + scan + 1 + 1), (True, False, 1 + scan + 1), (False, True, 3 + 1 + scan + 1 + 1)):
                res, st = src.apply_mask(src, complement=complement, validate=validate)
                try:
                    assert st["nnz_out"] == res.nnz == (0 if complement else nnz)
                    assert st["launches"] == want, (nnz, complement, validate, st["launches"], want)
                finally:
                    res.close()
        finally:
            src.close()
    ncol, csr, mask = _simple("empty_in")(np.float32)
    src = _upload(mctx, ncol, csr)
    try:
        res, st = src.apply_mask(mask, space="host")
        assert st["launches"] == 0 and res.nnz == 0
        res.close()
    finally:
        src.close()
