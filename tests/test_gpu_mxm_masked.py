"""osp_csr_mxm_masked on the GPU, on the built pair of tests/test_gpu_mxm.py: row pointers and columns exact, values equal as
BITS, against tests/mxm_masked_model.py (a NaN that came out of an arithmetic operation is a NaN whatever its payload) AND
against ``a.mxm(b, ...).apply_mask(mask, complement=...)`` computed on the same device (bit for bit, NaNs included).

The masks come from PLANS: a plan names, per row of the output, the output columns to keep.  A plan gives two masks with the
same expected result -- KEEP holds the chosen columns (and columns the product lacks), DROP holds the other output columns
(and columns the product lacks) and is applied complemented -- and every mask is also run in the other sense."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import mxm_masked_model as model
from tests import semiring_model
from tests import test_gpu_apply_mask as am   # _upload, _dev, _bits only
from tests import test_gpu_mxm as tm          # the built pair, its model product, _assert_same

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits, _upload = am._bits, am._upload
CAP, N, M = tm.CAP, tm.N, len(tm.A_ROWS)
SEMIRINGS = tm.SEMIRINGS
F64 = np.float64


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


# ---- the plans ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows():
    """Per output row: its columns, and the number of products that feed each (the pattern does not depend on the semiring
    or the dtype)."""
    (rowptr, col, _), _ = tm._want(F64, "plus", "times")
    a, b = tm._pair(F64)
    prow, pcol = model.product_columns(a, b)
    out = [col[rowptr[i]:rowptr[i + 1]].astype(np.int64) for i in range(M)]
    fed = [dict(zip(*np.unique(pcol[prow == i], return_counts=True))) for i in range(M)]
    assert all(sum(f.values()) == u for f, u in zip(fed, tm.PRODUCTS))
    return out, fed


def _feeding(i, target):
    """Output columns of row i that are fed by exactly `target` products between them."""
    out, fed = _rows()
    chosen, left = [], target
    for c in sorted(out[i], key=lambda c: (-fed[i][c], c)):
        if c != 7 and fed[i][c] <= left:
            chosen.append(c)
            left -= fed[i][c]
    assert left == 0, (i, target)
    return np.sort(np.array(chosen, np.int64))


@functools.lru_cache(maxsize=None)
def _plans():
    out, _ = _rows()
    none, seven = np.zeros(0, np.int64), np.array([7])
    every = {i: out[i] for i in range(M)}
    ends = np.array([0, 5, N - 1])                               # columns rows 0, 13 and 15 lack: both ends of a bisection
    assert all(not np.isin(ends, out[i]).any() for i in (0, 13, 15)) and all(N - 1 not in o for o in out)
    # chosen columns per row; rows not named keep nothing.  extra: lacking columns added to the row of KEEP / of DROP
    a = {2: out[2], 3: np.arange(32), 4: out[4], 5: out[5], 6: out[6][::2], 7: out[7], 8: _feeding(8, 1), 9: seven, 10: seven,
         11: seven, 12: _feeding(12, 33), 13: none, 14: out[14], 15: none, 17: out[17][::2]}
    b = {2: none, 3: out[3], 4: np.arange(33), 5: np.arange(1, 64), 6: out[6], 7: out[7][1::2], 8: none, 9: out[9][out[9] != 7],
         10: out[10][out[10] != 7], 11: none, 12: out[12], 13: out[13], 14: out[14][:1], 15: out[15], 17: out[17]}
    nolong = dict(every)                                         # every long row of the one batch keeps nothing
    nolong.update({8: none, 9: none, 10: none, 17: none, 7: _feeding(7, 1)})
    return {"a": (a, {0: ends, 13: ends}, {15: ends}), "b": (b, {15: ends}, {0: ends, 13: ends}),
            "all": (every, {}, {}), "nolong": (nolong, {0: ends}, {})}


@functools.lru_cache(maxsize=None)
def _mask(plan, which):
    """which = "keep": the chosen columns; "drop": the other output columns.  Returns (rowptr, col, unit values)."""
    out, _ = _rows()
    chosen, extra_keep, extra_drop = _plans()[plan]
    rows = []
    for i in range(M):
        c = np.asarray(chosen.get(i, np.zeros(0, np.int64)), np.int64)
        assert np.isin(c, out[i]).all(), (plan, i)
        r = c if which == "keep" else np.setdiff1d(out[i], c)
        x = (extra_keep if which == "keep" else extra_drop).get(i, np.zeros(0, np.int64))
        assert not np.isin(x, out[i]).any()
        rows.append(np.union1d(r, x))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.uint32)
    return rowptr, col, np.ones(len(col), F64)


def _kept_by_row(mask, complement):
    a, b = tm._pair(F64)
    prow, pcol = model.product_columns(a, b)
    keep = np.isin(prow * N + pcol, model._keys(mask[0], mask[1], N)) != complement
    return np.bincount(prow[keep], minlength=M)


def test_the_plans_hold_the_cases_they_are_for():
    """The shapes of the mask rows and the kept counts, asserted with the model before anything runs on the device."""
    out, fed = _rows()
    pile9 = fed[9][7]                                            # the 1077 of the pile, and the wide rows that hold column 7
    assert 1077 <= pile9 <= 1087 and (fed[10][7], fed[11][7]) == (5000, 65)
    ka, da = _mask("a", "keep"), _mask("a", "drop")
    lens = lambda m: np.diff(m[0]).tolist()   # noqa: E731
    row = lambda m, i: m[1][m[0][i]:m[0][i + 1]].astype(np.int64)   # noqa: E731
    assert lens(ka)[1] == 0 and lens(ka)[15] == 0 and np.array_equal(row(da, 15), np.union1d(out[15], [0, 5, N - 1]))   # empty rows
    assert np.array_equal(row(ka, 7), out[7]) and np.array_equal(row(ka, 14), out[14])                # equal to the output columns
    assert row(ka, 13).tolist() == [0, 5, N - 1] and not np.isin(row(ka, 13), out[13]).any()          # disjoint, both ends
    assert np.array_equal(row(ka, 6), out[6][::2]) and np.array_equal(row(ka, 17), out[17][::2])      # every other column
    kb = _mask("b", "keep")
    assert (lens(ka)[2], lens(kb)[3], lens(ka)[4], lens(ka)[5]) == (1, 63, 64, 65)
    for i in (9, 10, 11):
        assert row(ka, i).tolist() == [7]
    for m, c in ((ka, False), (da, True)):
        kept = _kept_by_row(m, c)
        assert [kept[i] for i in (13, 2, 4, 5, 3, 12)] == [0, 1, 64, 65, 32, 33]                      # 0, 1, 64, 65, 2^5, 2^5 + 1
        assert kept[7] == CAP and kept[8] == 1 and (kept[9], kept[10], kept[11]) == (pile9, 5000, 65)
    # complemented, everything but the pile's entry survives
    kept = _kept_by_row(ka, True)
    assert (kept[9], kept[10], kept[11]) == (3 * CAP + 5 - pile9, 1, 0)
    kept = _kept_by_row(kb, False)
    assert (kept[3], kept[4], kept[8], kept[11]) == (63, 33, 0, 0) and kept[9] == 3 * CAP + 5 - pile9
    assert _kept_by_row(_mask("all", "keep"), False).tolist() == tm.PRODUCTS                            # the first long row: everything
    kept = _kept_by_row(_mask("nolong", "keep"), False)
    assert [kept[i] for i in (8, 9, 10, 17)] == [0, 0, 0, 0] and kept[7] == 1 and kept[6] == CAP - 1


# ---- operands on the device -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def operands(mctx):
    made = {}
    for dt in tm.DTYPES:
        a, b = tm._pair(dt)
        made[dt] = (_upload(mctx, tm.K, a), _upload(mctx, N, b))
    yield made
    for ra, rb in made.values():
        ra.close()
        rb.close()


@pytest.fixture(scope="module")
def masks(mctx):
    made = {(p, w): _upload(mctx, N, _mask(p, w)) for p in _plans() for w in ("keep", "drop")}
    yield made
    for r in made.values():
        r.close()


STAT_KEYS = ["nnz_a", "nnz_b", "nnz_mask", "products", "products_kept", "nnz_out", "short_rows", "long_rows", "batches", "launches",
             "ms_total"]


def _run(operands, masks, dt, add, mul, plan, which, complement, cap=CAP, budget=semiring_model.BATCH, full_dev=None):
    """One masked product, checked against the model and (with full_dev, the plain product on the device) the composition."""
    a, b = tm._pair(dt)
    ra, rb = operands[dt]
    mask, rm = _mask(plan, which), masks[plan, which]
    full, fst = tm._want(dt, add, mul, cap, budget)
    want, wst = model.filter_product(full, fst, a, b, mask, N, complement)
    res, st = ra.mxm(rb, add, mul, mask=rm, complement=complement)
    try:
        what = (add, mul, plan, which, complement, cap, budget)
        assert res.shape == (M, N) and res.dtype == dt and list(st) == STAT_KEYS
        tm._assert_same(res, want, what)
        for key in ("products", "products_kept", "nnz_out", "short_rows", "long_rows", "batches", "nnz_mask"):
            assert st[key] == wst[key], (key, what)
        assert (st["nnz_a"], st["nnz_b"]) == (len(a[1]), len(b[1])) and st["launches"] > 0 and st["ms_total"] >= 0
        info = res.info
        assert (info["M"], info["K"], info["N"], info["row_begin"], info["row_end"]) == (M, tm.K, N, 0, M)
        assert (info["nnz_a"], info["nnz_b"], info["nnz_c"], info["partials"]) == (len(a[1]), len(b[1]), wst["nnz_out"], wst["products"])
        named = {"M", "K", "N", "row_begin", "row_end", "nnz_a", "nnz_b", "nnz_c", "partials", "dtype", "ms_total"}
        assert all(v == 0 for k, v in info.items() if k not in named), info
        if full_dev is not None:
            ref, _ = full_dev.apply_mask(rm, complement=complement)
            try:
                assert np.array_equal(res.rowptr, ref.rowptr) and np.array_equal(res.colidx, ref.colidx), what
                assert np.array_equal(_bits(res.vals), _bits(ref.vals)), what
            finally:
                ref.close()
        return st
    finally:
        res.close()


@pytest.mark.parametrize("add,mul", SEMIRINGS)
def test_every_semiring_equals_the_model_and_the_composition(operands, masks, add, mul):
    full_dev, fst = operands[F64][0].mxm(operands[F64][1], add, mul)
    try:
        sts = [_run(operands, masks, F64, add, mul, "a", which, c, full_dev=full_dev)
               for which, c in (("keep", False), ("drop", True), ("keep", True), ("drop", False))]
        # the two masks of a plan keep the same products; the two senses of a mask partition the plain product
        assert sts[0]["products_kept"] == sts[1]["products_kept"] and sts[0]["nnz_out"] == sts[1]["nnz_out"]
        for x, y in ((sts[0], sts[2]), (sts[1], sts[3])):
            assert x["nnz_out"] + y["nnz_out"] == fst["nnz_out"] and x["products_kept"] + y["products_kept"] == fst["products"]
        assert (sts[0]["short_rows"], sts[0]["long_rows"], sts[0]["batches"]) == (11, 4, 1)
    finally:
        full_dev.close()


@pytest.mark.parametrize("dt", tm.DTYPES)
@pytest.mark.parametrize("plan", ["a", "b", "all", "nolong"])
def test_every_plan_in_both_dtypes(operands, masks, plan, dt):
    for add, mul in (("plus", "times"), ("min", "plus")):
        full_dev, fst = operands[dt][0].mxm(operands[dt][1], add, mul)
        try:
            for which in ("keep", "drop"):
                s0 = _run(operands, masks, dt, add, mul, plan, which, False, full_dev=full_dev)
                s1 = _run(operands, masks, dt, add, mul, plan, which, True, full_dev=full_dev)
                assert s0["nnz_out"] + s1["nnz_out"] == fst["nnz_out"] and s0["products_kept"] + s1["products_kept"] == fst["products"]
            if plan == "all":   # the mask IS the product's pattern: the bits of the plain product, and nothing the other way
                got, _ = operands[dt][0].mxm(operands[dt][1], add, mul, mask=masks["all", "keep"])
                assert np.array_equal(got.rowptr, full_dev.rowptr) and np.array_equal(got.colidx, full_dev.colidx)
                assert np.array_equal(_bits(got.vals), _bits(full_dev.vals))
                got.close()
        finally:
            full_dev.close()


@pytest.mark.parametrize("name,value", [("OSP_MXM_BATCH", 1), ("OSP_MXM_BATCH", 70), ("OSP_MXM_BATCH", 1100),
                                        ("OSP_MXM_SHORT_CAP", 1), ("OSP_MXM_SHORT_CAP", 64)])
def test_batches_and_the_short_cap_change_nothing(operands, masks, monkeypatch, name, value):
    monkeypatch.setenv(name, str(value))
    cap, budget = (value, semiring_model.BATCH) if name == "OSP_MXM_SHORT_CAP" else (CAP, value)
    for add, mul in (("plus", "times"), ("min", "plus")):
        for plan in ("a", "b", "nolong"):
            for which, c in (("keep", False), ("drop", True), ("keep", True)):
                st = _run(operands, masks, F64, add, mul, plan, which, c, cap, budget)
                if name == "OSP_MXM_BATCH":
                    assert st["batches"] == len(semiring_model.cut_batches(np.array(tm.PRODUCTS), budget)) > 1
                else:
                    assert st["long_rows"] > 4


# ---- the same handle in two places, a mask of the other dtype ---------------------------------------------------------------------------
def test_the_same_handle_in_two_or_three_places(mctx):
    n, r, c, v = gen.rmat_coo(8, 16, "g500", seed=4, dtype=F64)
    g = gen.coo_to_csr(n, r, c, v)
    h = (g[0], g[1], np.arange(len(g[1]), dtype=np.float32))          # the same pattern as a float32 result
    rng = np.random.default_rng(3)
    keep = rng.random(len(g[1])) < 0.5
    other = (np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(g[0]))[keep], minlength=n))]).astype(np.int64),
             g[1][keep], g[2][keep])
    rg, rh, ro = _upload(mctx, n, g), _upload(mctx, n, h), _upload(mctx, n, other)
    try:
        for add, mul in (("min", "plus"), ("plus", "times")):
            for a, ra, b, rb, m, rm in ((g, rg, g, rg, g, rg),        # all three
                                        (g, rg, other, ro, g, rg),    # mask is a
                                        (other, ro, g, rg, g, rg),    # mask is b
                                        (g, rg, g, rg, other, ro),    # a is b
                                        (g, rg, other, ro, h, rh)):   # a mask of the other dtype
                for comp in (False, True):
                    want, wst = model.mxm_masked(a, b, m, n, comp, add, mul)
                    res, st = ra.mxm(rb, add, mul, mask=rm, complement=comp)
                    try:
                        tm._assert_same(res, want, (add, mul, comp))
                        assert (st["products"], st["products_kept"], st["nnz_out"]) == (wst["products"], wst["products_kept"], wst["nnz_out"])
                        assert res.dtype == F64
                    finally:
                        res.close()
        for r_, x in ((rg, g), (ro, other)):                             # the operands stay valid
            assert np.array_equal(r_.rowptr, x[0]) and np.array_equal(r_.colidx, x[1]) and np.array_equal(_bits(r_.vals), _bits(x[2]))
    finally:
        for x in (rg, rh, ro):
            x.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def _raw(a, b, m, sr, complement=0, out=True):
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    stats = _lib.MxmMaskedStats()
    stats.products_kept = 77
    h = lambda r: r._h if r is not None else None   # noqa: E731
    st = _lib.lib().osp_csr_mxm_masked(h(a), h(b), h(m), complement, ctypes.byref(sr) if sr is not None else None,
                                       ctypes.byref(o) if out else None, ctypes.byref(stats))
    return st, o.value == sentinel and stats.products_kept == 77


def test_argument_and_dimension_errors_leave_the_outputs_alone(mctx):
    rowptr = np.array([0, 2, 3, 3, 3], np.int64)
    col, val = np.array([0, 3, 1], np.uint32), np.array([1.0, 2.0, 3.0])
    res = mctx.merge_csr_parts(4, 4, [(rowptr, col, val)])
    f32 = mctx.merge_csr_parts(4, 4, [(rowptr, col, val.astype(np.float32))])
    wide = mctx.merge_csr_parts(4, 5, [(rowptr, col, val)])
    tall = mctx.merge_csr_parts(5, 4, [(np.append(rowptr, 3), col, val)])
    other = S.Context(0)
    sr = tm._sr
    try:
        foreign = other.merge_csr_parts(4, 4, [(rowptr, col, val)])
        assert _raw(res, res, res, None) == (_lib.ERR_ARG, True)
        assert _raw(res, res, res, sr(), out=False)[0] == _lib.ERR_ARG
        for args in ((None, res, res), (res, None, res), (res, res, None)):
            assert _raw(*args, sr()) == (_lib.ERR_ARG, True)
        E = _lib.EWISE_OPS
        for add in (-1, E["times"], E["second"], E["minus"], E["div"], 8, 1 << 20):
            assert _raw(res, res, res, sr(add, E["times"])) == (_lib.ERR_ARG, True)
        for mul in (-1, E["minus"], E["div"], 8, 1 << 20):
            assert _raw(res, res, res, sr(E["plus"], mul), 1) == (_lib.ERR_ARG, True)
            assert _lib.lib().osp_last_error_string()
        for word in range(8):
            s = sr()
            s.reserved[word] = 1
            assert _raw(res, res, res, s) == (_lib.ERR_ARG, True)
        for args in ((foreign, res, res), (res, foreign, res), (res, res, foreign), (f32, res, res), (res, f32, res)):
            assert _raw(*args, sr()) == (_lib.ERR_ARG, True)
        assert _raw(wide, res, res, sr()) == (_lib.ERR_DIM, True)                      # 4 x 5 times 4 x 4
        assert _raw(res, res, wide, sr()) == (_lib.ERR_DIM, True)                      # a 4 x 5 mask on a 4 x 4 product
        assert _raw(res, res, tall, sr(), 1) == (_lib.ERR_DIM, True)                   # a 5 x 4 mask
        assert _raw(res, wide, res, sr()) == (_lib.ERR_DIM, True)                      # the product is 4 x 5
        # a mask of the other dtype is taken, every legal pair is taken, stats may be null
        for m, comp in ((f32, 0), (res, 1), (wide, 7)):
            o = ctypes.c_void_p()
            s = sr(E["min"], E["first"])
            b = wide if m is wide else res
            assert _lib.lib().osp_csr_mxm_masked(res._h, b._h, m._h, comp, ctypes.byref(s), ctypes.byref(o), None) == 0
            S.CsrResult(mctx, o).close()
        # the Python surface
        with pytest.raises(ValueError):
            res.mxm(res, complement=True)
        with pytest.raises(TypeError):
            res.mxm(res, mask=(rowptr, col))
        for bad in (foreign,):
            with pytest.raises(S.OspError) as ei:
                res.mxm(res, mask=bad)
            assert ei.value.status == _lib.ERR_ARG
        with pytest.raises(S.OspError) as ei:
            res.mxm(res, mask=wide)
        assert ei.value.status == _lib.ERR_DIM
        foreign.close()
    finally:
        other.close()
        for x in (res, f32, wide, tall):
            x.close()


def test_a_partials_result_is_refused_in_each_place(mctx):
    import scipy.sparse as sp
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    ts = [am._dev(x) for x in (A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data, B.indptr.astype(np.int64),
                               B.indices.astype(np.uint32), B.data)]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    full = mctx.spgemm_csc_csr_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        for args in ((part, full, full), (full, part, full), (full, full, part), (part, part, part)):
            assert _raw(*args, tm._sr()) == (_lib.ERR_ARG, True)
    finally:
        part.close()
        full.close()


# ---- the zero cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", tm.DTYPES)
def test_zero_cases_give_an_empty_result(mctx, dt):
    z = lambda m: np.zeros(m + 1, np.int64)   # noqa: E731
    none_c, none_v = np.zeros(0, np.uint32), np.zeros(0, dt)
    full = (np.array([0, 2, 3, 3], np.int64), np.array([0, 2, 1], np.uint32), np.array([1, 2, 3], dt))       # 3 x 3
    meets_empty = (np.array([0, 1, 2, 2], np.int64), np.array([1, 1], np.uint32), np.array([4, 5], dt))     # points at row 1 only
    b_row1_empty = (np.array([0, 2, 2, 3], np.int64), np.array([0, 1, 2], np.uint32), np.array([1, 2, 3], dt))
    empty3, empty0 = (z(3), none_c, none_v), (z(0), none_c, none_v)
    prod = semiring_model.mxm(full, full, 3)[0]                                                              # full x full
    lacking = semiring_model._dense_to_csr(~semiring_model._csr_to_dense(prod, (3, 3), dt)[0], np.ones((3, 3), dt))
    cases = {"empty a": (empty3, full, full, False, 0), "empty b": (full, empty3, full, True, 0), "M == 0": (empty0, full, empty0, True, 0),
             "every k meets an empty row": (meets_empty, b_row1_empty, full, True, 0),
             "an empty mask": (full, full, empty3, False, None), "a mask that admits nothing": (full, full, lacking, False, None),
             "the product's own pattern, complemented": (full, full, prod, True, None)}
    for name, (a, b, m, comp, launches) in cases.items():
        ra, rb, rm = _upload(mctx, 3, a), _upload(mctx, 3, b), _upload(mctx, 3, m)
        try:
            for add, mul in (("plus", "times"), ("min", "first")):
                res, st = ra.mxm(rb, add, mul, mask=rm, complement=comp)
                try:
                    rows = len(a[0]) - 1
                    wst = model.mxm_masked(a, b, m, 3, comp, add, mul)[1]
                    assert res.shape == (rows, 3) and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(rows + 1, np.int64)), name
                    assert all(st[k] == wst[k] for k in ("products", "products_kept", "nnz_out", "short_rows", "long_rows", "batches")), name
                    assert st["products_kept"] == 0 and st["nnz_mask"] == len(m[1]) and res.info["partials"] == wst["products"]
                    if launches is not None:
                        assert st["products"] == 0 and (name == "every k meets an empty row" or st["launches"] == launches), name
                    if rows:
                        nxt, _ = res.mxm(rb, mask=rm)            # an empty result is an operand like any other
                        assert nxt.nnz == 0
                        nxt.close()
                finally:
                    res.close()
            if name == "an empty mask":                          # complemented: the bits of the plain product
                res, st = ra.mxm(rb, mask=rm, complement=True)
                tm._assert_same(res, prod)
                assert st["products_kept"] == st["products"] == semiring_model.mxm(a, b, 3)[1]["products"] == 3
                res.close()
        finally:
            for x in (ra, rb, rm):
                x.close()


@pytest.mark.parametrize("budget", [None, 1, 70])
def test_an_empty_mask_on_a_product_of_several_batches(mctx, operands, monkeypatch, budget):
    """Nothing can be kept, whatever the number of batches: an empty result with a row pointer of zeros (the path that skips
    the batches must also skip their assembly), the symbolic stats as the plain product's; complemented, the plain product."""
    if budget is not None:
        monkeypatch.setenv("OSP_MXM_BATCH", str(budget))
    a, b = tm._pair(F64)
    ra, rb = operands[F64]
    empty = (np.zeros(M + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, F64))
    rm = _upload(mctx, N, empty)
    try:
        for add, mul in (("plus", "times"), ("min", "first")):
            full, fst = tm._want(F64, add, mul, CAP, budget or semiring_model.BATCH)
            dirty, _ = ra.mxm(rb, add, mul)          # (the pool's buffers hold a product's counts when the masked call takes them)
            dirty.close()
            res, st = ra.mxm(rb, add, mul, mask=rm)
            try:
                assert res.shape == (M, N) and res.nnz == 0 and res.info["nnz_c"] == 0 and res.info["partials"] == fst["products"]
                assert np.array_equal(res.rowptr, np.zeros(M + 1, np.int64)) and len(res.colidx) == 0
                assert (st["products"], st["products_kept"], st["nnz_out"], st["nnz_mask"]) == (fst["products"], 0, 0, 0)
                assert (st["short_rows"], st["long_rows"], st["batches"]) == (fst["short_rows"], fst["long_rows"], fst["batches"])
                assert (st["batches"] > 1) == (budget is not None)
                T, _ = res.transpose()               # an ordinary result
                assert T.shape == (N, M) and T.nnz == 0
                T.close()
            finally:
                res.close()
            res, st = ra.mxm(rb, add, mul, mask=rm, complement=True)
            try:
                tm._assert_same(res, full, (add, mul, budget))
                assert st["products_kept"] == st["products"] == fst["products"] and st["batches"] == fst["batches"]
            finally:
                res.close()
    finally:
        rm.close()


# ---- composition, repetition, the plain call ----------------------------------------------------------------------------------------------
def test_masked_results_compose(mctx):
    n, r, c, v = gen.rmat_coo(8, 16, "g500", seed=6, dtype=F64)
    g = gen.coo_to_csr(n, r, c, v)
    rg = _upload(mctx, n, g)
    made = []
    try:
        P, _ = rg.mxm(rg, "min", "plus", mask=rg, complement=True)
        made.append(P)
        want = model.mxm_masked(g, g, g, n, True, "min", "plus")[0]
        tm._assert_same(P, want)
        Q, _ = P.mxm(rg, "max", "min", mask=P)                    # its own output as an operand and as the mask
        made.append(Q)
        tm._assert_same(Q, model.mxm_masked(want, g, want, n, False, "max", "min")[0])
        T, _ = P.transpose()
        made.append(T)
        back, _ = T.transpose()
        made.append(back)
        assert np.array_equal(back.rowptr, want[0]) and np.array_equal(back.colidx, want[1]) and np.array_equal(_bits(back.vals), _bits(want[2]))
    finally:
        for x in made:
            x.close()
        rg.close()


def test_twenty_back_to_back_calls_of_each_of_four_give_the_same_arrays_and_launches(operands, masks):
    ra, rb = operands[F64]
    first = {}
    for i in range(80):                       # four configurations in turn, twenty calls of each
        key = [("plus", "times", "a", "keep", False), ("min", "plus", "b", "drop", True), ("first", "second", "nolong", "keep", False),
               ("max", "min", "a", "keep", True)][i % 4]
        add, mul, plan, which, comp = key
        res, st = ra.mxm(rb, add, mul, mask=masks[plan, which], complement=comp)
        got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["nnz_out"], st["products_kept"], st["launches"])
        res.close()
        if key not in first:
            first[key] = got
        else:
            assert all(np.array_equal(x, y) for x, y in zip(got, first[key])), i


def test_the_plain_call_is_what_it_was(operands):
    ra, rb = operands[F64]
    res, st = ra.mxm(rb)
    try:
        assert list(st) == ["nnz_a", "nnz_b", "products", "nnz_out", "short_rows", "long_rows", "batches", "launches", "ms_total"]
        tm._assert_same(res, tm._want(F64, "plus", "times")[0])
        res2, st2 = ra.mxm(rb, mask=None, complement=False)
        assert list(st2) == list(st) and st2["launches"] == st["launches"] and np.array_equal(_bits(res2.vals), _bits(res.vals))
        res2.close()
    finally:
        res.close()
