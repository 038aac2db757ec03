"""osp_csr_select_k on the GPU against the numpy model of tests/select_k_model.py: row pointers and columns exact, value
BITS equal (values are copied), and the stats counters (nnz, capped rows, long rows, launches, read-backs) the model's.
Operands go up through ``Context.build(dup="error")`` and every seventh entry carries a special value.  The sweep over the
operand family, row lengths at the edges of a wave, a workgroup stride and the class boundary, ties of every kind, IEEE edge
values, layouts that cross compaction chunks, one row of 9 * 10^6 entries, wide columns, the identities that tie the select
to itself and to ``inflate_prune``, the refusals, and the sweep's slice in children on a poisoned and on a guarded pool."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import select_k_cases as sc
from tests import select_k_model as model
from tests import test_gpu_apply_mask as am   # _dev, _bits and _special only
from tests import wide_columns as wc

pytestmark = pytest.mark.gpu

ROOT = sc.ROOT
DEV = am.DEV
_bits = am._bits
LM = _lib.SELECT_K_LONG_MIN
CHUNK = 2048   # kCompactChunk: the entries one workgroup of the flag pass takes
CHILD_TIMEOUT_S = 180   # a hang guard: a child starts Python, loads the library, creates a context and makes 144 small selects
COUNTERS = ("nnz_in", "nnz_out", "rows_capped", "rows_long", "launches", "readbacks")


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _check(res, st, src, csr, ncol, k, order, seed=0):
    (rowptr, col, val), want = model.select_k(csr, ncol, k, order, seed)
    assert res.shape == src.shape and res.dtype == csr[2].dtype.type and res.nnz == len(col)
    assert np.array_equal(res.rowptr, rowptr)
    assert np.array_equal(res.colidx, col)
    assert np.array_equal(_bits(res.vals), _bits(val))
    assert {name: st[name] for name in COUNTERS} == want, (k, order)
    assert st["ms_total"] >= 0
    info, base = dict(res.info), dict(src.info)     # in's info with nnz_c and ms_total replaced
    assert info.pop("nnz_c") == len(col) and info.pop("ms_total") == st["ms_total"]
    base.pop("nnz_c"), base.pop("ms_total")
    assert info == base


def _sweep(mctx, csr, ncol, ks, orders=model.ORDERS, seed=0):
    """Uploads the operand and checks every (k, order) against the model; closes everything."""
    A = sc.build(mctx, csr, ncol)
    try:
        assert np.array_equal(A.rowptr, csr[0]) and np.array_equal(A.colidx, csr[1]) and np.array_equal(_bits(A.vals), _bits(csr[2]))
        for order in orders:
            for k in ks:
                res, st = A.select_k(int(k), order, seed=seed)
                try:
                    _check(res, st, A, csr, ncol, int(k), order, seed)
                finally:
                    res.close()
        assert A.to_host() is not None and A.info["nnz_c"] == A.nnz   # the operand stays valid
    finally:
        A.close()


def _rows(lengths, ncol, dt, seed):
    return sc.csr_of(sc.random_rows(lengths, ncol, seed), dt, seed)


def _one_row(vals, cols=None):
    vals = np.asarray(vals)
    cols = np.arange(len(vals)) if cols is None else np.asarray(cols)
    return np.array([0, len(vals)], np.int64), cols.astype(np.uint32), vals


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", model.ORDERS)
def test_select_k_equals_the_model_over_the_family(mctx, order, dt):
    assert sc.KS == (1, 2, 7, 64, (1 << 32) - 1)
    assert np.array_equal(_bits(sc.kc.special(dt)), _bits(am._special(dt)))
    for name, (csr, ncol) in sc.family(dt).items():
        _sweep(mctx, csr, ncol, sc.KS, [order], seed=17)


# ---- row lengths at the edges ------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = [63, 64, 65, 255, 256, 257, LM - 1, LM, LM + 1]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", model.ORDERS)
def test_row_lengths_around_a_wave_a_stride_and_the_class_boundary(mctx, order, dt):
    """One operand with a row of every edge length (and 1, 2, 3: k - 1, k, k + 1 at k = 2); every k below, at and above each."""
    assert LM == 2048
    csr = _rows([1, 2, 3] + EDGE_LENGTHS, 3 * LM, dt, 21)
    ks = sorted({2} | {m + d for m in EDGE_LENGTHS for d in (-1, 0, 1)})
    _sweep(mctx, csr, 3 * LM, ks, [order], seed=5)


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [300, LM + 900])
def test_a_row_of_one_repeated_value(mctx, n, dt):
    """Every radix pass runs and the tie column decides everything: the first k columns stay."""
    for value in (2.5, -0.0, np.nan):
        csr = _one_row(np.full(n, value, dt), np.arange(n) * 3 + 1)
        _sweep(mctx, csr, 3 * n + 5, (1, 63, 64, 65, 256, 257, n - 1), ("largest", "smallest"))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_kth_value_tied_across_the_cut(mctx, dt):
    rng = np.random.default_rng(31)
    for n in (40, 700, LM + 500):
        v = rng.choice(np.array([9.0, 5.0, 5.0, 5.0, 1.0, -3.0], dt), n)
        nine, five = int((v == 9).sum()), int((v == 5).sum())
        ks = sorted({1, nine, nine + 1, nine + five // 2, nine + five - 1, nine + five, nine + five + 1} - {0})
        _sweep(mctx, _one_row(v), n, ks, ("largest",))
        one, three = int((v == 1).sum()), int((v == -3).sum())
        _sweep(mctx, _one_row(v), n, sorted({three, three + 1, three + one // 2, three + one} - {0}), ("smallest",))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ties_that_straddle_a_wave_and_a_stride_of_a_long_row(mctx, dt):
    """The threshold's equals sit at positions 60..70, 250..262 and 3 * 256 - 2 .. 3 * 256 + 2 of a long row and of a short
    one; the cut falls inside each group in turn."""
    for n in (LM + 700, 1000):
        v = np.full(n, 1.0, dt)
        v[:20] = 8.0
        ties = np.concatenate([np.arange(60, 71), np.arange(250, 263), np.arange(3 * 256 - 2, 3 * 256 + 3)])
        v[ties] = 4.0
        ks = [20 + c for c in (1, 4, 5, 11, 12, 17, 23, 24, 26, 28, len(ties))] + [20 + len(ties) + 1]
        _sweep(mctx, _one_row(v), n, ks, ("largest",))
        _sweep(mctx, _one_row(-v), n, ks, ("smallest",))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_keys_that_differ_in_the_lowest_byte_only_and_in_the_top_byte_already(mctx, dt):
    u = np.uint32 if dt == np.float32 else np.uint64
    rng = np.random.default_rng(33)
    for n in (200, LM + 50):
        low = (np.asarray(1.0, dt).view(u) + rng.integers(0, 256, n).astype(u)).view(dt)   # every pass but the last sees one bucket
        _sweep(mctx, _one_row(low), n, (1, 2, 50, 128, n - 1), ("largest", "smallest"))
        _sweep(mctx, _one_row(-low), n, (1, 50, n - 1), ("largest", "smallest"))
        # exponents across the whole range, both signs: the first pass already separates most of the row (the early stop)
        top = (rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-120, 120, n).astype(np.float64))).astype(dt)
        _sweep(mctx, _one_row(top), n, (1, 2, 3, 50, n - 1), ("largest", "smallest"))


# ---- IEEE edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ieee_edge_values_in_one_row(mctx, dt):
    sp = am._special(dt)     # NaNs of both signs and two payloads, +-inf, +-0, denormals of both signs, the largest number, 1
    more = np.array([-1.0, -np.finfo(dt).max, -np.finfo(dt).tiny, np.finfo(dt).tiny, 0.0, -0.0, np.nan, -np.nan], dt)
    v = np.concatenate([sp, more, sp[::-1], -more])
    assert np.isnan(v).sum() >= 8 and np.isinf(v).sum() >= 4 and (v == 0).sum() >= 8 and (v < 0).sum() >= 6
    _sweep(mctx, _one_row(v, np.arange(len(v)) * 5), 5 * len(v), range(1, len(v) + 1), ("largest", "smallest"))
    # the same among a long row of ordinary numbers
    rng = np.random.default_rng(34)
    big = rng.standard_normal(LM + 300).astype(dt)
    big[rng.choice(len(big), len(v), replace=False)] = v
    _sweep(mctx, _one_row(big), len(big), (1, 5, 100, len(big) - 30, len(big) - 9, len(big) - 1), ("largest", "smallest"))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_row_that_is_all_nan(mctx, dt):
    u = np.uint32 if dt == np.float32 else np.uint64
    nan = np.asarray(np.nan, dt).view(u)
    for n in (100, LM + 10):
        v = (nan + np.arange(n).astype(u) % u(5) + (np.arange(n).astype(u) % u(2) << u(8 * dt().itemsize - 1))).view(dt)   # payloads, signs
        assert np.isnan(v).all()
        _sweep(mctx, _one_row(v), n, (1, 2, 64, n - 1), ("largest", "smallest"))


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_rows_that_straddle_compaction_chunks_and_empty_rows_between_capped_rows(mctx, dt):
    lengths = [CHUNK - 5, 20, 0, 0, 3 * CHUNK + 7, 1, 0, CHUNK, 9, 0, 0, 0, 2 * CHUNK - 1, 40]
    _sweep(mctx, _rows(lengths, 4 * CHUNK, dt, 41), 4 * CHUNK, (1, 8, 30, CHUNK - 6, CHUNK + 1))


def test_two_to_the_20_empty_rows_around_three_capped_ones(mctx):
    m = 1 << 20
    lengths = np.zeros(m, np.int64)
    lengths[[0, 1 << 19, m - 1]] = [9, LM + 3, 5]
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    inner = _rows([9, LM + 3, 5], 3 * LM, np.float64, 42)
    csr = (rowptr, inner[1], inner[2])
    _sweep(mctx, csr, 3 * LM, (1, 4, 100))


def test_no_rows_and_no_entries(mctx):
    csr, ncol = sc.family(np.float64)["ragged"]
    A = sc.build(mctx, csr, ncol)
    E = sc.build(mctx, *sc.family(np.float32)["empty"])
    try:
        Z = A.extract(rows=np.zeros(0, np.int64), space="host")[0]     # M == 0
        try:
            assert Z.shape == (0, ncol)
            for src in (Z, E):
                for order in model.ORDERS:
                    res, st = src.select_k(3, order)
                    assert res.shape == src.shape and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(src.shape[0] + 1, np.int64))
                    assert {name: st[name] for name in COUNTERS} == dict.fromkeys(COUNTERS, 0)
                    res.close()
        finally:
            Z.close()
    finally:
        A.close()
        E.close()


# ---- one row of 9 * 10^6 entries --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub(mctx):
    n = 9_000_000
    rng = np.random.default_rng(43)
    val = rng.integers(0, 1000, n).astype(np.float64)   # about 9000 copies of every value: the select runs to the last byte
    csr = (np.array([0, n], np.int64), np.arange(n, dtype=np.uint32), val)
    A = sc.build(mctx, csr, n)
    yield A, csr
    A.close()


@pytest.mark.parametrize("order", model.ORDERS)
def test_a_hub_row_of_nine_million_entries(mctx, hub, order):
    """The expectation comes from ``np.partition``, not from the model's sort of the whole row: the entries strictly better
    than the k-th key, and of the entries equal to it the leftmost ones."""
    A, (_, col, val) = hub
    n, k = len(col), 20_000
    key = model.random_keys(3, 0, col) if order == "random" else -val if order == "largest" else val
    kth = np.partition(key, k - 1)[k - 1]
    better = key < kth
    want = np.sort(np.concatenate([np.flatnonzero(better), np.flatnonzero(key == kth)[:k - int(better.sum())]]))
    assert len(want) == k and (order != "random" or int(better.sum()) == k - 1)
    res, st = A.select_k(k, order, seed=3)
    try:
        print(f"hub row, {order}: {st['ms_total']:.3f} ms, {st['launches']} launches")
        assert np.array_equal(res.rowptr, [0, k]) and np.array_equal(res.colidx, col[want]) and np.array_equal(_bits(res.vals), _bits(val[want]))
        assert {name: st[name] for name in COUNTERS} == {"nnz_in": n, "nnz_out": k, "rows_capped": 1, "rows_long": 1,
                                                         "launches": 1 + 1 + 1 + model.scan_launches(-(-n // 64)) + 2, "readbacks": 2}
    finally:
        res.close()


# ---- wide columns --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_columns_on_both_sides_of_bit_31_and_up_to_the_last_one(mctx, dt):
    N = (1 << 32) - 1
    narrow = _rows([90, 3, 0, 130, LM + 5], 3 * LM, dt, 44)
    table = wc.phi("straddle", 3 * LM, N)
    csr = wc.relabel_csr(narrow, table)
    first = csr[1][:90].astype(np.int64)
    assert (first < (1 << 31)).any() and (first >= (1 << 31)).any()
    last = csr[1].copy()
    last[csr[0][4] - 1] = N - 1                   # the capped row of 130 entries ends at the last column there is
    ending = (csr[0], last, csr[2])
    assert int(last[csr[0][4] - 1]) == (1 << 32) - 2 and csr[0][4] - csr[0][3] == 130 and np.all(np.diff(last[csr[0][3]:csr[0][4]].astype(np.int64)) > 0)
    for case in (csr, ending):
        _sweep(mctx, case, N, (1, 7, 64), seed=(1 << 64) - 1)
    # RANDOM reads the full column: the relabeled operand draws differently from the narrow one
    a = model.select_k(narrow, 3 * LM, 7, "random", 9)[0]
    b = model.select_k(csr, N, 7, "random", 9)[0]
    assert not np.array_equal(wc.relabel(a[1], table), b[1])


# ---- identities on the device ------------------------------------------------------------------------------------------------------
def _same(x, y):
    assert x.shape == y.shape and x.nnz == y.nnz
    assert np.array_equal(x.rowptr, y.rowptr) and np.array_equal(x.colidx, y.colidx) and np.array_equal(_bits(x.vals), _bits(y.vals))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_identities_on_the_device(mctx, dt):
    fam = sc.family(dt)
    tmp = []

    def keep(pair):
        tmp.append(pair[0])
        return pair
    try:
        for name in ("ragged", "long ties", "dense"):
            csr, ncol = fam[name]
            A = keep((sc.build(mctx, csr, ncol), None))[0]
            longest = int(np.diff(csr[0]).max())
            for order in model.ORDERS:
                # k >= the longest row: `in` bit for bit, and no select kernel (the classify pass alone, or nothing at all)
                for k in (longest, longest + 1, (1 << 32) - 1):
                    res, st = keep(A.select_k(k, order, seed=2))
                    _same(res, A)
                    assert st["launches"] == (1 if k < min(ncol, A.nnz) else 0) and st["rows_capped"] == 0
                # nesting
                for k, k2 in ((64, 7), (7, 2), (max(longest - 1, 1), min(64, max(longest - 1, 1))), (2, 2)):
                    _same(keep(keep(A.select_k(k, order, seed=2))[0].select_k(k2, order, seed=2))[0], keep(A.select_k(k2, order, seed=2))[0])
            while len(tmp) > 1:
                tmp.pop().close()
            tmp.pop().close()
    finally:
        for x in tmp:
            x.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_largest_keeps_what_inflate_prune_keeps_on_finite_non_negative_input(mctx, dt):
    """The existing code as an independent witness: its pattern, not its (normalised) values."""
    rng = np.random.default_rng(45)
    lengths = [0, 5, 64, 65, 300, LM, LM + 1, 3 * LM, 1, 17]
    rowptr, col, _ = _rows(lengths, 4 * LM, dt, 46)
    val = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 3.0, 1e-3, 7.5], dt), len(col))   # ties, zeros
    val[::3] = rng.random(len(val[::3])).astype(dt)
    A = sc.build(mctx, (rowptr, col, val), 4 * LM)
    try:
        for k in (1, 2, 7, 64, 299, LM, LM + 1):
            mine, _ = A.select_k(k, "largest")
            theirs, st = A.inflate_prune(power=1.0, threshold=0.0, max_per_row=k)
            try:
                assert np.array_equal(mine.rowptr, theirs.rowptr) and np.array_equal(mine.colidx, theirs.colidx), k
            finally:
                mine.close()
                theirs.close()
    finally:
        A.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", model.ORDERS)
def test_the_result_does_not_depend_on_the_class(mctx, order, dt):
    """The same entries selected by one wave and by a workgroup: a row of LM + 600 entries (the workgroup's class) keeps under
    k what its first LM entries (the wave's class) keep, whenever everything it keeps lies among them -- arranged by putting
    the row's worst keys behind position LM.  For RANDOM the keys are the hash's: the long row's choice is compared with
    the choice among the SAME columns cut at LM after a first select has shortened the row (nesting across the classes)."""
    n = LM + 600
    rng = np.random.default_rng(47)
    if order == "random":
        csr = _one_row(rng.standard_normal(n).astype(dt), np.arange(n) * 2)
        A = sc.build(mctx, csr, 2 * n)
        try:
            for k in (1, 64, 500):
                long_, st_long = A.select_k(k, order, seed=8)
                short, st_mid = A.select_k(LM, order, seed=8)        # a workgroup shortens the row to the wave's class
                again, st_short = short.select_k(k, order, seed=8)   # one wave selects among what is left
                try:
                    assert (st_long["rows_long"], st_mid["rows_long"], st_short["rows_long"]) == (1, 1, 0) and st_short["rows_capped"] == 1
                    _same(long_, again)
                finally:
                    for x in (long_, short, again):
                        x.close()
        finally:
            A.close()
        return
    v = rng.choice(np.array([1.0, 2.0, 2.0, 3.0, 5.0], dt), n)
    worst = dt(-9.0) if order == "largest" else dt(9.0)
    v[LM:] = worst
    long_csr, short_csr = _one_row(v), _one_row(v[:LM])
    A, B = sc.build(mctx, long_csr, n), sc.build(mctx, short_csr, n)
    try:
        for k in (1, 64, 700, LM - 1):
            x, sx = A.select_k(k, order)
            y, sy = B.select_k(k, order)
            try:
                assert (sx["rows_long"], sy["rows_long"]) == (1, 0) and sx["rows_capped"] == sy["rows_capped"] == 1
                _same(x, y)
            finally:
                x.close()
                y.close()
    finally:
        A.close()
        B.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(a, order=0, k=1, reserved=None):
    """osp_csr_select_k itself.  Returns (status, whether *out and *stats are as they were), or (0, the handle)."""
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.SelectKStats()
    st.nnz_in = 77
    spec = _lib.SelectK()
    spec.order, spec.k = order, k
    if reserved is not None:
        spec.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_select_k(a._h, ctypes.byref(spec), ctypes.byref(o), ctypes.byref(st))
    if rc == 0:
        return rc, o
    assert _lib.lib().osp_last_error_string()
    return rc, o.value == sentinel and st.nnz_in == 77


def test_refusals_leave_out_and_stats_untouched(mctx):
    csr, ncol = sc.family(np.float64)["ragged"]
    A = sc.build(mctx, csr, ncol)
    try:
        for order in (-1, 3, 1 << 20):
            assert _raw(A, order) == (_lib.ERR_ARG, True), order
        for order in (0, 1, 2):
            assert _raw(A, order, k=0) == (_lib.ERR_ARG, True)
        for word in range(8):
            assert _raw(A, reserved=word) == (_lib.ERR_ARG, True), word
        with pytest.raises(ValueError):
            A.select_k(0)
        rc, o = _raw(A, 2, 3)                            # and the library still works
        assert rc == 0
        got = S.CsrResult(mctx, o)
        assert np.array_equal(np.diff(got.rowptr), np.minimum(np.diff(csr[0]), 3))
        got.close()
    finally:
        A.close()


def test_a_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    acsc, bcsr = gen.coo_to_csc(n, r, c, v), gen.coo_to_csr(n, c, r, v)
    ts = [am._dev(x) for x in acsc + bcsr]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        assert _raw(part) == (_lib.ERR_ARG, True)
        with pytest.raises(S.OspError) as ei:
            part.select_k(3)
        assert ei.value.status == _lib.ERR_ARG
    finally:
        part.close()


# ---- the pool -----------------------------------------------------------------------------------------------------------------------------
_state = {"digest": None, "stop": None}


def test_the_slice_in_this_process(mctx):
    _state["digest"] = sc.slice_digest(mctx)
    assert _state["digest"][1] == 2 * len(sc.SLICE) * len(model.ORDERS) * len(sc.SLICE_KS)


def _child(mode):
    assert not _state["stop"], f"{_state['stop']}: nothing further is started on the GPU"
    assert _state["digest"] is not None, "the in-process run did not finish: no digest to compare with"
    env = dict(os.environ)
    env[mode] = "1"
    try:
        r = subprocess.run([sys.executable, "-m", "tests.select_k_cases"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _state["stop"] = f"the child under {mode} hung"
        raise
    if r.returncode != 0:
        _state["stop"] = f"the child under {mode} ended with status {r.returncode}"
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("SELECT_K_SLICE ")]
    assert line == [f"SELECT_K_SLICE {_state['digest'][0]} calls={_state['digest'][1]}"], r.stdout[-2000:]
    return r


def test_the_slice_in_a_child_under_poison():
    _child("OSP_POISON")


def test_the_slice_in_a_child_under_guard():
    r = _child("OSP_GUARD")
    assert "[osp] OSP_GUARD:" not in r.stderr, r.stderr[-4000:]
