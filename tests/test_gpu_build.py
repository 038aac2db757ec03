"""osp_csr_build on the GPU against tests/build_model.py -- row pointers, columns and value BITS equal, the stats too -- for
every operator on one built list whose runs have every length that matters and lie across the boundaries that matter,
special values, the sort's boundaries, lists without values, host lists, device tensors and bare addresses, its refusals
(host and device lists, `out` and `stats` untouched), empty shapes, chaining with the other result operations, and the
pool."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import build_model as model
from tests import test_gpu_apply_mask as am        # _bits, _special, _dev, DEV only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
DTYPES = [np.float32, np.float64]
OPS = list(model.DUP_OPS)
M, N = 300, 5000
L = model.LONG_RUN
# the lengths of the placed runs, each at a coordinate of its own; everything else is background
RUNS = [1, 2, 3, L - 1, L, L + 1, 2047, 2048, 2049, 20000]
SORT_TILE = model.SORT_TILE


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


# short runs put where they cross a boundary of the sorted order: (sorted position of the head, length)
STRADDLERS = [(63, 2), (127, 3), (190, 2), (2047, 2)]


@functools.lru_cache(maxsize=None)
def _built():
    """(rows, cols, the model's layout): ~63 000 entries in list order.  The placed runs sit in rows 40, 50, ...; in the rows
    before them the STRADDLERS are put at their sorted positions; behind them 1700 random coordinates are given twice and
    800 three times; the rest is given once.  Rows 0 and M - 1 are empty and the last sorted entry is alone at its
    coordinate.  The list is then shuffled by a seeded permutation."""
    rng = np.random.default_rng(31)
    placed = [(40 + 10 * i) * N + 17 + 311 * i for i in range(len(RUNS))]
    last = (M - 2) * N + N - 1
    uniq = rng.choice((M - 2) * N, 33000, replace=False) + N               # rows 1 .. M - 2
    uniq = np.union1d(np.setdiff1d(uniq, placed + [last]), placed + [last])   # ascending: the sorted order's coordinates
    mult = np.ones(len(uniq), np.int64)
    mult[np.searchsorted(uniq, placed)] = RUNS
    free = np.flatnonzero((uniq > 140 * N) & (uniq != last))               # behind the placed runs
    again = rng.permutation(free)[:2500]
    mult[again[:1700]], mult[again[1700:]] = 2, 3
    for at, k in STRADDLERS:                                               # in ascending order: each moves what lies behind it
        i = int(np.searchsorted(np.cumsum(mult) - mult, at))
        assert np.cumsum(mult)[i] - mult[i] == at and mult[i] == 1 and uniq[i] < 40 * N
        mult[i] = k
    key = np.repeat(uniq, mult)
    key = key[rng.permutation(len(key))]                                   # the seeded shuffle
    r, c = key // N, key % N
    lay = model.build(M, N, r, c, None, "count", np.float64)[2]
    head, length = lay["head"], lay["length"]
    end = head + length - 1
    # the placement the kernels' paths depend on, as the model reports it
    assert model.CHUNK == 2048 and len(key) <= 100000
    assert sorted(length[length > 3].tolist()) == sorted(k for k in RUNS if k > 3)
    assert all(length[np.searchsorted(head, at)] == k and head[np.searchsorted(head, at)] == at for at, k in STRADDLERS)
    short = (length >= 2) & (length <= L)
    assert (short & (head // 64 != end // 64)).any()                       # a lane's own run continues in the next word
    assert (short & (head // model.CHUNK != end // model.CHUNK)).any()     # and in the next workgroup's chunk
    assert (short & (head % 64 == 63)).any() and (short & (end % 64 == 63)).any()
    long_ = length > L
    assert (long_ & (head // 64 != end // 64)).any() and (long_ & (head // model.CHUNK != end // model.CHUNK)).any()
    assert (length > 128).any()                                            # the next head lies beyond the next word: the bisection
    assert length[-1] == 1 and head[-1] == len(key) - 1                    # the last sorted entry is a head
    assert r.min() >= 1 and r.max() == M - 2                               # the first and the last row are empty
    return r, c, lay


@functools.lru_cache(maxsize=None)
def _values(dt):
    return np.random.default_rng(32).standard_normal(len(_built()[0])).astype(dt)


def _assert_same(res, want, what="", computed_nans=False):
    """computed_nans: a NaN that an ADDITION made (inf - inf, NaN + 1) is a NaN in both, whatever its sign and payload --
    IEEE 754 leaves those to the machine; every other value, and every NaN that was only moved, must have equal bits."""
    rowptr, col, val = want
    assert res.nnz == len(col) == res.info["nnz_c"], what
    assert np.array_equal(res.rowptr, rowptr), what
    assert np.array_equal(res.colidx, col), what
    assert res.vals.dtype == val.dtype, what
    same = _bits(res.vals) == _bits(val)
    if computed_nans:
        same |= np.isnan(res.vals) & np.isnan(val)
    assert same.all(), what


def _same_arrays(a, b, what=""):
    assert a.shape == b.shape and a.nnz == b.nnz, what
    assert np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.colidx, b.colidx), what
    assert np.array_equal(_bits(a.vals), _bits(b.vals)), what


def _check(mctx, m, n, r, c, v, op, dt, space="host", what="", computed_nans=False):
    """One build against the model: arrays, stats, result info.  Returns the stats."""
    try:
        want, wst, _ = model.build(m, n, r, c, v, op, dt)
    except model.BuildError as e:
        with pytest.raises(S.OspError) as ei:
            mctx.build(m, n, r, c, v, dup=op, dtype=dt, space=space)
        assert ei.value.status == e.status, what
        return None
    res, st = mctx.build(m, n, r, c, v, dup=op, dtype=dt, space=space)
    try:
        what = (what, op, np.dtype(dt).name, st)
        assert res.shape == (m, n) and res.dtype == dt, what
        _assert_same(res, want, what, computed_nans)
        assert {k: st[k] for k in wst} == wst, (what, wst)
        assert st["ms_total"] >= 0
        info = res.info
        named = {"M": m, "N": n, "row_begin": 0, "row_end": m, "nnz_c": res.nnz, "dtype": _lib.OSP_F32 if dt == np.float32 else _lib.OSP_F64}
        assert all(info[k] == x for k, x in named.items()), what
        assert all(info[k] == 0 for k in info if k not in named and k not in ("ms_total", "rank_atomic", "dense_atomic")), what
    finally:
        res.close()
    return st


def _idx(a):
    """An index list as a device tensor (int32 holds a uint32 list's bits)."""
    return am._dev(np.asarray(a, np.uint32))


# ---- every operator on the built list -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_every_operator_equals_the_model_on_the_built_list(mctx, op, dt):
    r, c, lay = _built()
    st = _check(mctx, M, N, r, c, _values(dt), op, dt)
    if op == "error":
        assert st is None                                                 # the list repeats coordinates: status 233
    elif op in ("plus", "min", "max"):
        assert st["long_runs"] == sum(k > L for k in RUNS) == 5 and st["readbacks"] == 2
    else:
        assert st["long_runs"] == 0 and st["readbacks"] == 1


@pytest.mark.parametrize("dt", DTYPES)
def test_lists_without_values_hold_ones(mctx, dt):
    r, c, lay = _built()
    for op in OPS[1:]:
        st = _check(mctx, M, N, r, c, None, op, dt)
        assert st["long_runs"] == 0 and st["readbacks"] == 1
    # COUNT reads no value: with values it gives the same
    a, _ = mctx.build(M, N, r, c, _values(dt), dup="count", dtype=dt)
    b, _ = mctx.build(M, N, r, c, None, dup="count", dtype=dt)
    try:
        _same_arrays(a, b)
        assert a.vals.max() == 20000
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_result_does_not_depend_on_where_a_run_lies(mctx, dt):
    """The same runs behind 0 to 70 entries of an earlier row: every run's place in the sorted order, in its word and in its
    chunk moves, its value does not."""
    r, c, _ = _built()
    v = _values(dt)
    first = None
    for shift in (0, 1, 37, 64, 70):
        rr = np.concatenate([np.zeros(shift, np.int64), r])
        cc = np.concatenate([np.arange(shift, dtype=np.int64), c])
        vv = np.concatenate([np.ones(shift, dt), v])
        res, st = mctx.build(M, N, rr, cc, vv, dup="plus", dtype=dt)
        got = (res.colidx[shift:].copy(), _bits(res.vals)[shift:].copy())
        res.close()
        assert st["nnz_out"] == len(got[0]) + shift
        if first is None:
            first = got
            want = model.build(M, N, r, c, v, "plus", dt)[0]
            assert np.array_equal(got[0], want[1]) and np.array_equal(got[1], _bits(want[2]))
        else:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), shift


# ---- special values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_special_values(mctx, dt):
    sp_ = am._special(dt)                       # NaNs with payloads, infinities, both zeros, denormals, the largest number, 1
    table = np.concatenate([sp_, np.array([1, 2, 3], dt)])      # (values are taken from it by index: their bits are copied)
    QNAN, SNAN, PINF, NINF, NEG0, POS0, DEN, NDEN, BIG = 0, 1, 2, 3, 4, 5, 6, 7, 9
    ONE, TWO, THREE = len(sp_), len(sp_) + 1, len(sp_) + 2
    runs = [[k] for k in range(len(sp_))]       # alone at a coordinate: the bits stay, under every operator
    runs += [[QNAN, ONE, TWO], [ONE, SNAN, TWO], [TWO, QNAN, ONE], [ONE, TWO, QNAN],     # a NaN first, in the middle, last
             [NEG0, POS0], [POS0, NEG0], [NEG0, POS0, NEG0],                             # ties of the zeros
             [PINF, NINF], [NINF, ONE, PINF], [DEN, NDEN], [DEN, DEN], [BIG, BIG],       # inf - inf, denormals, overflow
             [THREE, ONE, TWO], [ONE] * (L + 3) + [QNAN] + [TWO] * 5]                    # ... and a NaN inside a wave's fold
    rows = np.concatenate([[1 + k % 7] * len(run) for k, run in enumerate(runs)])
    cols = np.concatenate([[k] * len(run) for k, run in enumerate(runs)])
    vals = table[np.concatenate(runs)]
    assert np.array_equal(_bits(vals[:len(sp_)]), _bits(sp_))
    # interleave the runs (a stable shuffle of the coordinates: each run keeps its own order)
    order = np.argsort(np.random.default_rng(33).integers(0, 5, len(rows)), kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    tr, tc, tv = _idx(rows), _idx(cols), am._dev(vals)
    torch.cuda.synchronize(DEV)
    for op in OPS[1:]:
        _check(mctx, 9, len(runs), rows, cols, vals, op, dt, computed_nans=op == "plus")
        want = model.build(9, len(runs), rows, cols, vals, op, dt)[0]
        res, _ = mctx.build(9, len(runs), tr, tc, tv, dup=op, dtype=dt, space="device")
        try:
            _assert_same(res, want, (op, "device"), computed_nans=op == "plus")
            pos = {int(cc): i for i, cc in enumerate(res.colidx)}
            if op != "count":                   # alone at its coordinate: the bits, whatever the operator
                assert all(_bits(res.vals)[pos[k]] == _bits(sp_)[k] for k in range(len(sp_))), op
        finally:
            res.close()
    # what the model says about the cases above, spelled out for MIN and MAX
    for op in ("min", "max"):
        _, col, val = model.build(9, len(runs), rows, cols, vals, op, dt)[0]
        at = {int(cc): i for i, cc in enumerate(col)}
        k0 = len(sp_)
        assert _bits(val)[at[k0]] == _bits(sp_)[QNAN]                                      # a NaN first stays
        assert val[at[k0 + 1]] == (1 if op == "min" else 2)                               # a NaN in the middle is skipped
        assert _bits(val)[at[k0 + 4]] == _bits(sp_)[NEG0] and _bits(val)[at[k0 + 5]] == 0  # the earlier zero stays


# ---- the sort's boundaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_list_lengths_around_the_radix_tile(mctx, nnz):
    assert SORT_TILE == 8192
    rng = np.random.default_rng(34 + nnz)
    r, c = rng.integers(0, 40, nnz), rng.integers(0, 150, nnz)             # 6000 coordinates: most repeat
    v = rng.standard_normal(nnz)
    for op, dt in (("plus", np.float64), ("last", np.float32), ("min", np.float32)):
        _check(mctx, 40, 150, r, c, v.astype(dt), op, dt, what=nnz)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 65537])
def test_shapes_around_the_digit_counts(mctx, m):
    """A dimension of 256 sorts one 8-bit digit, 257 two, 65 537 three: rows and columns alike."""
    rng = np.random.default_rng(35 + m)
    for n in (1, 255, 256, 257, 65537):
        nnz = 3000
        r, c = rng.integers(0, m, nnz), rng.integers(0, n, nnz)
        r[:4], c[:4] = m - 1, n - 1                                        # the largest index of each, four times
        r[4], c[4] = 0, 0
        v = rng.standard_normal(nnz)
        st = _check(mctx, m, n, r, c, v, "plus", np.float64, what=(m, n))
        passes = sum(1 if d <= 256 else 2 if d <= 65536 else 3 for d in (m, n))
        assert st["launches"] == 1 + passes * 3 + 3 + 2 + 2, (m, n, st)


# ---- host lists, device tensors, bare addresses -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_host_and_device_lists_give_equal_arrays(mctx, dt):
    r, c, _ = _built()
    v = _values(dt)
    tr, tc, tv = _idx(r), _idx(c), am._dev(v)
    torch.cuda.synchronize(DEV)
    for op in ("plus", "first", "count"):
        a, sa = mctx.build(M, N, r, c, v, dup=op, dtype=dt, space="host")
        b, sb = mctx.build(M, N, tr, tc, tv, dup=op, dtype=dt, space="device")
        c_, sc = mctx.build(M, N, (tr.data_ptr(), tr.numel()), (tc.data_ptr(), tc.numel()), tv.data_ptr(), dup=op, dtype=dt, space="device")
        d, sd = mctx.build(M, N, tr, tc, None, dup=op, dtype=dt, space="device")
        try:
            _assert_same(a, model.build(M, N, r, c, v, op, dt)[0])
            _same_arrays(a, b)
            _same_arrays(a, c_)
            _assert_same(d, model.build(M, N, r, c, None, op, dt)[0])
            assert {k: x for k, x in sa.items() if k != "ms_total"} == {k: x for k, x in sb.items() if k != "ms_total"} \
                == {k: x for k, x in sc.items() if k != "ms_total"}
        finally:
            for x in (a, b, c_, d):
                x.close()
    with pytest.raises(S.OspError) as ei:                                  # device values must be of dtype already
        mctx.build(M, N, tr, tc, am._dev(v.astype(np.float32 if dt == np.float64 else np.float64)), dup="plus", dtype=dt, space="device")
    assert ei.value.status == _lib.ERR_ARG


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(mctx, m, n, rows, cols, vals, space, dup, nnz=None, reserved=None, dtype=_lib.OSP_F64):
    """osp_csr_build called directly: (status, out and stats untouched) on an error, (0, handle) otherwise."""
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.BuildStats()
    st.nnz_in = 77
    b = _lib.Build()
    ptr = lambda a: None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()   # noqa: E731
    b.M, b.N, b.nnz = m, n, len(rows) if nnz is None else nnz
    b.rows, b.cols, b.vals = ptr(rows), ptr(cols), ptr(vals)
    b.dtype, b.space, b.dup = dtype, space, dup
    if reserved is not None:
        b.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_build(mctx._h, ctypes.byref(b), ctypes.byref(o), ctypes.byref(st))
    if rc == 0:
        return rc, o
    return rc, o.value == sentinel and st.nnz_in == 77


BAD_LISTS = {"a row equal to M": ([3, M, 5], [1, 2, 3]), "a column equal to N": ([3, 4, 5], [1, N, 3]),
             "the largest index as a row": ([3, 0xffffffff], [1, 2]), "the largest index as a column": ([3, 4], [0xffffffff, 2]),
             "the largest index twice": ([0xffffffff, 0xffffffff], [0xffffffff, 0xffffffff]),
             "a bad row and a repeated coordinate": ([3, 3, M], [1, 1, 0])}


@pytest.mark.parametrize("space", ["host", "device"])
def test_bad_lists_are_refused_with_out_and_stats_untouched(mctx, space):
    """(tests/test_build_cpu.py and the kernels' own text come first: an index is a key of the sort, compared in
    build_heads_kernel and never used as an address; what is used as one is the sort's permutation, which is below nnz.)"""
    sp_ = _lib.OSP_HOST if space == "host" else _lib.OSP_DEVICE
    PLUS, ERROR = _lib.DUP_OPS["plus"], _lib.DUP_OPS["error"]

    def arr(a, dt=np.uint32):
        a = np.array(a, dt)
        return a if space == "host" else am._dev(a)

    for name, (rr, cc) in BAD_LISTS.items():
        for dup in (PLUS, ERROR):
            rows, cols, vals = arr(rr), arr(cc), arr(np.ones(len(rr)), np.float64)
            if space == "device":
                torch.cuda.synchronize(DEV)
            assert _raw(mctx, M, N, rows, cols, vals, sp_, dup) == (_lib.ERR_RANGE, True), name
            assert _lib.lib().osp_last_error_string()
    rows, cols, vals = arr([1, 2, 1]), arr([5, 5, 5]), arr([1.0, 2.0, 3.0], np.float64)
    good_r, good_c = arr([1, 2, 1]), arr([5, 5, 6])
    if space == "device":
        torch.cuda.synchronize(DEV)
    assert _raw(mctx, M, N, rows, cols, vals, sp_, ERROR) == (_lib.ERR_DUPLICATE, True)       # one repeated coordinate: 233
    assert _lib.ERR_DUPLICATE == 233
    rc, o = _raw(mctx, M, N, good_r, good_c, vals, sp_, ERROR)                                # and without one it succeeds
    assert rc == 0
    got = S.CsrResult(mctx, o)
    _assert_same(got, model.build(M, N, [1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0], "error")[0])
    got.close()
    for word in range(7):
        assert _raw(mctx, M, N, rows, cols, vals, sp_, PLUS, reserved=word) == (_lib.ERR_ARG, True)
    for dup in (7, -1, 99):
        assert _raw(mctx, M, N, rows, cols, vals, sp_, dup) == (_lib.ERR_ARG, True)
    assert _raw(mctx, M, N, rows, cols, vals, 99, PLUS) == (_lib.ERR_ARG, True)
    assert _raw(mctx, M, N, rows, cols, vals, sp_, PLUS, dtype=5) == (_lib.ERR_ARG, True)
    assert _raw(mctx, 0xffffffff, N, rows, cols, vals, sp_, PLUS) == (_lib.ERR_ARG, True)
    assert _raw(mctx, M, 1 << 32, rows, cols, vals, sp_, PLUS) == (_lib.ERR_ARG, True)
    assert _raw(mctx, M, N, rows, cols, vals, sp_, PLUS, nnz=0xffffffff) == (_lib.ERR_ARG, True)
    assert _raw(mctx, M, N, None, cols, vals, sp_, PLUS, nnz=3) == (_lib.ERR_ARG, True)
    assert _raw(mctx, M, N, rows, None, vals, sp_, PLUS, nnz=3) == (_lib.ERR_ARG, True)
    rc, o = _raw(mctx, M, N, rows, cols, vals, sp_, PLUS)                                     # the context works after every refusal
    assert rc == 0
    got = S.CsrResult(mctx, o)
    _assert_same(got, model.build(M, N, [1, 2, 1], [5, 5, 5], [1.0, 2.0, 3.0], "plus")[0])
    got.close()
    if space == "host":                                                                       # the Python entry says the same
        for rr, cc, status in (([M], [0], _lib.ERR_RANGE), ([0], [N], _lib.ERR_RANGE), ([1, 1], [2, 2], _lib.ERR_DUPLICATE)):
            with pytest.raises(S.OspError) as ei:
                mctx.build(M, N, rr, cc, dup="error")
            assert ei.value.status == status


def test_empty_shapes_launch_nothing_and_read_no_list(mctx):
    bad = np.array([0xffffffff, 7], np.int64)
    for dt in DTYPES:
        for m, n, rr, cc in ((0, 5, bad, bad), (5, 0, bad, bad), (0, 0, bad, bad), (5, 7, [], [])):
            for op in OPS:
                res, st = mctx.build(m, n, rr, cc, dup=op, dtype=dt)
                try:
                    assert res.shape == (m, n) and res.nnz == 0 and res.dtype == dt
                    assert np.array_equal(res.rowptr, np.zeros(m + 1, np.int64)) and len(res.colidx) == 0 and len(res.vals) == 0
                    assert (st["nnz_in"], st["nnz_out"], st["long_runs"], st["launches"], st["readbacks"]) == (len(rr), 0, 0, 0, 0)
                    assert model.build(m, n, rr, cc, None, op, dt)[1] == {k: st[k] for k in st if k != "ms_total"}
                finally:
                    res.close()
    # null lists with no entry, and an empty result is an operand like any other
    rc, o = _raw(mctx, 5, 7, None, None, None, _lib.OSP_DEVICE, _lib.DUP_OPS["min"], nnz=0)
    assert rc == 0
    e = S.CsrResult(mctx, o)
    t, _ = e.transpose()
    assert t.shape == (7, 5) and t.nnz == 0
    t.close()
    e.close()


# ---- chaining, pool --------------------------------------------------------------------------------------------------------------------
def _import(mctx, m, n, csr):
    """The model's CSR as a library result through merge_csr_parts_device: the merge of ONE part is the part itself."""
    ts = [am._dev(x) for x in csr]
    torch.cuda.synchronize(DEV)
    res = mctx.merge_csr_parts_device(csr[2].dtype.type, m, n, [tuple(t.data_ptr() for t in ts)])
    del ts
    return res


@pytest.mark.parametrize("dt", DTYPES)
def test_build_chains_with_the_other_operations(mctx, dt):
    n, r, c, v = gen.rmat_coo(8, 8, "g500", seed=7, dtype=dt)
    rng = np.random.default_rng(36)
    again = rng.integers(0, len(r), 700)                                   # 700 entries once more: parallel edges
    r, c = np.concatenate([r, r[again]]).astype(np.int64), np.concatenate([c, c[again]]).astype(np.int64)
    v = np.concatenate([v, rng.standard_normal(700).astype(dt)])
    p = rng.permutation(len(r))
    r, c, v = r[p], c[p], v[p]
    want = model.build(n, n, r, c, v, "plus", dt)[0]
    made = []
    try:
        A, _ = mctx.build(n, n, r, c, v, dup="plus", dtype=dt)
        made.append(A)
        B = _import(mctx, n, n, want)
        made.append(B)
        _same_arrays(A, B, "the build and the import")
        I, J = rng.integers(0, n, 150), np.sort(rng.choice(n, 100, replace=False))
        x = rng.standard_normal(n).astype(dt)
        for name, op in (("transpose", lambda R: R.transpose()[0]), ("mxm", lambda R: R.mxm(R, "min", "plus")[0]),
                         ("extract", lambda R: R.extract(I, J, space="host")[0]), ("matmul", lambda R: R.matmul(R))):
            a, b = op(A), op(B)
            made += [a, b]
            _same_arrays(a, b, name)
            assert a.nnz > 0
        ya, _ = A.mxv(x, "plus", "times", space="host")
        yb, _ = B.mxv(x, "plus", "times", space="host")
        assert np.array_equal(_bits(ya), _bits(yb))
        # the transpose identity: on a duplicate-free list, build(cols, rows) is the transpose of build(rows, cols)
        u = np.unique(r * n + c)
        ur, uc = (u // n)[::-1].copy(), (u % n)[::-1].copy()              # (descending: nothing is sorted for the library)
        uv = rng.standard_normal(len(u)).astype(dt)
        F, _ = mctx.build(n, n, ur, uc, uv, dup="first", dtype=dt)
        made.append(F)
        Ft, _ = F.transpose()
        made.append(Ft)
        G, _ = mctx.build(n, n, uc, ur, uv, dup="first", dtype=dt)
        made.append(G)
        _same_arrays(G, Ft, "build(cols, rows) and the transpose")
    finally:
        for x_ in made:
            x_.close()


@pytest.mark.parametrize("op", ["plus", "last"])
def test_fifty_back_to_back_calls_give_the_same_arrays_and_the_pool_does_not_grow(mctx, op, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call (the error word and the counter of long runs are zeroed by
    every call), and after the first call no call allocates device memory: the library's own count of pool misses, printed
    under OSP_VERBOSE, as tests/test_gpu_extract.py reads it."""
    r, c, _ = _built()
    v = _values(np.float64)
    tr, tc, tv = _idx(r), _idx(c), am._dev(v)
    torch.cuda.synchronize(DEV)
    want, wst, _ = model.build(M, N, r, c, v, op, np.float64)
    monkeypatch.setenv("OSP_VERBOSE", "1")
    first, misses = None, []
    for i in range(50):
        capfd.readouterr()
        res, st = mctx.build(M, N, tr, tc, tv, dup=op, dtype=np.float64, space="device")
        err = capfd.readouterr().err
        got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy())
        res.close()
        found = re.findall(r"\[osp\] build .*pool misses so far: (\d+) hipMalloc calls", err)
        assert len(found) == 1, err
        misses.append(int(found[0]))
        assert {k: st[k] for k in wst} == wst, i
        if first is None:
            first = got
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], _bits(want[2]))
        else:
            assert all(np.array_equal(x, y) for x, y in zip(got, first)), i
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses
