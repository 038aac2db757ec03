"""osp_csr_transpose on the GPU against tests/transpose_model.py -- row pointers and columns exact, values equal as BITS
(they are moved, never computed: a NaN keeps its payload) -- on both paths, and CsrResult.matmul (the transpose feeding the
outer-product pipeline) against CsrResult.mxm under (PLUS, TIMES) in all three arrays."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import build_model
from tests import semiring_model
from tests import test_gpu_apply_mask as am   # _upload, _bits, _special, _traps only
from tests import transpose_model as model
from tests import vector_model

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
DTYPES = [np.float32, np.float64]
_SORT = open(os.path.join(am.ROOT, "outerspace_amd", "csrc", "osp_sort.h")).read()
# the sort's unit of work: kRsThreads * kRsItems consecutive elements
TILE = int(re.search(r"kRsThreads\s*=\s*(\d+)", _SORT).group(1)) * int(re.search(r"kRsItems\s*=\s*(\d+)", _SORT).group(1))


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
    assert res.vals.dtype == val.dtype and np.array_equal(_bits(res.vals), _bits(val)), what


def _values(nnz, dt, rng):
    """Random values with the special ones (NaN payloads, infinities, both zeros, denormals) at every seventh entry."""
    val = rng.standard_normal(nnz).astype(dt)
    sp_ = am._special(dt)
    val[::7] = np.resize(sp_, len(val[::7]))
    return val


def _csr_of(M, N, keys, dt, rng):
    keys = np.unique(np.asarray(keys, np.int64))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(keys // N, minlength=M))]).astype(np.int64)
    return rowptr, (keys % N).astype(np.uint32), _values(len(keys), dt, rng)


@functools.lru_cache(maxsize=None)
def _built(N, nnz, dt):
    """M x N (M > 64: the sort path) with exactly nnz entries: rows 3 and M - 1 are empty, column 1 is empty (N > 2), an
    entry lies in column 0 and one in column N - 1."""
    rng = np.random.default_rng(N % 1000 + nnz)
    M = 2 * nnz + 70 if N <= 2 else 200
    forced = np.unique([5 * N + 0, 7 * N + N - 1])[:nnz]
    keys = forced
    while len(keys) < nnz:
        k = 2 * nnz + 100
        r, c = rng.integers(0, M, k), rng.integers(0, N, k)
        ok = (r != 3) & (r != M - 1) & ((c != 1) | (N <= 2))
        more = np.setdiff1d(np.unique(r[ok] * N + c[ok]), keys)
        keys = np.concatenate([keys, rng.permutation(more)[:nnz - len(keys)]])
    csr = _csr_of(M, N, keys, dt, rng)
    assert len(csr[1]) == nnz and csr[0][4] == csr[0][3] and csr[1].min() == 0
    assert nnz < 2 or csr[1].max() == N - 1
    return M, csr


@functools.lru_cache(maxsize=None)
def _hub(dt):
    """20 000 rows that all hold column 500 (an output row of 20 000 entries: it spans several sort tiles), and two more
    random columns each."""
    rng = np.random.default_rng(20)
    M, N = 20000, 1000
    r = np.repeat(np.arange(M), 3)
    c = np.concatenate([np.full((M, 1), 500), rng.integers(0, N, (M, 2))], axis=1).ravel()
    return M, N, _csr_of(M, N, r * N + c, dt, rng)


@functools.lru_cache(maxsize=None)
def _rowmask(M, dt, N=1000):
    """M <= 64 rows (65: the first shape beyond the row-mask path): every row holds column 5, the last row columns 0 and
    N - 1, and a few random columns each; row 1 of a longer input is empty but for column 5."""
    rng = np.random.default_rng(100 + M)
    r = np.concatenate([np.arange(M), [M - 1, M - 1], rng.integers(0, M, 40 * M)])
    c = np.concatenate([np.full(M, 5), [0, N - 1], rng.integers(0, N, 40 * M)])
    keep = (r != 1) | (c == 5) | (M <= 2)
    return _csr_of(M, N, r[keep] * N + c[keep], dt, rng)


@functools.lru_cache(maxsize=None)
def _one_long_row(dt):
    """3 x 2^20: row 1 holds 2^19 entries (a frontier), rows 0 and 2 a handful."""
    rng = np.random.default_rng(19)
    N = 1 << 20
    long_ = np.sort(rng.choice(N, 1 << 19, replace=False))
    keys = np.concatenate([[0, 5, N - 1], N + long_, 2 * N + long_[::50000], [2 * N + N - 1]])
    return N, _csr_of(3, N, keys, dt, rng)


def _transpose_and_check(src, csr, N, path, what=""):
    res, st = src.transpose()
    try:
        M = len(csr[0]) - 1
        assert res.shape == (N, M) and res.dtype == csr[2].dtype.type
        _assert_same(res, model.transpose(*csr, N), what)
        nnz = len(csr[1])
        assert (st["nnz"], st["path"]) == (nnz, path), (what, st)
        assert st["passes"] == (model.passes(N) if path == 2 else 0), (what, st)
        assert st["ms_total"] >= 0 and st["launches"] > 0
        info = res.info
        assert (info["M"], info["N"], info["K"], info["row_begin"], info["row_end"]) == (N, M, src.info["K"], 0, N)
        assert (info["nnz_a"], info["nnz_b"], info["nnz_c"], info["partials"]) == (nnz, 0, nnz, 0)
        named = {"M", "K", "N", "row_begin", "row_end", "nnz_a", "nnz_c", "dtype", "ms_total"}
        assert all(v == 0 for k, v in info.items() if k not in named), info
    finally:
        res.close()
    return st


# ---- the sort path ----------------------------------------------------------------------------------------------------------------
# one, two, three and four passes and their edges; an entry count on, below and above the sort's tile and several tiles
SORT_CASES = [(1, TILE), (2, 1), (256, TILE - 1), (257, TILE + 1), (65536, 3 * TILE + 5), (65537, TILE), ((1 << 24) + 3, 3 * TILE + 5)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,nnz", SORT_CASES)
def test_sort_path_equals_the_model(mctx, N, nnz, dt):
    assert TILE == 8192
    M, csr = _built(N, nnz, dt)
    src = _upload(mctx, N, csr)
    try:
        st = _transpose_and_check(src, csr, N, 2, (N, nnz))
        assert st["passes"] == {1: 1, 2: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, (1 << 24) + 3: 4}[N]
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_a_hub_column_spans_several_sort_tiles(mctx, dt):
    M, N, csr = _hub(dt)
    assert np.count_nonzero(csr[1] == 500) == M > 2 * TILE
    src = _upload(mctx, N, csr)
    try:
        _transpose_and_check(src, csr, N, 2)
    finally:
        src.close()


# ---- the row-mask path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,path", [(1, 1), (2, 1), (63, 1), (64, 1), (65, 2)])
def test_row_mask_path_up_to_64_rows(mctx, M, path, dt):
    csr = _rowmask(M, dt)
    src = _upload(mctx, 1000, csr)
    try:
        _transpose_and_check(src, csr, 1000, path, M)
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_row_mask_path_one_row_of_half_a_million_entries(mctx, dt):
    N, csr = _one_long_row(dt)
    src = _upload(mctx, N, csr)
    try:
        _transpose_and_check(src, csr, N, 1)
    finally:
        src.close()


# ---- the launch count -------------------------------------------------------------------------------------------------------------
def _launches(M, N, nnz, gather):
    """Kernels of a call on a non-empty input, as transpose_impl counts them.  Row mask: the mask, the scan of its popcounts,
    the placement.  Sort: the packing of the records (not with the bisecting gather), a histogram, a scan of the histogram
    and a scatter per pass, the row pointer.  The constants come from the sources, as tests/build_model.py reads them."""
    if M <= 64:
        return 1 + build_model._scan_launches(N) + 1
    per_pass = 2 + build_model._scan_launches(-(-nnz // build_model.SORT_TILE) * build_model.RADIX)
    return (0 if gather == "bisect" else 1) + model.passes(N) * per_pass + 1


# entries beyond which the scan of the sort's histogram takes its three-launch form
BIG = build_model.SCAN_SMALL_TILES * build_model.SCAN_TILE // build_model.RADIX * build_model.SORT_TILE


@functools.lru_cache(maxsize=None)
def _counted(M, N, draws):
    if M == 64:
        return _rowmask(64, np.float64)
    rng = np.random.default_rng(N + draws)
    return _csr_of(M, N, np.concatenate([[0, M * N - 1], rng.integers(0, M * N, draws)]), np.float64, rng)


@pytest.mark.parametrize("gather", [None, "bisect"])
@pytest.mark.parametrize("M,N,draws,passes", [(65, 200, 300, 1), (65, 300, 300, 2), (65, 70000, 300, 3), (65, 70000, 2 * BIG, 3),
                                              (64, 1000, 0, 0)])
def test_transpose_reports_its_launches(mctx, monkeypatch, M, N, draws, passes, gather):
    """M = 65 is one row past the row-mask path: about 300 entries sorted in one, two and three passes, and over a million
    in three (the histogram's scan in three launches instead of one); M = 64 takes the row mask, whatever the gather."""
    monkeypatch.delenv("OSP_TRANSPOSE_PATH", raising=False)
    if gather is None:
        monkeypatch.delenv("OSP_TRANSPOSE_GATHER", raising=False)
    else:
        monkeypatch.setenv("OSP_TRANSPOSE_GATHER", gather)
    csr = _counted(M, N, draws)
    nnz = len(csr[1])
    assert M == 64 or 280 <= nnz <= 302 or (draws == 2 * BIG and nnz > BIG)
    src = _upload(mctx, N, csr)
    try:
        st = _transpose_and_check(src, csr, N, 1 if M == 64 else 2, (M, N, gather))
        print("transpose launches", (M, N, draws, gather), st["launches"], st["passes"])
        assert st["passes"] == passes
        assert st["launches"] == _launches(M, N, nnz, gather), (M, N, gather, st)
    finally:
        src.close()


# ---- the same input through every variant -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_variants_agree_on_the_same_input(mctx, monkeypatch, dt):
    """M = 64: the automatic choice (row mask), the sort forced, the sort with the bisecting gather, and the sort of a context
    whose stable ranks come from ballot matching (OSP_RANK=ballot, read when a context is created, as
    tests/test_gpu_parity.py forces it) all give the model's arrays.  The hub input (two passes, an output row over several
    tiles) goes through the two gathers and the ballot ranks as well."""
    csr64 = _rowmask(64, dt)
    M, N, hub = _hub(dt)
    want64, want_hub = model.transpose(*csr64, 1000), model.transpose(*hub, N)

    def run(ctx, csr, ncol, want, path):
        src = _upload(ctx, ncol, csr)
        try:
            res, st = src.transpose()
            try:
                assert st["path"] == path
                _assert_same(res, want, (path, os.environ.get("OSP_TRANSPOSE_GATHER")))
            finally:
                res.close()
        finally:
            src.close()

    run(mctx, csr64, 1000, want64, 1)
    monkeypatch.setenv("OSP_TRANSPOSE_PATH", "rowmask")      # any value but "sort" means automatic
    run(mctx, csr64, 1000, want64, 1)
    run(mctx, hub, N, want_hub, 2)                           # (the row-mask path is never forced beyond 64 rows)
    monkeypatch.setenv("OSP_TRANSPOSE_PATH", "sort")
    run(mctx, csr64, 1000, want64, 2)
    monkeypatch.setenv("OSP_TRANSPOSE_GATHER", "bisect")
    run(mctx, csr64, 1000, want64, 2)
    run(mctx, hub, N, want_hub, 2)
    monkeypatch.setenv("OSP_RANK", "ballot")
    with S.Context(0) as c:
        run(c, csr64, 1000, want64, 2)
        run(c, hub, N, want_hub, 2)
        monkeypatch.delenv("OSP_TRANSPOSE_GATHER")
        run(c, csr64, 1000, want64, 2)
        run(c, hub, N, want_hub, 2)


# ---- involution, reduce -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_transposing_twice_gives_the_input_back(mctx, dt):
    n, r, c, v = gen.rmat_coo(12, 4, "g500", seed=2, dtype=dt)
    prod = mctx.spgemm_coo(n, n, n, (r, c, v), (r, c, v))
    ncol, traps = am._traps(dt)[:2]
    trap = _upload(mctx, ncol, traps)
    try:
        for src, what in ((prod, "rmat12 self-product"), (trap, "traps")):
            t, st = src.transpose()
            tt, st2 = t.transpose()
            try:
                # (the traps have few rows: row mask there, the sort on the way back)
                assert (st["path"], st2["path"]) == ((1 if src.shape[0] <= 64 else 2), 2) and t.shape == src.shape[::-1] and tt.shape == src.shape
                _assert_same(t, model.transpose(src.rowptr, src.colidx, src.vals, src.shape[1]), what)
                _assert_same(tt, (src.rowptr, src.colidx, src.vals), what)
            finally:
                t.close()
                tt.close()
        assert prod.nnz > 8 * TILE
    finally:
        prod.close()
        trap.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_columns_of_the_device_transpose_is_reduce_rows(mctx, dt):
    ncol, csr = am._traps(dt)[:2]
    src = _upload(mctx, ncol, csr)
    tr, _ = src.transpose()
    try:
        for op in vector_model.REDUCE_OPS:
            a, sa = src.reduce("rows", op)
            b, sb = tr.reduce("cols", op)
            assert np.array_equal(_bits(a), _bits(b)), op      # (the same segments in the same order: NaN payloads included)
            assert sa["long_segments"] == sb["long_segments"]
            c, _ = tr.reduce("rows", op)
            d, _ = src.reduce("cols", op)
            assert np.array_equal(_bits(c), _bits(d)), op
    finally:
        src.close()
        tr.close()


# ---- errors and empty cases -----------------------------------------------------------------------------------------------------------
def _raw(r, tp, out=True, stats=True):
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.TransposeStats()
    st.nnz = 77
    rc = _lib.lib().osp_csr_transpose(r._h if r is not None else None, ctypes.byref(tp) if tp is not None else None,
                                      ctypes.byref(o) if out else None, ctypes.byref(st) if stats else None)
    if rc == 0:
        return rc, o
    return rc, o.value == sentinel and st.nnz == 77


def test_argument_errors(mctx):
    """Every refusal that can be built: a null in or out, a non-zero reserved word, a result of osp_spgemm_partials.  (An
    operand of 2^32 - 1 entries and one of more than 2^32 rows -- OSP_ERR_DIM -- cannot be made: every function that makes a
    result refuses those sizes itself.)"""
    rowptr = np.array([0, 2, 3, 3, 3], np.int64)
    col, val = np.array([0, 3, 1], np.uint32), np.array([1.0, 2.0, 3.0])
    res = mctx.merge_csr_parts(4, 5, [(rowptr, col, val)])
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    acsc, bcsr = gen.coo_to_csc(n, r, c, v), gen.coo_to_csr(n, c, r, v)
    ts = [am._dev(x) for x in acsc + bcsr]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        assert _raw(None, _lib.Transpose()) == (_lib.ERR_ARG, True)
        assert _raw(res, _lib.Transpose(), out=False)[0] == _lib.ERR_ARG
        assert _raw(part, None) == (_lib.ERR_ARG, True)
        assert _lib.lib().osp_last_error_string()
        for word in range(8):
            tp = _lib.Transpose()
            tp.reserved[word] = 1
            assert _raw(res, tp) == (_lib.ERR_ARG, True)
        # a null tp and null stats are legal
        for tp, stats in ((None, True), (_lib.Transpose(), False), (None, False)):
            rc, o = _raw(res, tp, stats=stats)
            assert rc == 0
            got = S.CsrResult(mctx, o)
            _assert_same(got, model.transpose(rowptr, col, val, 5))
            got.close()
    finally:
        res.close()
        part.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_inputs_launch_nothing(mctx, dt):
    none = (np.zeros(0, np.uint32), np.zeros(0, dt))
    for M, N in ((0, 5), (5, 0), (0, 0), (3, 4), (100, 70)):
        src = _upload(mctx, N, (np.zeros(M + 1, np.int64),) + none)
        try:
            res, st = src.transpose()
            try:
                assert res.shape == (N, M) and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(N + 1, np.int64)), (M, N)
                assert (st["nnz"], st["path"], st["passes"], st["launches"]) == (0, 0, 0, 0), (M, N)
                back, st2 = res.transpose()                  # an empty result is an operand like any other
                assert back.shape == (M, N) and back.nnz == 0 and st2["launches"] == 0
                back.close()
            finally:
                res.close()
        finally:
            src.close()


# ---- chaining, pool -----------------------------------------------------------------------------------------------------------------
def test_the_transpose_is_an_operand_of_every_operation(mctx):
    n, r, c, v = gen.rmat_coo(8, 8, "g500", seed=6)
    g = gen.coo_to_csr(n, r, c, v)
    src = _upload(mctx, n, g)
    made = []
    try:
        T, _ = src.transpose()
        made.append(T)
        want = model.transpose(*g, n)
        _assert_same(T, want)
        trow = np.repeat(np.arange(n), np.diff(want[0]))
        sel, _ = T.select("offdiag")
        made.append(sel)
        off = trow != want[1]
        assert sel.nnz == int(off.sum()) and np.array_equal(sel.colidx, want[1][off]) and np.array_equal(_bits(sel.vals), _bits(want[2][off]))
        both, _ = T.intersect(src, "first")                  # the edges that run both ways, T's values
        made.append(both)
        tk, sk = trow * n + want[1], np.repeat(np.arange(n), np.diff(g[0])) * n + g[1]
        common = np.isin(tk, sk)
        assert both.nnz == int(common.sum()) > 0 and np.array_equal(_bits(both.vals), _bits(want[2][common]))
        msk, _ = T.apply_mask(src)
        made.append(msk)
        assert np.array_equal(msk.rowptr, both.rowptr) and np.array_equal(msk.colidx, both.colidx)
        un, _ = T.union(src, "plus")
        made.append(un)
        assert un.nnz == len(np.union1d(tk, sk))
        P, _ = T.mxm(src, "min", "plus")
        made.append(P)
        wp = semiring_model.mxm(want, g, n, "min", "plus")[0]
        assert np.array_equal(P.rowptr, wp[0]) and np.array_equal(P.colidx, wp[1]) and np.array_equal(_bits(P.vals), _bits(wp[2]))
        PT, st = P.transpose()
        made.append(PT)
        _assert_same(PT, model.transpose(*wp, n))
        back, _ = T.transpose()
        made.append(back)
        _assert_same(back, g)
        assert np.array_equal(src.rowptr, g[0]) and np.array_equal(_bits(src.vals), _bits(g[2]))     # the operand stays valid
    finally:
        for x in made:
            x.close()
        src.close()


@pytest.mark.parametrize("which", ["sort", "rowmask"])
def test_fifty_back_to_back_calls_give_the_same_arrays_and_the_pool_does_not_grow(mctx, which, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call (the row masks are zeroed by every call), and after the first
    call no call allocates device memory: the library's own count of pool misses, printed under OSP_VERBOSE, as
    tests/test_gpu_mxm.py reads it."""
    if which == "sort":
        M, N, csr = _hub(np.float64)
    else:
        N, csr = 1000, _rowmask(64, np.float64)
    src = _upload(mctx, N, csr)
    monkeypatch.setenv("OSP_VERBOSE", "1")
    first, misses = None, []
    try:
        for i in range(50):
            capfd.readouterr()
            res, st = src.transpose()
            err = capfd.readouterr().err
            got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy(), st["path"])
            res.close()
            found = re.findall(r"\[osp\] transpose .*pool misses so far: (\d+) hipMalloc calls", err)
            assert len(found) == 1, err
            misses.append(int(found[0]))
            if first is None:
                first = got
                _w = model.transpose(*csr, N)
                assert np.array_equal(got[0], _w[0]) and np.array_equal(got[1], _w[1]) and np.array_equal(got[2], _bits(_w[2]))
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, first)), i
    finally:
        src.close()
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses


# ---- matmul: the transpose feeds the outer-product pipeline ---------------------------------------------------------------------------
def _same_arrays(a, b, what=""):
    assert a.shape == b.shape and a.nnz == b.nnz, what
    assert np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.colidx, b.colidx), what
    assert np.array_equal(_bits(a.vals), _bits(b.vals)), what


def _random_csr(M, N, per_row, dt, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, per_row, M)
    lens[M // 2] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, k, replace=False)) for k in lens]).astype(np.uint32)
    return rowptr, col, rng.standard_normal(len(col)).astype(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_matmul_is_mxm_plus_times_in_all_three_arrays(mctx, dt):
    n, r, c, v = gen.rmat_coo(10, 16, "g500", seed=1, dtype=dt)
    A = _upload(mctx, n, gen.coo_to_csr(n, r, c, v))
    F = _upload(mctx, 4096, _random_csr(64, 4096, 200, dt, 3))        # 64 x 4096: the transpose takes the row-mask path
    G = _upload(mctx, 300, _random_csr(4096, 300, 12, dt, 4))         # 4096 x 300
    H = _upload(mctx, 300, _random_csr(64, 300, 40, dt, 5))           # 64 x 300
    made = []
    try:
        for a, b, what in ((A, A, "rmat10 self-product, the same handle on both sides"), (F, G, "64 x 4096 times 4096 x 300")):
            got = a.matmul(b)
            made.append(got)
            want, _ = a.mxm(b)
            made.append(want)
            assert got.nnz > 0 and got.shape == (a.shape[0], b.shape[1])
            _same_arrays(got, want, what)
        chain = made[2].matmul(made[2], self_transposed=True)         # (F G)^T (F G): a product is an operand of the next
        made.append(chain)
        fgt, _ = made[2].transpose()
        made.append(fgt)
        want, _ = fgt.mxm(made[2])
        made.append(want)
        _same_arrays(chain, want, "chain")
        for a, b, what in ((A, A, "A^T A"), (F, H, "F^T H")):
            got = a.matmul(b, self_transposed=True)
            made.append(got)
            at, _ = a.transpose()
            made.append(at)
            want, _ = at.mxm(b)
            made.append(want)
            assert got.nnz > 0 and got.shape == (a.shape[1], b.shape[1])
            _same_arrays(got, want, what)
        assert np.array_equal(A.colidx, gen.coo_to_csr(n, r, c, v)[1])           # the operands stay valid
    finally:
        for x in made + [A, F, G, H]:
            x.close()


def test_matmul_refuses_mismatched_operands(mctx):
    rowptr = np.array([0, 2, 3, 3, 3], np.int64)
    col, val = np.array([0, 3, 1], np.uint32), np.array([1.0, 2.0, 3.0])
    res = mctx.merge_csr_parts(4, 4, [(rowptr, col, val)])
    f32 = mctx.merge_csr_parts(4, 4, [(rowptr, col, val.astype(np.float32))])
    wide = mctx.merge_csr_parts(4, 5, [(rowptr, col, val)])
    other = S.Context(0)
    try:
        foreign = other.merge_csr_parts(4, 4, [(rowptr, col, val)])
        for bad in (f32, foreign):
            for kw in ({}, {"self_transposed": True}):
                with pytest.raises(S.OspError) as ei:
                    res.matmul(bad, **kw)
                assert ei.value.status == _lib.ERR_ARG
        with pytest.raises(S.OspError) as ei:
            wide.matmul(res)                                  # 4 x 5 times 4 x 4
        assert ei.value.status == _lib.ERR_DIM
        tall, _ = wide.transpose()                            # 5 x 4: as self^T its inner dimension is 5, res has 4 rows
        with pytest.raises(S.OspError) as ei:
            tall.matmul(res, self_transposed=True)
        assert ei.value.status == _lib.ERR_DIM
        tall.close()
        with pytest.raises(TypeError):
            res.matmul(val)
        ok = wide.matmul(res, self_transposed=True)           # (4 x 5)^T times 4 x 4
        assert ok.shape == (5, 4)
        ok.close()
        foreign.close()
    finally:
        other.close()
        for x in (res, f32, wide):
            x.close()
