"""osp_csr_assign on the GPU against tests/assign_model.py -- row pointers and columns exact, moved values equal as BITS,
computed values as tests/test_gpu_ewise.py compares them (bits equal where the model's result is no NaN, a NaN where it is)
-- for every pair of a row list and a column list on the built matrix of tests/test_gpu_extract.py with three kinds of a,
every accum operator, host and device lists, the composed column path against scipy, the two identities that tie it to
extract, embeddings, its refusals (host and device lists, `out` untouched), the no-work shapes, chaining with the other result
operations, 2^32 - 1 columns, and the pool."""
import ctypes
import re

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import assign_model as model
from tests import extract_model
from tests import mxv_model
from tests import semiring_model
from tests import wide_columns as W
from tests import test_assign_cpu as cpu           # _scipy_assign only
from tests import test_gpu_apply_mask as am        # _upload, _bits, _special, _dev only
from tests import test_gpu_extract as ge           # the built matrix c and its upload only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits, _upload = am._bits, am._upload
DTYPES = [np.float32, np.float64]
M, N, QUIET = ge.M, ge.N, ge.QUIET
STAT_KEYS = ("nnz_c", "nnz_a", "nnz_region", "nnz_both", "nnz_out", "readbacks")


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _row_lists():
    return {"none": None, "identity": np.arange(M), "reversed": np.arange(M)[::-1], "the full row": np.array([80]),
            "empty rows first and last": np.array([70, 10, 0, 299, 60]), "empty": np.zeros(0, np.int64)}


def _col_lists():
    return {"none": None, "all": np.arange(N), "first": np.array([0]), "last": np.array([N - 1]), "63 64": np.array([63, 64]),
            "every 64th": np.arange(0, N, 64), "quiet": QUIET, "empty": np.zeros(0, np.int64)}


def _csr_of_dense(has, dt, seed):
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int64)
    col = np.nonzero(has)[1].astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    at = np.arange(0, len(val), 7)                      # the special values at every seventh entry
    val[at] = np.resize(np.roll(am._special(dt), 4), len(at))
    return rowptr, col, val


def _variants(csr, I, J, dt, seed):
    """The three a of a pair of lists, as (rowptr, col, val): about 30 % dense with a full and an empty row, empty, and the
    pattern of c(I, J) itself."""
    m, n = M if I is None else len(I), N if J is None else len(J)
    rng = np.random.default_rng(seed)
    has = rng.random((m, n)) < 0.3
    if m:
        has[0] = True
        has[m - 1] = False
    hit_ptr, hit_col, _ = extract_model.extract(*csr, N, I, J)[0]
    hits = (hit_ptr, hit_col, _csr_of_dense(np.ones((1, len(hit_col)), bool), dt, seed + 2)[2])
    return {"dense": _csr_of_dense(has, dt, seed + 1), "empty": (np.zeros(m + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt)),
            "hits": hits}, (m, n)


def _build(mctx, a, shape, dt):
    """a as a library result through ``Context.build``: a coordinate given once keeps its value's bits."""
    rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(a[0]))
    res, _ = mctx.build(shape[0], shape[1], rows, a[1], a[2], dup="error", dtype=dt, space="host")
    assert res.shape == shape and np.array_equal(res.rowptr, a[0]) and np.array_equal(_bits(res.vals), _bits(a[2]))
    return res


def _assert_values(got, want, computed, accum):
    gb, wb = _bits(got), _bits(want)
    if accum is None or accum in model.COPY_OPS:
        assert np.array_equal(gb, wb)
        return
    nan = computed & np.isnan(want)
    assert np.array_equal(gb[~nan], wb[~nan])
    assert np.isnan(got[nan]).all()


def _check(res, st, src, want, accum, what=""):
    (rowptr, col, val), computed, wst = want
    assert res.shape == src.shape and res.dtype == src.dtype, what
    assert res.nnz == len(col) == res.info["nnz_c"], what
    assert np.array_equal(res.rowptr, rowptr), what
    assert np.array_equal(res.colidx, col), what
    assert res.vals.dtype == val.dtype, what
    _assert_values(res.vals, val, computed, accum)
    if wst is not None:
        print(what, {k: st[k] for k in STAT_KEYS}, "launches", st["launches"])
        assert {k: st[k] for k in STAT_KEYS} == {k: wst[k] for k in STAT_KEYS}, (what, st, wst)
        assert (st["launches"] == 0) == wst["no_work"] and st["ms_total"] >= 0 and not st["composed"], (what, st)
    info = res.info
    assert all(info[k] == src.info[k] for k in info if k not in ("nnz_c", "ms_total")), what      # c's, but for the two


# ---- every pair of lists, without accum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rn", list(_row_lists()))
def test_every_pair_of_lists_equals_the_model(mctx, rn, dt):
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    I = _row_lists()[rn]
    try:
        for k, (cn, J) in enumerate(_col_lists().items()):
            variants, shape = _variants(csr, I, J, dt, 100 + k)
            for vn, a in variants.items():
                A = _build(mctx, a, shape, dt)
                res = None
                try:
                    res, st = src.assign(A, I, J, space="host")
                    _check(res, st, src, model.assign(csr, N, a, shape[1], I, J), None, (rn, cn, vn))
                    if vn == "hits" and shape[0] and shape[1] and not (I is None and J is None):
                        assert st["nnz_both"] == st["nnz_region"] == len(a[1]) and res.nnz == src.nnz
                finally:
                    A.close()
                    if res is not None:
                        res.close()
        assert np.array_equal(src.rowptr, csr[0]) and np.array_equal(_bits(src.vals), _bits(csr[2]))     # c stays valid
    finally:
        src.close()


# ---- every accum operator -------------------------------------------------------------------------------------------------------------
ACCUM_PAIRS = {"reversed, every 64th": ("reversed", "every 64th"), "the full row, all": ("the full row", "all"), "none, none": ("none", "none"),
               "empty rows first and last, quiet": ("empty rows first and last", "quiet")}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("accum", model.ACCUM_OPS)
def test_every_accum_operator_equals_the_model(mctx, accum, dt):
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    try:
        for k, (name, (rn, cn)) in enumerate(ACCUM_PAIRS.items()):
            I, J = _row_lists()[rn], _col_lists()[cn]
            variants, shape = _variants(csr, I, J, dt, 200 + k)
            for vn, a in variants.items():
                A = _build(mctx, a, shape, dt)
                res = None
                try:
                    res, st = src.assign(A, I, J, accum, space="host")
                    want = model.assign(csr, N, a, shape[1], I, J, accum)
                    _check(res, st, src, want, accum, (name, vn, accum))
                    if vn == "hits":
                        assert st["nnz_both"] == len(a[1]) == int(want[1].sum()) and res.nnz == src.nnz
                finally:
                    A.close()
                    if res is not None:
                        res.close()
    finally:
        src.close()


def test_second_is_not_no_accum(mctx):
    dt = np.float64
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    I, J = np.array([80, 70]), np.arange(0, N, 2)
    a = (np.array([0, 1, 1], np.int64), np.array([5], np.uint32), np.array([2.5]))
    A = _build(mctx, a, (2, len(J)), dt)
    try:
        plain, st0 = src.assign(A, I, J, None, space="host")
        second, st1 = src.assign(A, I, J, "second", space="host")
        assert st0["nnz_region"] == st1["nnz_region"] > 2000
        assert plain.nnz == src.nnz - st0["nnz_region"] + 1 and second.nnz == src.nnz + 1 - st1["nnz_both"]
        _check(second, st1, src, model.assign(csr, N, a, len(J), I, J, "second"), "second")
        plain.close()
        second.close()
    finally:
        A.close()
        src.close()


# ---- the three spaces of a list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_host_lists_device_tensors_and_bare_addresses_give_equal_arrays(mctx, dt):
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    rng = np.random.default_rng(31)
    I = rng.permutation(M)[:200]
    J = np.sort(rng.choice(N, 1200, replace=False))
    ti, tj = ge._idx(I), ge._idx(J)
    torch.cuda.synchronize(DEV)
    try:
        for rows_h, cols_h, rows_d, cols_d in ((I, J, ti, tj), (I, None, ti, None), (None, J, None, tj)):
            variants, shape = _variants(csr, rows_h, cols_h, dt, 300)
            A = _build(mctx, variants["dense"], shape, dt)
            for accum in (None, "plus"):
                a, sa = src.assign(A, rows_h, cols_h, accum, space="host")
                b, sb = src.assign(A, rows_d, cols_d, accum)                      # space="device" is the default
                c, sc = src.assign(A, None if rows_d is None else (rows_d.data_ptr(), rows_d.numel()),
                                   None if cols_d is None else (cols_d.data_ptr(), cols_d.numel()), accum)   # bare addresses
                try:
                    _check(a, sa, src, model.assign(csr, N, variants["dense"], shape[1], rows_h, cols_h, accum), accum)
                    ge._same_arrays(a, b)
                    ge._same_arrays(a, c)
                    keys = STAT_KEYS + ("launches",)
                    assert [sa[k] for k in keys] == [sb[k] for k in keys] == [sc[k] for k in keys]
                finally:
                    for x in (a, b, c):
                        x.close()
            A.close()
    finally:
        src.close()


# ---- general column lists: the composed path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("space", ["host", "device"])
def test_the_composed_column_path_matches_scipy(mctx, dt, space):
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    rng = np.random.default_rng(32)
    # (scipy's side assigns the region densely through lil: the regions are kept to a few hundred thousand coordinates)
    cases = {"a permutation of every column": (rng.permutation(M)[:60], rng.permutation(N)), "no rows": (None, rng.permutation(N)[:300]),
             "reversed both": (np.arange(M)[::-1][:100], np.arange(N)[::-1]), "a few": (np.array([80, 3, 70]), rng.permutation(N)[:700])}
    try:
        for name, (I, J) in cases.items():
            variants, shape = _variants(csr, I, np.sort(J), dt, 400)
            a = variants["dense"]
            A = _build(mctx, a, shape, dt)
            if space == "device":
                rows, cols = None if I is None else ge._idx(I), ge._idx(J)
                torch.cuda.synchronize(DEV)
            else:
                rows, cols = I, J
            try:
                for accum in (None, "plus"):
                    res, st = src.assign(A, rows, cols, accum, space=space)
                    try:
                        assert st["composed"] and st["ms_total"] > 0 and st["nnz_out"] == res.nnz, name
                        want, computed = model.assign_any(csr, N, a, shape[1], I, J, accum)
                        _check(res, st, src, (want, computed, None), accum, name)
                        wp, wc, pc, pa = cpu._scipy_assign(csr, N, a, I, J, accum)
                        assert np.array_equal(res.rowptr, wp) and np.array_equal(res.colidx, wc), name
                        only_c, only_a = (pc >= 0) & (pa < 0), (pa >= 0) & (pc < 0)
                        assert np.array_equal(_bits(res.vals[only_c]), _bits(csr[2][pc[only_c]])), name
                        assert np.array_equal(_bits(res.vals[only_a]), _bits(a[2][pa[only_a]])), name
                    finally:
                        res.close()
            finally:
                A.close()
        two = _build(mctx, (np.array([0, 1], np.int64), np.array([1], np.uint32), np.ones(1, dt)), (1, 3), dt)
        with pytest.raises(S.OspError) as ei:      # a repeated column fails in the library as not strictly ascending
            src.assign(two, [4], np.array([9, 2, 9]), space="host")
        assert ei.value.status == _lib.ERR_ARG and "ascending" in str(ei.value)
        two.close()
    finally:
        src.close()


# ---- the inverse of extract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_assign_and_extract_are_inverse_on_the_device(mctx, dt):
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    rng = np.random.default_rng(33)
    made = []
    try:
        for I, J in ((rng.permutation(M)[:150], np.sort(rng.choice(N, 2500, replace=False))), (np.array([80, 0, 70]), None), (None, np.arange(0, N, 3))):
            sub, _ = src.extract(I, J, space="host")
            made.append(sub)
            back, st = src.assign(sub, I, J, space="host")             # assign(extract(I, J), I, J) == c
            made.append(back)
            ge._same_arrays(back, src, "assign(extract)")
            assert st["nnz_both"] == st["nnz_region"] == sub.nnz
            variants, shape = _variants(csr, I, J, dt, 500)
            A = _build(mctx, variants["dense"], shape, dt)
            made.append(A)
            put, _ = src.assign(A, I, J, space="host")
            made.append(put)
            again, _ = put.extract(I, J, space="host")                 # extract(assign(a, I, J), I, J) == a
            made.append(again)
            ge._same_arrays(again, A, "extract(assign)")
    finally:
        for x in made:
            x.close()
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_an_embedding_into_an_empty_result(mctx, dt):
    csr = ge._built(dt)
    rng = np.random.default_rng(34)
    I, J = rng.permutation(M)[:40], np.sort(rng.choice(N, 900, replace=False))
    variants, shape = _variants(csr, I, J, dt, 600)
    a = variants["dense"]
    A = _build(mctx, a, shape, dt)
    empty, _ = mctx.build(M, N, [], [], dtype=dt, space="host")
    made = [A, empty]
    try:
        none = (np.zeros(M + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))
        for accum in (None, "times"):
            res, st = empty.assign(A, I, J, accum, space="host")
            made.append(res)
            _check(res, st, empty, model.assign(none, N, a, shape[1], I, J, accum), accum, "into an empty c")
            assert (st["nnz_region"], st["nnz_both"], st["nnz_out"], st["readbacks"]) == (0, 0, len(a[1]), 1) and st["launches"] > 0
        E, st = A.embed((M, N), I, J, space="host")
        made.append(E)
        ge._assert_same(E, model.embed(a, shape[1], (M, N), I, J))
        ge._same_arrays(E, made[2])
        back, _ = E.extract(I, J, space="host")                        # embed, then extract: a
        made.append(back)
        ge._same_arrays(back, A)
        P, st = A.embed((M, N), I, J[::-1].copy(), space="host")       # the composed path: a's columns land reversed
        made.append(P)
        assert st["composed"]
        ge._assert_same(P, model.embed(a, shape[1], (M, N), I, J[::-1]))
    finally:
        for x in made:
            x.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(c, a, rows, cols, space, accum=-1, reserved=None, n_rows=None, n_cols=None):
    """osp_csr_assign itself.  Lists: numpy uint32 arrays (space host) or device tensors.  Returns (status, whether *out
    and *stats are as they were)."""
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.AssignStats()
    st.nnz_c = 77
    spec = _lib.Assign()
    ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()   # noqa: E731
    if rows is not None:
        spec.rows, spec.n_rows = ptr(rows), len(rows) if n_rows is None else n_rows
    if cols is not None:
        spec.cols, spec.n_cols = ptr(cols), len(cols) if n_cols is None else n_cols
    spec.space, spec.accum = space, accum
    if reserved is not None:
        spec.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_assign(c._h, a._h, ctypes.byref(spec), ctypes.byref(o), ctypes.byref(st))
    if rc == 0:
        return rc, o
    return rc, o.value == sentinel and st.nnz_c == 77


# (rows, cols) for an a of 2 x 2
BAD_LISTS = {"a row index equal to M": ([3, M], [1, 2]), "a repeated row": ([3, 3], [1, 2]), "a repeated row, no columns": ([80, 80], None),
             "a column equal to N": ([3, 4], [1, N]), "a column equal to N, no rows": (None, [1, N]), "descending columns": ([1, 2], [5, 4]),
             "repeated columns": ([1, 2], [5, 5]), "repeated columns, no rows": (None, [7, 7]), "the largest index": ([0xffffffff, 1], [0xffffffff, 1])}


@pytest.mark.parametrize("space", ["host", "device"])
def test_bad_arguments_are_refused_with_out_untouched(mctx, space):
    """(tests/test_assign_cpu.py and the kernels' own text come first: assign_rowmap_kernel claims no word for an index >= M
    and extract_colmap_kernel sets no bit for a column >= N -- neither is ever an address.)"""
    dt = np.float64
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    a22 = (np.array([0, 1, 2], np.int64), np.array([0, 1], np.uint32), np.array([1.5, 2.5]))
    shapes = {(2, 2): _build(mctx, a22, (2, 2), dt), (M, 2): _build(mctx, (np.zeros(M + 1, np.int64), a22[1][:0], a22[2][:0]), (M, 2), dt),
              (2, N): _build(mctx, (np.array([0, 1, 2], np.int64), np.array([0, 1], np.uint32), a22[2]), (2, N), dt)}
    # (the M x 2 one is empty: without accum it still takes the general path, which reads the lists)
    f32 = _build(mctx, (a22[0], a22[1], a22[2].astype(np.float32)), (2, 2), np.float32)
    sp_ = _lib.OSP_HOST if space == "host" else _lib.OSP_DEVICE
    put = (lambda x: x) if space == "host" else am._dev
    try:
        for name, (I, J) in BAD_LISTS.items():
            A = shapes[(M if I is None else 2, N if J is None else 2)]
            I = None if I is None else put(np.array(I, np.uint32))
            J = None if J is None else put(np.array(J, np.uint32))
            torch.cuda.synchronize(DEV)
            for accum in (-1, 0):
                if accum == 0 and A.nnz == 0:
                    continue                                          # (with accum an empty a is a no-work shape)
                assert _raw(src, A, I, J, sp_, accum) == (_lib.ERR_ARG, True), (name, accum)
                assert _lib.lib().osp_last_error_string()
        good = put(np.array([1, 2], np.uint32))
        torch.cuda.synchronize(DEV)
        A = shapes[(2, 2)]
        assert _raw(src, A, good, good, 99) == (_lib.ERR_ARG, True)
        for accum in (-2, _lib.EWISE_OPS["minus"], _lib.EWISE_OPS["div"], 8):
            assert _raw(src, A, good, good, sp_, accum) == (_lib.ERR_ARG, True), accum
        for word in range(6):
            assert _raw(src, A, good, good, sp_, reserved=word) == (_lib.ERR_ARG, True)
        assert _raw(src, A, good, None, sp_, n_rows=0xffffffff) == (_lib.ERR_ARG, True)
        assert _raw(src, A, None, good, sp_, n_cols=1 << 33) == (_lib.ERR_ARG, True)
        assert _raw(src, f32, good, good, sp_) == (_lib.ERR_ARG, True)                 # dtypes differ
        other = S.Context(0)
        try:
            foreign = _build(other, a22, (2, 2), dt)
            assert _raw(src, foreign, good, good, sp_) == (_lib.ERR_ARG, True)         # contexts differ
            foreign.close()
        finally:
            other.close()
        # a's shape is not the region's
        three = put(np.array([1, 2, 3], np.uint32))
        torch.cuda.synchronize(DEV)
        for I, J in ((three, good), (good, three), (None, good), (good, None), (None, None)):
            assert _raw(src, A, I, J, sp_) == (_lib.ERR_DIM, True)
        rc, o = _raw(src, A, good, good, sp_)                            # and the library still works after every refusal
        assert rc == 0
        got = S.CsrResult(mctx, o)
        ge._assert_same(got, model.assign(csr, N, a22, 2, [1, 2], [1, 2])[0])
        got.close()
    finally:
        for x in list(shapes.values()) + [f32, src]:
            x.close()


def test_a_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    acsc, bcsr = gen.coo_to_csc(n, r, c, v), gen.coo_to_csr(n, c, r, v)
    ts = [am._dev(x) for x in acsc + bcsr]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    ok = _upload(mctx, n, bcsr)
    try:
        assert _raw(part, ok, None, None, _lib.OSP_HOST, 0) == (_lib.ERR_ARG, True)
        assert _raw(ok, part, None, None, _lib.OSP_HOST, 0) == (_lib.ERR_ARG, True)
        with pytest.raises(S.OspError) as ei:
            ok.assign(part, accum="plus")
        assert ei.value.status == _lib.ERR_ARG
    finally:
        part.close()
        ok.close()


# ---- the no-work shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_no_work_shapes_launch_nothing_and_read_no_list(mctx, dt):
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    none = (np.zeros(0, np.uint32), np.zeros(0, dt))

    def empty(m, n):
        return _build(mctx, (np.zeros(m + 1, np.int64),) + none, (m, n), dt)

    made = {k: empty(*k) for k in ((0, N), (M, 0), (0, 0), (2, 0), (0, 1), (2, 2), (M, N), (0, 70), (100, 70))}
    full = _build(mctx, csr, (M, N), dt)
    try:
        bad = [M, M]          # never read
        cases = [(src, (0, N), [], None, None, "c"), (src, (M, 0), None, [], None, "c"), (src, (0, 0), [], [], "plus", "c"),
                 (src, (2, 0), bad, [], None, "c"), (src, (0, 1), [], [N], None, "c"), (src, (2, 2), bad, [9, 3], "plus", "c"),
                 (src, (M, N), None, None, "max", "c"), (src, (M, N), None, None, None, "a"), (made[(M, N)], (M, N), None, None, None, "a"),
                 (made[(M, N)], (M, N), None, None, "plus", "a"), (made[(M, N)], (2, 2), bad, [9, 3], None, "c"),
                 (made[(0, 70)], (0, 70), None, None, None, "c"), (made[(0, 70)], (0, 0), [], [], "plus", "c"),
                 (made[(100, 70)], (2, 2), [100, 100], [70, 0], None, "c")]
        for c, akey, I, J, accum, same_as in cases:
            a = made[akey]
            res, st = c.assign(a, I, J, accum, space="host")
            try:
                what = (c.shape, akey, I, J, accum, st)
                ge._same_arrays(res, c if same_as == "c" else a, what)
                assert res.shape == c.shape and (st["launches"], st["readbacks"], st["nnz_region"], st["nnz_both"]) == (0, 0, 0, 0), what
                assert (st["nnz_c"], st["nnz_a"], st["nnz_out"]) == (c.nnz, a.nnz, res.nnz), what
            finally:
                res.close()
        res, st = src.assign(full, None, None, None)                    # both lists NULL without accum: a copy of a
        ge._same_arrays(res, full)
        assert st["launches"] == 0 and res.info["nnz_a"] == src.info["nnz_a"]
        res.close()
        # what is NOT a no-work shape reads its lists: an empty a without accum deletes the region
        with pytest.raises(S.OspError):
            src.assign(made[(2, 2)], bad, [3, 9], None, space="host")
        res, st = src.assign(made[(2, 2)], [80, 70], [3, 9], None, space="host")
        _check(res, st, src, model.assign(csr, N, (np.zeros(3, np.int64),) + none, 2, [80, 70], [3, 9]), None, "an empty a deletes")
        assert st["launches"] > 0 and st["nnz_region"] >= 1 and res.nnz == src.nnz - st["nnz_region"]
        res.close()
    finally:
        for x in list(made.values()) + [full, src]:
            x.close()


# ---- chaining ------------------------------------------------------------------------------------------------------------------------------
def test_assign_chains_with_the_other_operations(mctx):
    n, r, c, v = gen.rmat_coo(8, 8, "g500", seed=6)
    g = gen.coo_to_csr(n, r, c, v)
    src = _upload(mctx, n, g)
    rng = np.random.default_rng(35)
    I, J = rng.permutation(n)[:150], np.sort(rng.choice(n, 100, replace=False))
    made = []

    def host(res):
        return res.rowptr, res.colidx, res.vals

    try:
        # a transpose, a select and an mxm result, cut to the region's shape, assigned
        T, _ = src.transpose()
        sel, _ = src.select("offdiag")
        P, _ = src.mxm(src, "min", "plus")
        made += [T, sel, P]
        for name, X, accum in (("a transpose", T, None), ("a select", sel, "plus"), ("an mxm", P, "min")):
            sub, _ = X.extract(I, J, space="host")
            made.append(sub)
            res, st = src.assign(sub, I, J, accum, space="host")
            made.append(res)
            _check(res, st, src, model.assign(g, n, host(sub), len(J), I, J, accum), accum, name)
        # the whole of another result into this one, and an assigned result as an operand
        whole, st = src.assign(P, None, None, "plus")
        made.append(whole)
        want = model.assign(g, n, host(P), n, None, None, "plus")
        _check(whole, st, src, want, "plus", "an mxm, both lists None")
        res = made[4]                                                # the assign of the transpose's part
        w = host(res)
        x = rng.standard_normal(n)
        y, _ = res.mxv(x, "plus", "times", space="host")
        assert np.array_equal(_bits(y), _bits(mxv_model.mxv(*w, x, "plus", "times")[0]))
        prod, _ = res.mxm(src, "plus", "times")
        made.append(prod)
        ge._assert_same(prod, semiring_model.mxm(w, g, n, "plus", "times")[0], "as the left operand of mxm")
        ex, _ = res.extract(J, I, space="host")
        made.append(ex)
        ge._assert_same(ex, extract_model.extract_any(*w, n, J, I), "as the operand of extract")
        # a is c: both lists None under plus doubles every value; into a region of itself where the shapes allow it
        twice, st = src.assign(src, None, None, "plus")
        made.append(twice)
        assert np.array_equal(twice.rowptr, g[0]) and np.array_equal(twice.colidx, g[1]) and np.array_equal(_bits(twice.vals), _bits(g[2] + g[2]))
        assert st["nnz_both"] == st["nnz_region"] == src.nnz
        perm = rng.permutation(n)
        own, st = src.assign(src, perm, None, None, space="host")
        made.append(own)
        _check(own, st, src, model.assign(g, n, g, n, perm, None), None, "a is c, rows permuted")
    finally:
        for x_ in made:
            x_.close()
        src.close()


# ---- 2^32 - 1 columns -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_columns_at_the_top_of_the_range_and_across_bit_31(mctx, dt):
    """N = 2^32 - 1, the listed columns at the top of the range and on both sides of 2^31: cols[k] and a column's rank are
    32-bit quantities next to their limits."""
    WN = W.WIDTHS[-1]
    n0 = 4000
    table = W.phi("straddle", n0, WN)                                 # the lower half stays, the upper half ends at WN - 1
    narrow = am._csr_from_lengths([0, 5, 2049, 64, 0, 3000, 1, 700], n0, dt, seed=36, lo=0)
    cw = W.relabel_csr(narrow, table)
    src = _upload(mctx, WN, cw)
    rng = np.random.default_rng(37)
    picked = np.sort(rng.choice(n0, 1500, replace=False))
    J = np.unique(np.concatenate([table[picked].astype(np.int64), [1 << 31, (1 << 31) - 1, WN - 1, WN - 2, 5000, 0]]))
    assert J.min() == 0 and J.max() == WN - 1 and (J < 1 << 31).any() and (J > 1 << 31).any()
    I = np.array([5, 2, 7, 0])
    has = rng.random((len(I), len(J))) < 0.3
    has[0] = True
    a = _csr_of_dense(has, dt, 38)
    A = _build(mctx, a, has.shape, dt)
    made = [A]
    try:
        for accum in (None, "plus", "second"):
            res, st = src.assign(A, I, J, accum, space="host")
            made.append(res)
            want = model.assign(cw, WN, a, len(J), I, J, accum)
            _check(res, st, src, want, accum, ("wide", accum))
            assert 0 < st["nnz_both"] < st["nnz_region"] and res.colidx.max() == WN - 1
        back, _ = made[1].extract(I, J, space="host")
        made.append(back)
        ge._same_arrays(back, A, "extract(assign) at the full width")
    finally:
        for x in made:
            x.close()
        src.close()


# ---- the pool ------------------------------------------------------------------------------------------------------------------------------
def test_fifty_back_to_back_calls_give_the_same_arrays_and_the_pool_does_not_grow(mctx, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call (the row map, the column bitmap, the error word and the
    counter are zeroed by every call), and after the first call no call allocates device memory: the library's own
    count of pool misses, printed under OSP_VERBOSE, as tests/test_gpu_extract.py reads it."""
    dt = np.float64
    csr = ge._built(dt)
    src = ge._source(mctx, dt)
    rng = np.random.default_rng(39)
    I, J = rng.permutation(M)[:120], np.sort(rng.choice(N, 2000, replace=False))
    variants, shape = _variants(csr, I, J, dt, 700)
    a = variants["dense"]
    A = _build(mctx, a, shape, dt)
    wants = {acc: model.assign(csr, N, a, shape[1], I, J, acc) for acc in (None, "plus")}
    monkeypatch.setenv("OSP_VERBOSE", "1")
    first, misses = {}, []
    try:
        for i in range(50):
            accum = None if i % 2 == 0 else "plus"
            capfd.readouterr()
            res, st = src.assign(A, I, J, accum, space="host")
            err = capfd.readouterr().err
            got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy())
            if accum not in first:
                _check(res, st, src, wants[accum], accum)
                first[accum] = got
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, first[accum])), i
            res.close()
            found = re.findall(r"\[osp\] assign .*pool misses so far: (\d+) hipMalloc calls", err)
            assert len(found) == 1, err
            misses.append(int(found[0]))
    finally:
        A.close()
        src.close()
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses
