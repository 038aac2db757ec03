"""osp_csr_extract on the GPU against tests/extract_model.py -- row pointers and columns exact, values equal as BITS (they are
moved, never computed) -- for every pair of a row list and a column list on one built matrix, the identities that tie it to
transpose and select_vertices, host and device lists, the composed path for general column lists against scipy, its refusals
(host and device lists, `out` untouched), empty shapes, chaining with the other result operations, and the pool."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from tests import extract_model as model
from tests import mxv_model
from tests import semiring_model
from tests import test_extract_cpu as cpu          # _scipy_extract only
from tests import test_gpu_apply_mask as am        # _upload, _bits, _special, _dev, CHUNK only
from tests import transpose_model

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
_upload = am._upload
DTYPES = [np.float32, np.float64]
M, N = 300, 5000
# where the rows of the lengths that matter sit; row 0 is empty, every other row is short (0 to 8 entries)
LONG = {10: 1, 20: 63, 30: 64, 40: 65, 50: 2047, 60: 2048, 70: 2049, 80: 5000}
QUIET = np.arange(100, 110)     # columns that only the full row (80) holds


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _built(dt):
    rng = np.random.default_rng(18)
    lengths = rng.integers(0, 9, M)
    lengths[0] = lengths[M - 1] = 0
    for r, k in LONG.items():
        lengths[r] = k
    free = np.setdiff1d(np.arange(N), QUIET)
    cols = [np.sort(rng.choice(N if k == N else free, size=int(k), replace=False)) for k in lengths]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    at = np.arange(0, len(val), 7)                      # the special values at every seventh entry, the full row included
    val[at] = np.resize(am._special(dt), len(at))
    assert am.CHUNK == 2048 and (np.diff(rowptr)[list(LONG)] == list(LONG.values())).all()
    return rowptr, col, val


def _source(mctx, dt):
    """The built matrix as a library result, its special values' bits intact in the full row too: _upload's merge sums a
    full row into a dense accumulator, which does not keep a signalling NaN's bits, so the TRANSPOSE is uploaded -- its
    rows are short -- and turned on the device, which moves bits (tests/test_gpu_transpose.py)."""
    csr = _built(dt)
    up = _upload(mctx, M, transpose_model.transpose(*csr, N))
    try:
        src, _ = up.transpose()
    finally:
        up.close()
    assert src.shape == (M, N) and np.array_equal(src.rowptr, csr[0]) and np.array_equal(src.colidx, csr[1])
    assert np.array_equal(_bits(src.vals), _bits(csr[2]))
    return src


def _row_lists():
    return {"none": None, "identity": np.arange(M), "reversed": np.arange(M)[::-1], "twice": np.repeat(np.arange(M), 2),
            "empty row first and last": np.array([0, 5, 70, 20, 80, 0]), "2049 three times": np.array([70, 70, 70]),
            "one": np.array([60]), "empty": np.zeros(0, np.int64)}


def _col_lists():
    return {"none": None, "all": np.arange(N), "first": np.array([0]), "last": np.array([N - 1]), "63 64": np.array([63, 64]),
            "every 64th": np.arange(0, N, 64), "quiet": QUIET, "empty": np.zeros(0, np.int64)}


def _assert_same(res, want, what=""):
    rowptr, col, val = want
    assert res.nnz == len(col) == res.info["nnz_c"], what
    assert np.array_equal(res.rowptr, rowptr), what
    assert np.array_equal(res.colidx, col), what
    assert res.vals.dtype == val.dtype and np.array_equal(_bits(res.vals), _bits(val)), what


def _same_arrays(a, b, what=""):
    assert a.shape == b.shape and a.nnz == b.nnz, what
    assert np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.colidx, b.colidx), what
    assert np.array_equal(_bits(a.vals), _bits(b.vals)), what


def _idx(a):
    """An index list as a device tensor (int32 holds a uint32 list's bits)."""
    return am._dev(np.asarray(a, np.uint32))


# ---- every pair of lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_every_pair_of_lists_equals_the_model(mctx, dt):
    csr = _built(dt)
    src = _source(mctx, dt)
    try:
        for rn, I in _row_lists().items():
            for cn, J in _col_lists().items():
                want, wst = model.extract(*csr, N, I, J)
                res, st = src.extract(I, J, space="host")
                try:
                    what = (rn, cn, st)
                    assert res.shape == (M if I is None else len(I), N if J is None else len(J)) and res.dtype == dt, what
                    _assert_same(res, want, what)
                    assert {k: st[k] for k in wst} == wst, (what, wst)
                    assert st["ms_total"] >= 0 and not st["composed"]
                    info = res.info
                    changed = {"M": res.shape[0], "N": res.shape[1], "row_begin": 0, "row_end": res.shape[0], "nnz_c": res.nnz}
                    assert all(info[k] == v for k, v in changed.items()), what
                    assert all(info[k] == src.info[k] for k in info if k not in changed and k != "ms_total"), what
                finally:
                    res.close()
        # the quiet columns hit nothing but the full row
        assert model.extract(*csr, N, [70, 70, 70], QUIET)[1] == {"nnz_in": len(csr[1]), "nnz_gathered": 3 * 2049, "nnz_out": 0, "readbacks": 2}
        assert np.array_equal(src.rowptr, csr[0]) and np.array_equal(_bits(src.vals), _bits(csr[2]))     # `in` stays valid
    finally:
        src.close()


# ---- identities on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_identities_on_the_device(mctx, dt):
    csr = _built(dt)
    rng = np.random.default_rng(21)
    keep_r, keep_c = rng.random(M) < 0.5, rng.random(N) < 0.5
    keep_r[[0, 70, 80]] = True
    I, J = np.flatnonzero(keep_r), np.flatnonzero(keep_c)
    src = _source(mctx, dt)
    made = []
    try:
        both, _ = src.extract(I, J, space="host")
        made.append(both)
        _assert_same(both, model.extract(*csr, N, I, J)[0])
        # rows, then columns
        r_only, _ = src.extract(I, None, space="host")
        made.append(r_only)
        then_c, st = r_only.extract(None, J, space="host")
        made.append(then_c)
        _same_arrays(then_c, both, "extract(I, None) then extract(None, J)")
        assert st["nnz_gathered"] == r_only.nnz
        # the transpose of the extract is the extract of the transpose, lists swapped
        bt, _ = both.transpose()
        made.append(bt)
        T, _ = src.transpose()
        made.append(T)
        tb, _ = T.extract(J, I, space="host")
        made.append(tb)
        _same_arrays(bt, tb, "extract(I, J).transpose() and transpose().extract(J, I)")
        # select_vertices with the same keep vectors: the same entries, not renumbered, the removed rows still there
        sel, _ = src.select_vertices(keep_r.astype(np.uint8), keep_c.astype(np.uint8), space="host")
        made.append(sel)
        rank = np.cumsum(keep_c) - 1
        assert np.array_equal(both.rowptr, np.concatenate([[0], np.cumsum(np.diff(sel.rowptr)[I])]))
        assert np.array_equal(both.colidx, rank[sel.colidx]) and np.array_equal(_bits(both.vals), _bits(sel.vals))
        assert (np.diff(sel.rowptr)[~keep_r] == 0).all()
    finally:
        for x in made:
            x.close()
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_host_and_device_lists_give_equal_arrays(mctx, dt):
    csr = _built(dt)
    src = _source(mctx, dt)
    rng = np.random.default_rng(22)
    I = rng.integers(0, M, 500)
    J = np.sort(rng.choice(N, 1200, replace=False))
    ti, tj = _idx(I), _idx(J)
    torch.cuda.synchronize(DEV)
    try:
        for rows_h, cols_h, rows_d, cols_d in ((I, J, ti, tj), (I, None, ti, None), (None, J, None, tj)):
            a, sa = src.extract(rows_h, cols_h, space="host")
            b, sb = src.extract(rows_d, cols_d)                      # space="device" is the default
            c, sc = src.extract(None if rows_d is None else (rows_d.data_ptr(), rows_d.numel()),
                                None if cols_d is None else (cols_d.data_ptr(), cols_d.numel()))   # bare addresses
            try:
                _assert_same(a, model.extract(*csr, N, rows_h, cols_h)[0])
                _same_arrays(a, b)
                _same_arrays(a, c)
                keys = ("nnz_in", "nnz_gathered", "nnz_out", "launches", "readbacks")
                assert [sa[k] for k in keys] == [sb[k] for k in keys] == [sc[k] for k in keys]
            finally:
                a.close()
                b.close()
                c.close()
    finally:
        src.close()


# ---- general column lists: the composed path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("space", ["host", "device"])
def test_the_composed_path_matches_scipy(mctx, dt, space):
    csr = _built(dt)
    src = _source(mctx, dt)
    rng = np.random.default_rng(23)
    cases = {"permutation": (None, rng.permutation(N)), "reversed both": (np.arange(M)[::-1], np.arange(N)[::-1]),
             "duplicates": (rng.integers(0, M, 40), np.concatenate([[7, 7, 7], rng.integers(0, N, 900), [7]]))}
    try:
        for name, (I, J) in cases.items():
            if space == "device":
                rows, cols = None if I is None else _idx(I), _idx(J)
                torch.cuda.synchronize(DEV)
            else:
                rows, cols = I, J
            res, st = src.extract(rows, cols, space=space)
            try:
                assert st["composed"] and st["ms_total"] > 0 and st["nnz_in"] == src.nnz and st["nnz_out"] == res.nnz, name
                wp, wc, wpos = cpu._scipy_extract(csr, N, I, J)
                _assert_same(res, (wp, wc, csr[2][wpos]), name)
                _assert_same(res, model.extract_any(*csr, N, I, J), name)
            finally:
                res.close()
        for bad in ([N], [3, 2, N]):                                  # an index beyond its dimension, on the composed path too
            with pytest.raises(S.OspError) as ei:
                src.extract(None, np.array([5, 4] + bad), space="host")
            assert ei.value.status == _lib.ERR_ARG
    finally:
        src.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_permute_and_its_inverse_give_the_input_back(mctx, dt):
    n, r, c, v = gen.rmat_coo(10, 8, "g500", seed=5, dtype=dt)
    g = gen.coo_to_csr(n, r, c, v)
    src = _upload(mctx, n, g)
    p = np.random.default_rng(24).permutation(n)
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    made = []
    try:
        P, st = src.permute(p, space="host")
        made.append(P)
        assert st["composed"] and P.shape == (n, n) and P.nnz == src.nnz
        _assert_same(P, model.extract_any(*g, n, p, p))
        back, _ = P.permute(_idx(inv))
        made.append(back)
        _assert_same(back, g)
        same, st = src.permute(np.arange(n), space="host")             # the identity is ascending: the direct path
        made.append(same)
        assert not st["composed"]
        _assert_same(same, g)
    finally:
        for x in made:
            x.close()
        src.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(res, rows, cols, space, reserved=None, n_rows=None, n_cols=None):
    """osp_csr_extract itself (CsrResult.extract would compose a descending list).  Lists: numpy uint32 arrays
    (space host) or device tensors.  Returns (status, whether *out and *stats are as they were)."""
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.ExtractStats()
    st.nnz_in = 77
    ex = _lib.Extract()
    ptr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()   # noqa: E731
    if rows is not None:
        ex.rows, ex.n_rows = ptr(rows), len(rows) if n_rows is None else n_rows
    if cols is not None:
        ex.cols, ex.n_cols = ptr(cols), len(cols) if n_cols is None else n_cols
    ex.space = space
    if reserved is not None:
        ex.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_extract(res._h, ctypes.byref(ex), ctypes.byref(o), ctypes.byref(st))
    if rc == 0:
        return rc, o
    return rc, o.value == sentinel and st.nnz_in == 77


BAD_LISTS = {"a row index equal to M": ([3, M, 5], None), "a row index equal to M, with columns": ([3, M, 5], [1, 2]),
             "a column equal to N": (None, [1, N]), "a column equal to N, with rows": ([3, 4], [1, N]),
             "descending columns": (None, [5, 4]), "descending columns, with rows": ([1], [2, 900, 899]),
             "repeated columns": (None, [5, 5]), "repeated columns, with rows": ([80, 80], [0, 7, 7]),
             "the largest index": ([0xffffffff], [0xffffffff])}


@pytest.mark.parametrize("space", ["host", "device"])
def test_bad_lists_are_refused_with_out_untouched(mctx, space):
    """(tests/test_extract_cpu.py and the kernels' own text come first: extract_len_kernel gives an index >= M the length 0
    and extract_colmap_kernel sets no bit for a column >= N -- neither is ever an address.)"""
    csr = _built(np.float64)
    src = _source(mctx, np.float64)
    try:
        for name, (I, J) in BAD_LISTS.items():
            I = None if I is None else np.array(I, np.uint32)
            J = None if J is None else np.array(J, np.uint32)
            if space == "device":
                I, J = None if I is None else am._dev(I), None if J is None else am._dev(J)
                torch.cuda.synchronize(DEV)
            assert _raw(src, I, J, _lib.OSP_HOST if space == "host" else _lib.OSP_DEVICE) == (_lib.ERR_ARG, True), name
            assert _lib.lib().osp_last_error_string()
        good = np.array([1, 2], np.uint32)
        good = good if space == "host" else am._dev(good)
        sp_ = _lib.OSP_HOST if space == "host" else _lib.OSP_DEVICE
        assert _raw(src, good, good, 99) == (_lib.ERR_ARG, True)
        for word in range(7):
            assert _raw(src, good, good, sp_, reserved=word) == (_lib.ERR_ARG, True)
        assert _raw(src, good, None, sp_, n_rows=0xffffffff) == (_lib.ERR_ARG, True)
        assert _raw(src, None, good, sp_, n_cols=1 << 32) == (_lib.ERR_ARG, True)
        rc, o = _raw(src, good, good, sp_)                            # and the library still works after every refusal
        assert rc == 0
        got = S.CsrResult(mctx, o)
        _assert_same(got, model.extract(*csr, N, [1, 2], [1, 2])[0])
        got.close()
    finally:
        src.close()


def test_a_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    acsc, bcsr = gen.coo_to_csc(n, r, c, v), gen.coo_to_csr(n, c, r, v)
    ts = [am._dev(x) for x in acsc + bcsr]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    try:
        rows = np.array([0, 1], np.uint32)
        assert _raw(part, rows, None, _lib.OSP_HOST) == (_lib.ERR_ARG, True)
        with pytest.raises(S.OspError) as ei:
            part.extract([0, 1], space="host")
        assert ei.value.status == _lib.ERR_ARG
    finally:
        part.close()


# ---- empty shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_empty_shapes_launch_nothing(mctx, dt):
    csr = _built(dt)
    src = _source(mctx, dt)
    none = (np.zeros(0, np.uint32), np.zeros(0, dt))
    empty = _upload(mctx, 70, (np.zeros(101, np.int64),) + none)
    nothing = _upload(mctx, 0, (np.zeros(1, np.int64),) + none)
    try:
        cases = [(src, [], None, (0, N)), (src, None, [], (M, 0)), (src, [], [], (0, 0)), (src, [3, 3], [], (2, 0)), (src, [], [7], (0, 1)),
                 (empty, None, None, (100, 70)), (empty, [5, 5, 99], None, (3, 70)), (empty, None, [0, 69], (100, 2)),
                 (empty, [1], [2], (1, 1)), (nothing, None, None, (0, 0)), (nothing, [], [], (0, 0))]
        for a, I, J, shape in cases:
            res, st = a.extract(I, J, space="host")
            try:
                assert res.shape == shape and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(shape[0] + 1, np.int64)), (I, J)
                assert (st["launches"], st["readbacks"], st["nnz_out"]) == (0, 0, 0), (I, J, st)
                assert st["nnz_in"] == a.nnz and st["nnz_gathered"] == (a.nnz if I is None else 0)
                again, st2 = res.extract(None, None)                 # an empty result is an operand like any other
                assert again.shape == shape and st2["launches"] == 0
                again.close()
            finally:
                res.close()
        # rows that hold nothing: known only after the lengths came back, nothing is launched after that
        for J, launches in ((None, 3), ([1, 2], 5)):
            res, st = src.extract([0, M - 1, 0], J, space="host")
            assert res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(4, np.int64)) and res.shape == (3, N if J is None else 2)
            assert (st["nnz_gathered"], st["nnz_out"], st["readbacks"], st["launches"]) == (0, 0, 1, launches), st
            res.close()
    finally:
        for x in (src, empty, nothing):
            x.close()


# ---- chaining, pool --------------------------------------------------------------------------------------------------------------------
def test_extract_chains_with_the_other_operations(mctx):
    n, r, c, v = gen.rmat_coo(8, 8, "g500", seed=6)
    g = gen.coo_to_csr(n, r, c, v)
    src = _upload(mctx, n, g)
    rng = np.random.default_rng(25)
    I, J = rng.integers(0, n, 150), np.sort(rng.choice(n, 100, replace=False))
    made = []
    try:
        T, _ = src.transpose()
        made.append(T)
        et, _ = T.extract(I, J, space="host")
        made.append(et)
        _assert_same(et, model.extract(*transpose_model.transpose(*g, n), n, I, J)[0], "of a transpose")
        sel, _ = src.select("offdiag")
        made.append(sel)
        es, _ = sel.extract(I, J, space="host")
        made.append(es)
        _assert_same(es, model.extract(sel.rowptr, sel.colidx, sel.vals, n, I, J)[0], "of a select")
        P, _ = src.mxm(src, "min", "plus")
        made.append(P)
        ep, _ = P.extract(I, J, space="host")
        made.append(ep)
        wp = semiring_model.mxm(g, g, n, "min", "plus")[0]
        _assert_same(ep, model.extract(*wp, n, I, J)[0], "of an mxm")
        # an extract as an operand: 150 x n times x, and (150 x n) times (n x 100)
        rows_only, _ = src.extract(I, None, space="host")
        made.append(rows_only)
        cols_only, _ = src.extract(None, J, space="host")
        made.append(cols_only)
        a, b = model.extract(*g, n, I, None)[0], model.extract(*g, n, None, J)[0]
        x = rng.standard_normal(n)
        y, _ = rows_only.mxv(x, "plus", "times", space="host")
        assert np.array_equal(_bits(y), _bits(mxv_model.mxv(*a, x, "plus", "times")[0]))
        prod, _ = rows_only.mxm(cols_only, "plus", "times")
        made.append(prod)
        wprod = semiring_model.mxm(a, b, len(J), "plus", "times")[0]
        assert prod.shape == (150, 100)
        _assert_same(prod, wprod, "as the operands of mxm")
    finally:
        for x_ in made:
            x_.close()
        src.close()


@pytest.mark.parametrize("which", ["both lists", "rows only", "columns only"])
def test_fifty_back_to_back_calls_give_the_same_arrays_and_the_pool_does_not_grow(mctx, which, monkeypatch, capfd):
    """Recycled pool buffers carry nothing over from call to call (the column bitmap and the error word are zeroed by every
    call), and after the first call no call allocates device memory: the library's own count of pool misses, printed under
    OSP_VERBOSE, as tests/test_gpu_transpose.py reads it."""
    csr = _built(np.float64)
    src = _source(mctx, np.float64)
    rng = np.random.default_rng(26)
    I = rng.integers(0, M, 400) if which != "columns only" else None
    J = np.sort(rng.choice(N, 2000, replace=False)) if which != "rows only" else None
    want = model.extract(*csr, N, I, J)[0]
    monkeypatch.setenv("OSP_VERBOSE", "1")
    first, misses = None, []
    try:
        for i in range(50):
            capfd.readouterr()
            res, st = src.extract(I, J, space="host")
            err = capfd.readouterr().err
            got = (res.rowptr.copy(), res.colidx.copy(), _bits(res.vals).copy())
            res.close()
            found = re.findall(r"\[osp\] extract .*pool misses so far: (\d+) hipMalloc calls", err)
            assert len(found) == 1, err
            misses.append(int(found[0]))
            if first is None:
                first = got
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], _bits(want[2]))
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, first)), i
    finally:
        src.close()
    print("pool misses after every call:", misses)
    assert misses[1:] == [misses[0]] * 49, misses
