"""osp_csr_kron on the GPU against the numpy model of tests/kron_model.py, by the rule of tests/test_gpu_ewise.py: row
pointers and columns exact, value BITS equal for FIRST, SECOND, MIN and MAX (copies); for TIMES and PLUS the bits are equal
where the model's result is no NaN, and the result is a NaN where it is.  Operands go up through ``Context.build(dup="error")``
and every seventh entry carries a special value.  The sweep over the operand family, the chunk edges of the entries kernel,
one row of 9 * 10^6 entries, millions of empty rows, shapes at the limits of the column and row spaces, the refusals, the
identities that tie the product to the other operations, and the sweep's slice in children on a poisoned and on a guarded
pool."""
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
from tests import kron_cases as kc
from tests import kron_model as model
from tests import test_gpu_apply_mask as am   # _dev and _bits only

pytestmark = pytest.mark.gpu

ROOT = kc.ROOT
CHUNK = kc.CHUNK
DEV = am.DEV
_bits = am._bits
CHILD_TIMEOUT_S = 120   # a hang guard: a child starts Python, loads the library, creates a context and makes 96 small products


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _assert_values(got, want, op):
    gb, wb = _bits(got), _bits(want)
    if op in model.COPY_OPS:
        assert np.array_equal(gb, wb)
        return
    nan = np.isnan(want)
    assert np.array_equal(gb[~nan], wb[~nan])
    assert np.isnan(got[nan]).all()


def _check(res, st, a, na, b, nb, op):
    (rowptr, col, val), (M, N), want = model.kron(a, na, b, nb, op)
    assert res.shape == (M, N) and res.dtype == a[2].dtype.type
    assert res.nnz == len(col) == len(a[1]) * len(b[1])
    assert np.array_equal(res.rowptr, rowptr)
    assert np.array_equal(res.colidx, col)
    _assert_values(res.vals, val, op)
    assert {k: st[k] for k in ("nnz_a", "nnz_b", "nnz_out", "launches", "readbacks")} == {k: want[k] for k in
                                                                                         ("nnz_a", "nnz_b", "nnz_out", "launches", "readbacks")}
    assert st["ms_total"] >= 0
    info = dict(res.info)
    named = {"M": M, "K": 0, "N": N, "row_begin": 0, "row_end": M, "nnz_a": len(a[1]), "nnz_b": len(b[1]), "nnz_c": len(col),
             "partials": len(col), "dtype": _lib.OSP_F32 if a[2].dtype == np.float32 else _lib.OSP_F64}
    for k, v in named.items():
        assert info.pop(k) == v, k
    assert info.pop("ms_total") == st["ms_total"]
    assert not any(info.values()), info   # every other field is 0
    return res


def _kron(mctx, a, na, b, nb, op):
    """Uploads both operands, checks the product against the model; returns nothing and closes everything."""
    A, B = kc.build(mctx, a, na), kc.build(mctx, b, nb)
    try:
        res, st = A.kron(B, op)
        try:
            _check(res, st, a, na, b, nb, op)
        finally:
            res.close()
    finally:
        A.close()
        B.close()


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
def test_the_special_values_are_the_mask_filters():
    for dt in (np.float32, np.float64):
        assert np.array_equal(_bits(kc.special(dt)), _bits(am._special(dt)))
        fam = kc.family(dt)
        assert [len(c[0]) - 1 for c, _ in fam.values()] == [1, 1, 70, 9, 5, 4] and [n for _, n in fam.values()] == [1, 70, 1, 11, 7, 6]
        assert np.diff(fam["ragged"][0][0]).tolist() == kc.RAGGED and len(fam["empty"][0][1]) == 0


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("op", model.OPS)
def test_kron_equals_the_model_over_the_family(mctx, op, dt):
    fam = kc.family(dt)
    made = {name: kc.build(mctx, csr, ncol) for name, (csr, ncol) in fam.items()}
    try:
        for name, (csr, ncol) in fam.items():   # the upload keeps every bit
            got = made[name]
            assert np.array_equal(got.rowptr, csr[0]) and np.array_equal(got.colidx, csr[1]) and np.array_equal(_bits(got.vals), _bits(csr[2]))
        for an, (a, na) in fam.items():
            for bn, (b, nb) in fam.items():       # (an == bn: the same handle twice)
                res, st = made[an].kron(made[bn], op)
                try:
                    _check(res, st, a, na, b, nb, op)
                finally:
                    res.close()
        for x in made.values():                    # both operands stay valid
            assert x.to_host() is not None and x.info["nnz_c"] == x.nnz
    finally:
        for x in made.values():
            x.close()


# ---- chunk edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("nnz_out", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_chunk_edges(mctx, nnz_out, dt):
    """(one entry) (x) (rows of length 1, every third row empty): every step of a lane leaves its row of out; and with the
    sides swapped every step changes a's row."""
    assert CHUNK == 1024
    lists, k = [], 0
    while k < nnz_out:
        if len(lists) % 3 == 2:
            lists.append([])
        else:
            lists.append([(5 * k) % 97])
            k += 1
    rows, one = kc.csr_of(lists, dt, 11), kc.csr_of([[2]], dt, 12)
    for op in ("times", "first", "second"):
        _kron(mctx, one, 3, rows, 97, op)
        _kron(mctx, rows, 97, one, 3, op)


# ---- one row of 9 * 10^6 entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["times", "first"])
def test_hub_times_hub_is_one_long_row(mctx, op):
    a, b = kc.csr_of([np.arange(3000)], np.float64, 13), kc.csr_of([np.arange(3000)], np.float64, 14)
    _kron(mctx, a, 3000, b, 3000, op)


# ---- rows sparse in entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sparse (x) ragged", "ragged (x) sparse"])
def test_millions_of_empty_rows(mctx, order):
    m = 1 << 20
    lengths = np.zeros(m, np.int64)
    lengths[[0, 1 << 19, m - 1]] = [2, 3, 1]
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    col = np.array([0, 2, 0, 1, 2, 1], np.uint32)
    sparse = (rowptr, col, kc.csr_of([col], np.float64, 15)[2])
    ragged, nr = kc.family(np.float64)["ragged"]
    (a, na), (b, nb) = ((sparse, 3), (ragged, nr)) if order.startswith("sparse") else ((ragged, nr), (sparse, 3))
    A, B = kc.build(mctx, a, na), kc.build(mctx, b, nb)
    try:
        res, st = A.kron(B, "times")
        try:
            assert res.shape[0] == 9 << 20
            assert np.array_equal(res.rowptr, model.closed_form_rowptr(a[0], b[0]))   # in full
            _check(res, st, a, na, b, nb, "times")
        finally:
            res.close()
    finally:
        A.close()
        B.close()


# ---- wide and tall --------------------------------------------------------------------------------------------------------------------------
def test_the_last_column_of_the_widest_result(mctx):
    a = kc.csr_of([[0, 65534], [65534]], np.float64, 16)
    b = kc.csr_of([[0, 65536], [], [65536]], np.float64, 17)
    (_, col, _), (_, N), _ = model.kron(a, 65535, b, 65537)
    assert N == (1 << 32) - 1 and int(col.max()) == (1 << 32) - 2
    for op in ("times", "second"):
        _kron(mctx, a, 65535, b, 65537, op)


def test_columns_on_both_sides_of_bit_31_in_one_row(mctx):
    a = kc.csr_of([[0, 23170, 46340], [], [46339]], np.float32, 18)
    b = kc.csr_of([[0, 1, 46340], [46340]], np.float32, 19)
    (rowptr, col, _), (_, N), _ = model.kron(a, 46341, b, 46341)
    assert N == 2147488281
    first = col[rowptr[0]:rowptr[1]].astype(np.int64)
    assert (first < (1 << 31)).any() and (first >= (1 << 31)).any()
    for op in ("times", "first"):
        _kron(mctx, a, 46341, b, 46341, op)


def test_two_to_the_24_rows(mctx):
    lists = [[] for _ in range(4096)]
    for r, cols in ((0, [0, 1]), (1, [1]), (2047, [0]), (4095, [0, 1])):
        lists[r] = cols
    a, b = kc.csr_of(lists, np.float64, 20), kc.csr_of(lists[::-1], np.float64, 21)
    A, B = kc.build(mctx, a, 2), kc.build(mctx, b, 2)
    try:
        res, st = A.kron(B, "plus")
        try:
            assert res.shape == (1 << 24, 4)
            _check(res, st, a, 2, b, 2, "plus")
        finally:
            res.close()
    finally:
        A.close()
        B.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _raw(a, b, op=_lib.EWISE_OPS["times"], reserved=None):
    """osp_csr_kron itself.  Returns (status, whether *out and *stats are as they were), or (0, the handle)."""
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.KronStats()
    st.nnz_a = 77
    spec = _lib.Kron()
    spec.op = op
    if reserved is not None:
        spec.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_kron(a._h, b._h, ctypes.byref(spec), ctypes.byref(o), ctypes.byref(st))
    if rc == 0:
        return rc, o
    assert _lib.lib().osp_last_error_string()
    return rc, o.value == sentinel and st.nnz_a == 77


def _full(m, n, dt=np.float64):
    return (np.arange(m + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.uint32), m), np.ones(m * n, dt))


def test_refusals_leave_out_and_stats_untouched(mctx):
    one = (np.array([0, 1], np.int64), np.zeros(1, np.uint32), np.ones(1))
    made = {}

    def put(name, csr, ncol):
        made[name] = kc.build(mctx, csr, ncol)
        return made[name]
    try:
        wide = put("wide", one, 65536)
        assert _raw(wide, wide) == (_lib.ERR_ARG, True)                                   # N = 2^32
        t1 = put("t1", (np.concatenate([[0], np.ones(65535, np.int64)]), one[1], one[2]), 1)
        t2 = put("t2", (np.concatenate([[0], np.ones(65537, np.int64)]), one[1], one[2]), 1)
        assert _raw(t1, t2) == (_lib.ERR_ARG, True) and _raw(t2, t1) == (_lib.ERR_ARG, True)   # M = 2^32 - 1
        sq = put("sq", _full(256, 256), 256)
        assert sq.nnz == 65536 and _raw(sq, sq) == (_lib.ERR_CAPACITY, True)                # 2^32 entries
        n1, n2 = put("n1", _full(255, 257), 257), put("n2", _full(1, 65537), 65537)
        assert n1.nnz * n2.nnz == (1 << 32) - 1
        assert _raw(n1, n2) == (_lib.ERR_CAPACITY, True) and _raw(n2, n1) == (_lib.ERR_CAPACITY, True)   # exactly 2^32 - 1
        # the argument checks come before the size checks
        assert _raw(sq, sq, _lib.EWISE_OPS["minus"]) == (_lib.ERR_ARG, True)
        small = put("small", one, 3)
        for op in (-1, _lib.EWISE_OPS["minus"], _lib.EWISE_OPS["div"], 8, 1 << 20):
            assert _raw(small, small, op) == (_lib.ERR_ARG, True), op
        for word in range(7):
            assert _raw(small, small, reserved=word) == (_lib.ERR_ARG, True), word
        f32 = put("f32", (one[0], one[1], np.ones(1, np.float32)), 3)
        assert _raw(small, f32) == (_lib.ERR_ARG, True) and _raw(f32, small) == (_lib.ERR_ARG, True)
        with pytest.raises(S.OspError) as ei:
            small.kron(f32)
        assert ei.value.status == _lib.ERR_ARG
        with pytest.raises(S.OspError) as ei:
            sq.kron(sq)
        assert ei.value.status == _lib.ERR_CAPACITY
        other = S.Context(0)
        try:
            foreign = kc.build(other, one, 3)
            assert _raw(small, foreign) == (_lib.ERR_ARG, True)
            foreign.close()
        finally:
            other.close()
        rc, o = _raw(small, small)                                                       # and the library still works
        assert rc == 0
        got = S.CsrResult(mctx, o)
        assert got.shape == (1, 9) and got.colidx.tolist() == [0] and got.vals.tolist() == [1.0]
        got.close()
    finally:
        for x in made.values():
            x.close()


def test_a_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(8, 4, "g500", seed=3)
    acsc, bcsr = gen.coo_to_csc(n, r, c, v), gen.coo_to_csr(n, c, r, v)
    ts = [am._dev(x) for x in acsc + bcsr]
    torch.cuda.synchronize(DEV)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in ts])
    ok = kc.build(mctx, (np.array([0, 1], np.int64), np.zeros(1, np.uint32), np.ones(1)), 1)
    try:
        assert _raw(part, ok) == (_lib.ERR_ARG, True) and _raw(ok, part) == (_lib.ERR_ARG, True)
        with pytest.raises(S.OspError) as ei:
            ok.kron(part)
        assert ei.value.status == _lib.ERR_ARG
    finally:
        part.close()
        ok.close()


# ---- identities on the device ------------------------------------------------------------------------------------------------------------
def _same(x, y):
    assert x.shape == y.shape and x.nnz == y.nnz
    assert np.array_equal(x.rowptr, y.rowptr) and np.array_equal(x.colidx, y.colidx) and np.array_equal(_bits(x.vals), _bits(y.vals))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_identities_on_the_device(mctx, dt):
    fam = kc.family(dt)
    made = {name: kc.build(mctx, csr, ncol) for name, (csr, ncol) in fam.items()}
    nn = {name: kc.build(mctx, (csr[0], csr[1], np.where(np.isnan(csr[2]), dt(-7.5), csr[2])), ncol) for name, (csr, ncol) in fam.items()}
    tmp = []

    def keep(pair):
        tmp.append(pair[0])
        return pair[0]
    try:
        one = made["one"]
        for name in ("ragged", "dense", "column", "row", "empty"):
            a = made[name]
            _same(keep(a.kron(one, "first")), a)          # a (x) 1 is a
            _same(keep(one.kron(a, "second")), a)         # 1 (x) b is b
        for an, bn in (("ragged", "dense"), ("column", "ragged"), ("row", "ragged")):
            a, b = made[an], made[bn]
            ab = keep(a.kron(b))
            # (a (x) b)^T = a^T (x) b^T
            _same(keep(ab.transpose()), keep(keep(a.transpose()).kron(keep(b.transpose()))))
            # the rows' counts are the outer product of the counts
            want = np.outer(np.diff(fam[an][0][0]), np.diff(fam[bn][0][0])).reshape(-1)
            assert np.array_equal(ab.reduce("rows", "count")[0].astype(np.int64), want)
            # associativity: the structure always, the values where the operator is associative in bits -- FIRST, and MIN and
            # MAX on operands without NaNs (y < x ? y : x keeps the leftmost of the smallest values however the fold is
            # grouped, but a NaN hides what stands behind it: min(min(2, NaN), 1) = 1 and min(2, min(NaN, 1)) = 2)
            x, y, z = nn[an], nn[bn], nn["dense"]
            for op in model.OPS:
                left, right = keep(keep(x.kron(y, op)).kron(z, op)), keep(x.kron(keep(y.kron(z, op)), op))
                assert np.array_equal(left.rowptr, right.rowptr) and np.array_equal(left.colidx, right.colidx)
                if op in ("min", "max", "first"):
                    assert np.array_equal(_bits(left.vals), _bits(right.vals)), op
            while tmp:
                tmp.pop().close()
    finally:
        for x in list(made.values()) + list(nn.values()) + tmp:
            x.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_mixed_product_property(mctx, dt):
    """(a (x) b)(c (x) d) = (a c) (x) (b d), in bits with small positive integer values: every sum is exact, and none
    is a zero, whose sign would depend on the side (a sum that cancels is +0, and +0 times a negative value is -0)."""
    rng = np.random.default_rng(22)

    def rand(m, n, density):
        lists = [np.flatnonzero(rng.random(n) < density) for _ in range(m)]
        rowptr, col, _ = kc.csr_of(lists, dt, 0)
        return (rowptr, col, rng.integers(1, 4, len(col)).astype(dt)), n
    (a, na), (c, nc), (b, nb), (d, nd) = rand(6, 9, 0.4), rand(9, 5, 0.4), rand(7, 4, 0.5), rand(4, 8, 0.5)
    A, B, Cc, D = (kc.build(mctx, x, n) for x, n in ((a, na), (b, nb), (c, nc), (d, nd)))
    tmp = []
    try:
        ab, cd = A.kron(B)[0], Cc.kron(D)[0]
        tmp += [ab, cd]
        left = ab.mxm(cd)[0]
        tmp.append(left)
        ac, bd = A.mxm(Cc)[0], B.mxm(D)[0]
        tmp += [ac, bd]
        right = ac.kron(bd)[0]
        tmp.append(right)
        assert left.nnz > 0
        _same(left, right)
    finally:
        for x in [A, B, Cc, D] + tmp:
            x.close()


# ---- the pool -----------------------------------------------------------------------------------------------------------------------------
_state = {"digest": None, "stop": None}


def test_the_slice_in_this_process(mctx):
    _state["digest"] = kc.slice_digest(mctx)
    assert _state["digest"][1] == 2 * len(kc.SLICE) * len(model.OPS)


def _child(mode):
    if _state["stop"]:
        pytest.skip(f"{_state['stop']}: nothing further is started on the GPU")
    assert _state["digest"] is not None, "the in-process run did not finish: no digest to compare with"
    env = dict(os.environ)
    env[mode] = "1"
    try:
        r = subprocess.run([sys.executable, "-m", "tests.kron_cases"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _state["stop"] = f"the child under {mode} hung"
        raise
    if r.returncode != 0:
        _state["stop"] = f"the child under {mode} ended with status {r.returncode}"
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("KRON_SLICE ")]
    assert line == [f"KRON_SLICE {_state['digest'][0]} calls={_state['digest'][1]}"], r.stdout[-2000:]
    return r


def test_the_slice_in_a_child_under_poison():
    _child("OSP_POISON")


def test_the_slice_in_a_child_under_guard():
    r = _child("OSP_GUARD")
    assert "[osp] OSP_GUARD:" not in r.stderr, r.stderr[-4000:]
