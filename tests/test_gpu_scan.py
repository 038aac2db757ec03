"""osp_csr_scan on the GPU against the numpy model of tests/scan_model.py: row pointers and columns exact, values equal to the
BIT (a NaN where the model has one: which NaN an addition returns the header leaves open), and the stats counters the model's.
Operands go up through ``Context.build(dup="error")`` and every seventh entry of the family carries a special value.  The
sweep over the operand family, row lengths at the edges of one, two, 16/17 and 64/128 blocks, layouts around the local pass's
workgroup tile, many short rows, empty rows by the million, one row of 2^20 + 5 entries, IEEE edge values, wide columns, the
identities that tie the scan to ``reduce`` and ``extract`` and to itself, the pinned stats, the refusals, and a slice of the
sweep in children on a poisoned and on a guarded pool."""
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
from tests import scan_cases as sc
from tests import scan_model as model
from tests import test_gpu_apply_mask as am   # _dev and DEV only
from tests import wide_columns as wc

pytestmark = pytest.mark.gpu

ROOT = sc.ROOT
DEV = am.DEV
B = model.BLOCK
TILE = model.LOCAL_TILE      # blocks of one workgroup of the local pass
CHILD_TIMEOUT_S = 180        # a hang guard: a child starts Python, loads the library, creates a context and makes 60 small calls
COUNTERS = ("nnz_in", "nnz_out", "blocks", "launches", "readbacks")
DTS = [np.float32, np.float64]


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _check(res, st, src, csr, ncol, op):
    want = model.scan(csr, op)[2]
    assert res.shape == src.shape and res.dtype == csr[2].dtype.type and res.nnz == len(csr[1])
    assert np.array_equal(res.rowptr, csr[0])
    assert np.array_equal(res.colidx, csr[1])
    got = res.vals
    assert model.same(got, want), (op, np.flatnonzero(model.bits(got) != model.bits(want))[:8])
    if op != "plus":
        assert not np.isnan(got).any()
    assert {name: st[name] for name in COUNTERS} == model.scan_stats(csr, ncol), op
    assert st["ms_total"] >= 0
    info, base = dict(res.info), dict(src.info)     # in's info with ms_total replaced
    assert info.pop("ms_total") == st["ms_total"]
    base.pop("ms_total")
    assert info == base


def _sweep(mctx, csr, ncol, ops=model.OPS):
    """Uploads the operand and checks every op against the model; closes everything."""
    A = sc.build(mctx, csr, ncol)
    try:
        for op in ops:
            res, st = A.scan(op)
            try:
                _check(res, st, A, csr, ncol, op)
            finally:
                res.close()
        # the operand stays valid
        assert np.array_equal(A.rowptr, csr[0]) and np.array_equal(A.colidx, csr[1]) and np.array_equal(model.bits(A.vals), model.bits(csr[2]))
    finally:
        A.close()


def _rows(lengths, ncol, dt, seed):
    return sc.csr_of(sc.random_rows(lengths, ncol, seed), dt, seed)


def _plain(lengths, dt, seed, ncol=None):
    """Rows of the given lengths on columns 0 .. m - 1, normal values (cheap to make when the rows are long or many)."""
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.arange(m, dtype=np.uint32) for m in lengths] + [np.zeros(0, np.uint32)])
    return (rowptr, col, rng.standard_normal(len(col)).astype(dt)), int(max(max(lengths, default=0), 1) if ncol is None else ncol)


def _one_row(vals, cols=None):
    vals = np.asarray(vals)
    cols = np.arange(len(vals)) if cols is None else np.asarray(cols)
    return np.array([0, len(vals)], np.int64), cols.astype(np.uint32), vals


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", model.OPS)
def test_scan_equals_the_model_over_the_family(mctx, op, dt):
    for name, (csr, ncol) in sc.family(dt).items():
        _sweep(mctx, csr, ncol, [op])


# ---- row lengths at the edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_row_lengths_around_one_and_two_blocks_the_chain_s_paths_and_its_loads(mctx, dt):
    """0, 1, 31..33, 63..65: one and two blocks; 511..513, 544, 545: the chain's lane and wave paths (16 and 17 blocks);
    2047..2049 and 4095..4097: 64 blocks, one load of the chain's wave path, and two.  Each length also alone in its operand:
    nothing before or after it."""
    assert (B, model.CHAIN_LANE) == (32, 16)
    assert set([0, 1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 544, 545, 2047, 2048, 2049, 4095, 4096, 4097]) <= set(sc.BLOCK_EDGES)
    for m in sc.BLOCK_EDGES:
        _sweep(mctx, _rows([m], max(m, 1) + 3, dt, 20 + m), max(m, 1) + 3)
    _sweep(mctx, _rows(sc.BLOCK_EDGES[::-1], 130 * B, dt, 19), 130 * B)


@pytest.mark.parametrize("dt", DTS)
def test_layouts_around_the_local_pass_s_tile(mctx, dt):
    """A workgroup of the local pass owns 128 consecutive blocks: rows that end one entry before, at and after its last
    block's end, a row whose first block is the tile's last, and tiles made of one-entry blocks."""
    full = TILE * B
    for lengths in ([full - 1], [full], [full + 1], [full - B, 100], [full - B - 1, 100], [full - B + 1, 100], [full - 1, 1, 70], [full, 1, 70],
                    [1] * (TILE - 1) + [70], [1] * TILE + [70], [1] * (TILE + 1) + [70], [0, B, 0, 0, full - B, 0, 33, 0]):
        csr, ncol = _plain(lengths, dt, len(lengths))
        _sweep(mctx, csr, ncol, ("plus", "min"))


@pytest.mark.parametrize("dt", DTS)
def test_5000_rows_of_two_blocks_the_second_of_one_entry(mctx, dt):
    csr, ncol = _plain([33] * 5000, dt, 3)
    _sweep(mctx, csr, ncol)


@pytest.mark.parametrize("dt", DTS)
def test_a_million_empty_rows_around_three_full_ones_and_the_empty_operands(mctx, dt):
    M = 1 << 20
    lengths = np.zeros(M, np.int64)
    lengths[[0, M // 2, M - 1]] = [40, 700, 33]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.arange(40), np.arange(700), np.arange(33)]).astype(np.uint32)
    val = np.random.default_rng(4).standard_normal(len(col)).astype(dt)
    _sweep(mctx, (rowptr, col, val), 700, ("plus", "max"))
    # M == 0 (an extract of no rows) and nnz == 0: no kernel
    A = sc.build(mctx, *sc.family(dt)["ragged"])
    E = sc.build(mctx, *sc.family(dt)["empty"])
    Z = A.extract(rows=np.zeros(0, np.int64), space="host")[0]
    try:
        assert Z.shape[0] == 0 and E.nnz == 0 and E.shape[0] == 4
        for src in (Z, E):
            for op in model.OPS:
                res, st = src.scan(op)
                try:
                    assert res.shape == src.shape and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(src.shape[0] + 1, np.int64))
                    assert (st["launches"], st["readbacks"], st["nnz_out"], st["blocks"]) == (0, 0, 0, src.shape[0])
                finally:
                    res.close()
    finally:
        for x in (A, E, Z):
            x.close()


@pytest.mark.parametrize("dt", DTS)
def test_one_row_of_2_to_the_20_plus_5_entries(mctx, dt):
    """32769 blocks: 513 loads of the chain's wave path.  Non-negative values: the scan is also monotone."""
    n = (1 << 20) + 5
    rng = np.random.default_rng(5)
    val = np.ldexp(rng.random(n) + 0.5, rng.integers(-30, 31, n)).astype(dt)
    val[rng.random(n) < 0.2] = 0
    csr = _one_row(val)
    A = sc.build(mctx, csr, n)
    try:
        for op in model.OPS:
            res, st = A.scan(op)
            try:
                print(f"one row of 2^20 + 5, {np.dtype(dt).name}, {op}: {st['ms_total']:.3f} ms")
                _check(res, st, A, csr, n, op)
                if op == "plus":
                    got = res.vals
                    assert np.all(got[1:] >= got[:-1])
                    zero = np.flatnonzero(val[1:] == 0) + 1
                    assert np.array_equal(model.bits(got[zero]), model.bits(got[zero - 1]))
            finally:
                res.close()
    finally:
        A.close()


# ---- special values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_ieee_edge_values(mctx, dt):
    tiny = np.finfo(dt).smallest_subnormal
    nan, inf = np.nan, np.inf
    rows = [[-0.0, -0.0, 0.0, -0.0, 1.0, -1.0, -0.0],                      # a leading -0.0 reads +0.0 under PLUS
            [inf, 1.0, -inf, 2.0],                                          # +inf then -inf: NaN from there on under PLUS
            [nan, nan, 3.0, -nan, 1.0, 5.0],                                # a leading NaN: the identity under MIN and MAX
            [-nan, -inf, inf],
            [tiny, tiny, -tiny, 3 * tiny, 0.0, np.finfo(dt).tiny],          # denormals
            [np.finfo(dt).max, np.finfo(dt).max, -np.finfo(dt).max],        # overflow to +inf, then inf - max
            [1.0] * 31 + [nan] + [2.0] * 40,                                # a NaN in the last position of a block
            [1.0] * 32 + [nan] + [2.0] * 40,                                # and in the first of the next
            [nan] * 70,
            [-0.0] * 40,
            [1.0, 2.0 ** -24, 2.0 ** -24, 0.0] * 20]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([np.arange(len(r)) for r in rows]).astype(np.uint32)
    val = np.array([x for r in rows for x in r], dt)
    csr = (rowptr, col, val)
    _sweep(mctx, csr, 80)
    plus, low, high = (model.scan(csr, op)[2] for op in model.OPS)
    assert not np.signbit(plus[0]) and not np.signbit(plus[1]) and np.isnan(plus[rowptr[1] + 2:rowptr[2]]).all()
    assert (low[rowptr[2]:rowptr[2] + 2] == inf).all() and (high[rowptr[2]:rowptr[2] + 2] == -inf).all()
    assert not np.isnan(plus[rowptr[6]:rowptr[6] + 31]).any() and np.isnan(plus[rowptr[6] + 31:rowptr[7]]).all()
    assert not np.isnan(plus[rowptr[7]:rowptr[7] + 32]).any() and np.isnan(plus[rowptr[7] + 32:rowptr[8]]).all()
    assert (low[rowptr[8]:rowptr[9]] == inf).all()


@pytest.mark.parametrize("dt", DTS)
def test_monotone_on_adversarial_magnitudes(mctx, dt):
    """Non-negative entries from 2^-60 to 2^60, a fifth of them zero, rows up to 5000 entries: S never decreases and a zero
    entry repeats the value before it, on the device as in the model."""
    rng = np.random.default_rng(6)
    lengths = [int(x) for x in rng.integers(1, 400, 60)] + [5000, 3000, 1025]
    (rowptr, col, _), ncol = _plain(lengths, dt, 7)
    val = np.ldexp(rng.random(len(col)) + 0.5, rng.integers(-60, 61, len(col))).astype(dt)
    val[rng.random(len(col)) < 0.2] = 0
    csr = (rowptr, col, val)
    A = sc.build(mctx, csr, ncol)
    try:
        res, st = A.scan("plus")
        try:
            _check(res, st, A, csr, ncol, "plus")
            got = res.vals
            for i in range(len(lengths)):
                s, v = got[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]]
                assert np.all(s[1:] >= s[:-1]), i
                zero = np.flatnonzero(v[1:] == 0) + 1
                assert np.array_equal(model.bits(s[zero]), model.bits(s[zero - 1])), i
        finally:
            res.close()
    finally:
        A.close()


# ---- wide columns --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_columns_on_both_sides_of_bit_31_are_copied(mctx, dt):
    N = (1 << 32) - 1
    narrow = _rows([90, 3, 0, 130, 2100], 3 * 2048, dt, 44)
    csr = wc.relabel_csr(narrow, wc.phi("straddle", 3 * 2048, N))
    first = csr[1][:90].astype(np.int64)
    assert (first < (1 << 31)).any() and (first >= (1 << 31)).any()
    _sweep(mctx, csr, N)


# ---- identities on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_identities_on_the_device(mctx, dt):
    rng = np.random.default_rng(8)
    lengths = [0, 5, 32, 33, 64, 300, 513, 2100, 1, 17, 4100]
    (rowptr, col, _), ncol = _plain(lengths, dt, 9)
    val = (rng.random(len(col)) + 0.25).astype(dt)     # positive, NaN-free
    csr = (rowptr, col, val)
    A = sc.build(mctx, csr, ncol)
    made = [A]
    try:
        # the last value of a row under MAX is reduce("rows", "max")
        smax, _ = A.scan("max")
        made.append(smax)
        red, _ = A.reduce("rows", "max")
        got = smax.vals
        ends = rowptr[1:][np.diff(rowptr) > 0] - 1
        assert np.array_equal(model.bits(got[ends]), model.bits(red[np.diff(rowptr) > 0]))
        # position independence: a row's scan is the scan of the same values in a one-row operand
        for op in model.OPS:
            whole, _ = A.scan(op)
            made.append(whole)
            w = whole.vals
            for i in (3, 6, 7, 10):
                lone = sc.build(mctx, _one_row(val[rowptr[i]:rowptr[i + 1]]), ncol)
                made.append(lone)
                one, _ = lone.scan(op)
                made.append(one)
                assert np.array_equal(model.bits(one.vals), model.bits(w[rowptr[i]:rowptr[i + 1]])), (op, i)
            # scan of an extract of rows equals the rows of the scan
            pick = np.array([7, 3, 3, 0, 10, 5], np.int32)
            ex, _ = A.extract(rows=pick, space="host")
            made.append(ex)
            sx, _ = ex.scan(op)
            made.append(sx)
            xs, _ = whole.extract(rows=pick, space="host")
            made.append(xs)
            assert np.array_equal(sx.rowptr, xs.rowptr) and np.array_equal(sx.colidx, xs.colidx)
            assert np.array_equal(model.bits(sx.vals), model.bits(xs.vals)), op
    finally:
        torch.cuda.synchronize(DEV)
        for x in made:
            x.close()


# ---- stats -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths,ncol,blocks,launches", [([3, 0, 32, 5], 40, 5, 4), ([33, 0, 2048], 2048, 68, 4), ([2, 2049, 2], 2049, 67, 4),
                                                          ([3, 0, 32, 5], 32, 5, 2), ([1] * 70000, 1, 70000 // 32 + 70000, 4)])
def test_stats_are_pinned(mctx, lengths, ncol, blocks, launches):
    """launches: the block table's scan (1 kernel up to 32768 rows, 3 beyond), the local pass, and -- when min(N, nnz) > 32 --
    the chain and the add.  Nothing is read back; blocks is the host's bound nnz // 32 + M."""
    csr, _ = _plain(lengths, np.float64, 10, ncol)
    A = sc.build(mctx, csr, ncol)
    try:
        for op in model.OPS:
            res, st = A.scan(op)
            res.close()
            assert {k: st[k] for k in COUNTERS} == {"nnz_in": sum(lengths), "nnz_out": sum(lengths), "blocks": blocks, "launches": launches,
                                                    "readbacks": 0}
            assert model.scan_stats(csr, ncol) == {k: st[k] for k in COUNTERS}
    finally:
        A.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(a, op=0, reserved=None):
    """osp_csr_scan itself.  Returns (status, whether *out and *stats are as they were), or (0, the handle)."""
    sentinel = 0x1234
    o = ctypes.c_void_p(sentinel)
    st = _lib.ScanStats()
    st.nnz_in = 77
    spec = _lib.Scan()
    spec.op = op
    if reserved is not None:
        spec.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_scan(a._h, ctypes.byref(spec), ctypes.byref(o), ctypes.byref(st))
    if rc == 0:
        return rc, o
    assert _lib.lib().osp_last_error_string()
    return rc, o.value == sentinel and st.nnz_in == 77


def test_refusals_leave_out_and_stats_untouched(mctx):
    csr, ncol = sc.family(np.float64)["ragged"]
    A = sc.build(mctx, csr, ncol)
    try:
        for op in (-1, 3, 4, 1 << 20):          # 3 is COUNT
            assert _raw(A, op) == (_lib.ERR_ARG, True), op
        for word in range(8):
            assert _raw(A, reserved=word) == (_lib.ERR_ARG, True), word
        with pytest.raises(ValueError):
            A.scan("count")
        rc, o = _raw(A, 1)                       # and the library still works
        assert rc == 0
        got = S.CsrResult(mctx, o)
        assert model.same(got.vals, model.scan(csr, "min")[2])
        got.close()
        # without stats
        o = ctypes.c_void_p()
        spec = _lib.Scan()
        assert _lib.lib().osp_csr_scan(A._h, ctypes.byref(spec), ctypes.byref(o), None) == 0
        got = S.CsrResult(mctx, o)
        assert model.same(got.vals, model.scan(csr, "plus")[2])
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
        for call in (lambda: part.scan("plus"), lambda: part.draw(1)):
            with pytest.raises(S.OspError) as ei:
                call()
            assert ei.value.status == _lib.ERR_ARG
    finally:
        part.close()


# ---- the pool -----------------------------------------------------------------------------------------------------------------------------
_state = {"digest": None, "stop": None}


def test_the_slice_in_this_process(mctx):
    _state["digest"] = sc.slice_digest(mctx)
    assert _state["digest"][1] == 2 * len(sc.SLICE) * (len(model.OPS) + len(sc.SLICE_DRAWS))


def _child(mode):
    assert not _state["stop"], f"{_state['stop']}: nothing further is started on the GPU"
    assert _state["digest"] is not None, "the in-process run did not finish: no digest to compare with"
    env = dict(os.environ)
    env[mode] = "1"
    try:
        r = subprocess.run([sys.executable, "-m", "tests.scan_cases"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _state["stop"] = f"the child under {mode} hung"
        raise
    if r.returncode != 0:
        _state["stop"] = f"the child under {mode} ended with status {r.returncode}"
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("SCAN_SLICE ")]
    assert line == [f"SCAN_SLICE {_state['digest'][0]} calls={_state['digest'][1]}"], r.stdout[-2000:]
    return r


def test_the_slice_in_a_child_under_poison():
    _child("OSP_POISON")


def test_the_slice_in_a_child_under_guard():
    r = _child("OSP_GUARD")
    assert "[osp] OSP_GUARD:" not in r.stderr, r.stderr[-4000:]
