"""osp_csr_draw on the GPU against the numpy model of tests/scan_model.py: columns and positions exact, over the operand
family of tests/scan_cases.py (every seventh entry a special value: NaNs, infinities, zeros and negatives weigh nothing) with
1, 2, 7 and 64 draws, two seeds, both dtypes, host and device outputs; the tie to the device's own ``scan("plus")``; rows that
cannot be drawn from; one positive entry among 3000 zeros; denormal totals; 2^20 rows of one entry; the independence of rows;
the refusals; and the draws' slice in children on a poisoned and on a guarded pool."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import spgemm as S
from tests import scan_cases as sc
from tests import scan_model as model
from tests import test_gpu_apply_mask as am   # _dev and DEV only

pytestmark = pytest.mark.gpu

DEV = am.DEV
DTS = [np.float32, np.float64]
COUNTERS = ("nnz_in", "nnz_out", "launches", "readbacks")
CHILD_TIMEOUT_S = 180   # a hang guard: a child starts Python, loads the library, creates a context and makes 72 small draws


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _check(A, csr, ncol, draws, seed, space):
    want_cols, want_pos, without = model.draw(csr, draws, seed)
    cols, pos, st = A.draw(draws, seed=seed, positions=True, space=space)
    if space == "device":
        assert cols.dtype == torch.int64 and cols.device.type == "cuda" and tuple(cols.shape) == want_cols.shape
        cols, pos = cols.cpu().numpy(), pos.cpu().numpy()
    assert cols.dtype == np.int64 and pos.dtype == np.int64
    assert np.array_equal(pos, want_pos), (draws, seed, np.argwhere(pos != want_pos)[:5])
    assert np.array_equal(cols, want_cols)
    hit = pos >= 0
    assert np.array_equal(cols[hit], csr[1][pos[hit]]) and (cols[~hit] == -1).all()      # cols == colidx[pos]
    w = model.weights(csr[2])
    assert (w[pos[hit]] > 0).all()
    assert st["rows_without"] == without == int((~hit[:, 0]).sum())
    assert {k: st[k] for k in COUNTERS} == model.draw_stats(csr, ncol, draws)
    only, st2 = A.draw(draws, seed=seed, space=space)                                       # without positions: the same columns
    only = only.cpu().numpy() if space == "device" else only
    assert np.array_equal(only, want_cols) and st2["rows_without"] == without


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("space", ["host", "device"])
def test_draw_equals_the_model_over_the_family(mctx, space, dt):
    assert sc.DRAWS == (1, 2, 7, 64)
    for name, (csr, ncol) in sc.family(dt).items():
        A = sc.build(mctx, csr, ncol)
        try:
            for draws in sc.DRAWS:
                for seed in (0, (1 << 64) - 3):
                    _check(A, csr, ncol, draws, seed, space)
            assert np.array_equal(model.bits(A.vals), model.bits(csr[2]))    # the operand stays valid
        finally:
            A.close()


@pytest.mark.parametrize("dt", DTS)
def test_the_draws_are_the_bisection_of_the_device_s_own_scan(mctx, dt):
    """A clean positive operand: the CDF that osp_csr_draw bisects is osp_csr_scan's PLUS scan, to the bit."""
    csr, ncol = sc.family(dt)["edges positive"]
    rowptr, col, val = csr
    A = sc.build(mctx, csr, ncol)
    try:
        cdf, _ = A.scan("plus")
        S_ = cdf.vals
        cdf.close()
        draws, seed = 7, 11
        cols, pos, st = A.draw(draws, seed=seed, positions=True, space="host")
        s0 = np.uint64(model.mix(seed + model.GOLDEN))
        d = np.arange(draws, dtype=np.uint64)
        for i in range(len(rowptr) - 1):
            b, e = rowptr[i], rowptr[i + 1]
            if e == b or not S_[e - 1] > 0:
                assert (pos[i] == -1).all()
                continue
            t = (model.uniform(model.mix_array(s0 ^ ((np.uint64(i) << np.uint64(32)) | d)), dt) * S_[e - 1]).astype(dt)
            assert [int(p - b) for p in pos[i]] == [model.pick(S_[b:e], x) for x in t], i
            assert np.array_equal(cols[i], col[pos[i]])
    finally:
        A.close()


@pytest.mark.parametrize("dt", DTS)
def test_rows_that_cannot_be_drawn_from_and_one_entry_among_zeros(mctx, dt):
    big = np.finfo(dt).max
    rows = [[0.0] * 5, [np.nan] * 40, [-1.0, -2.5, -np.inf], [0.75 * big, 0.75 * big], [], [np.inf, 1.0e30],
            [0.0] * 1700 + [2.5] + [0.0] * 1300,            # one positive entry among 3000 zeros
            [0.0, 0.0, 4.0], [4.0, 0.0, 0.0], [-0.0, np.nan, 3.0, np.inf, -7.0, 1.0]]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([np.arange(len(r)) * 3 + 2 for r in rows]).astype(np.uint32)
    val = np.array([x for r in rows for x in r], dt)
    csr = (rowptr, col, val)
    A = sc.build(mctx, csr, 3 * 3001 + 5)
    try:
        for draws in (1, 64, 300):
            _check(A, csr, 3 * 3001 + 5, draws, 4, "host")
        cols, pos, st = A.draw(300, seed=4, positions=True, space="host")
        assert st["rows_without"] == 5 and (cols[:5] == -1).all() and (pos[:5] == -1).all()
        assert (pos[5] == rowptr[5] + 1).all()                                   # the infinity weighs nothing, the number is drawn
        assert (pos[6] == rowptr[6] + 1700).all() and (cols[6] == 1700 * 3 + 2).all()
        assert (pos[7] == rowptr[7] + 2).all() and (pos[8] == rowptr[8]).all()
        assert set((pos[9] - rowptr[9]).tolist()) == {2, 5}
    finally:
        A.close()


def test_denormal_totals_in_f32(mctx):
    """Weights of 2^-140: the total is denormal, u * total rounds to a multiple of 2^-149, and every entry is still reached."""
    w = np.full(6, 2.0 ** -140, np.float32)
    assert w[0] > 0 and w.sum() < np.finfo(np.float32).tiny
    csr = (np.array([0, 6, 6, 9], np.int64), np.array([0, 1, 2, 3, 4, 5, 1, 3, 5], np.uint32), np.concatenate([w, w[:3]]))
    A = sc.build(mctx, csr, 6)
    try:
        _check(A, csr, 6, 64, 2, "host")
        cols, st = A.draw(600, seed=2, space="host")
        assert st["rows_without"] == 1 and set(cols[0].tolist()) == set(range(6)) and set(cols[2].tolist()) == {1, 3, 5}
    finally:
        A.close()


@pytest.mark.parametrize("dt", DTS)
def test_one_draw_on_a_million_rows_of_one_entry(mctx, dt):
    M = 1 << 20
    rng = np.random.default_rng(7)
    val = rng.random(M).astype(dt) + dt(0.5)
    val[::1000] = 0                                    # these rows cannot be drawn from
    col = rng.integers(0, 50, M).astype(np.uint32)
    csr = (np.arange(M + 1, dtype=np.int64), col, val)
    A = sc.build(mctx, csr, 50)
    try:
        cols, pos, st = A.draw(1, seed=3, positions=True)
        cols, pos = cols.cpu().numpy()[:, 0], pos.cpu().numpy()[:, 0]
        ok = val > 0
        assert np.array_equal(pos, np.where(ok, np.arange(M), -1)) and np.array_equal(cols, np.where(ok, col.astype(np.int64), -1))
        assert st["rows_without"] == int((~ok).sum()) and st["nnz_out"] == M
        assert (st["launches"], st["readbacks"]) == (3 + 1 + 2 + 1 + 2, 1)    # the table's scan is three kernels beyond 32768 rows
    finally:
        A.close()


@pytest.mark.parametrize("dt", DTS)
def test_changing_one_row_leaves_every_other_row_s_draws_unchanged(mctx, dt):
    csr, ncol = sc.family(dt)["edges positive"]
    rowptr, col, val = csr
    i = 9
    changed = val.copy()
    changed[rowptr[i]:rowptr[i + 1]] = np.random.default_rng(8).random(rowptr[i + 1] - rowptr[i]).astype(dt) + dt(0.1)
    A, B_ = sc.build(mctx, csr, ncol), sc.build(mctx, (rowptr, col, changed), ncol)
    try:
        a, pa, _ = A.draw(7, seed=5, positions=True, space="host")
        b, pb, _ = B_.draw(7, seed=5, positions=True, space="host")
        keep = np.arange(len(rowptr) - 1) != i
        assert np.array_equal(a[keep], b[keep]) and np.array_equal(pa[keep], pb[keep]) and not np.array_equal(pa[i], pb[i])
        c, _ = A.draw(7, seed=6, space="host")
        assert not np.array_equal(a, c)
        two, _ = A.draw(2, seed=5, space="host")        # a draw depends on its number, not on how many are asked for
        assert np.array_equal(two, a[:, :2])
    finally:
        A.close()
        B_.close()


# ---- outputs and refusals ------------------------------------------------------------------------------------------------------------
def _raw(a, draws=1, cols=True, space=_lib.OSP_HOST, reserved=None, reserved0=0, n=64):
    """osp_csr_draw itself.  Returns (status, whether cols, pos and *stats are as they were)."""
    c, p = np.full(n, 55, np.int64), np.full(n, 66, np.int64)
    st = _lib.DrawStats()
    st.nnz_in = 77
    spec = _lib.Draw()
    spec.draws, spec.reserved0 = draws, reserved0
    if reserved is not None:
        spec.reserved[reserved] = 1
    rc = _lib.lib().osp_csr_draw(a._h, ctypes.byref(spec), ctypes.c_void_p(c.ctypes.data) if cols else None, ctypes.c_void_p(p.ctypes.data), space,
                                 ctypes.byref(st))
    if rc != 0:
        assert _lib.lib().osp_last_error_string()
    return rc, bool((c == 55).all() and (p == 66).all() and st.nnz_in == 77)


def test_refusals_leave_the_outputs_and_stats_untouched(mctx):
    csr, ncol = sc.family(np.float64)["dense"]
    A = sc.build(mctx, csr, ncol)
    try:
        M = A.shape[0]
        assert _raw(A, draws=0) == (_lib.ERR_ARG, True)
        assert _raw(A, cols=False) == (_lib.ERR_ARG, True)
        assert _raw(A, space=2) == (_lib.ERR_ARG, True)
        assert _raw(A, reserved0=1) == (_lib.ERR_ARG, True)
        for word in range(8):
            assert _raw(A, reserved=word) == (_lib.ERR_ARG, True), word
        assert _raw(A, draws=2, n=2 * M) == (0, False)        # and the library still works
        for bad in (0, 1 << 32, -1, 1.5):
            with pytest.raises(ValueError):
                A.draw(bad)
        # caller's outputs: filled and returned; the wrong shape or dtype is refused before anything runs
        out, out_pos = np.full((M, 3), 9, np.int64), np.full((M, 3), 9, np.int64)
        cols, pos, st = A.draw(3, seed=1, out=out, out_pos=out_pos, space="host")
        assert cols is out and pos is out_pos
        want = model.draw(csr, 3, 1)
        assert np.array_equal(out, want[0]) and np.array_equal(out_pos, want[1])
        t = torch.full((M, 3), 9, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize(DEV)
        cols, st = A.draw(3, seed=1, out=t)
        assert cols is t and np.array_equal(t.cpu().numpy(), want[0])
        for bad in (np.zeros((M, 2), np.int64), np.zeros((M, 3), np.int32), np.zeros(3 * M, np.int64)):
            with pytest.raises(S.OspError):
                A.draw(3, out=bad, space="host")
        with pytest.raises(S.OspError):
            A.draw(3, out=torch.zeros((M, 3), dtype=torch.float64, device=DEV))
        # without stats there is no read-back to pin from outside, but the call is legal and fills the same columns
        c = np.full(M * 3, 55, np.int64)
        spec = _lib.Draw()
        spec.draws, spec.seed = 3, 1
        assert _lib.lib().osp_csr_draw(A._h, ctypes.byref(spec), ctypes.c_void_p(c.ctypes.data), None, _lib.OSP_HOST, None) == 0
        assert np.array_equal(c.reshape(M, 3), want[0])
    finally:
        A.close()


@pytest.mark.parametrize("dt", DTS)
def test_the_empty_operands(mctx, dt):
    """M == 0 (an extract of no rows) and nnz == 0: no kernel, every draw is -1."""
    A = sc.build(mctx, *sc.family(dt)["ragged"])
    E = sc.build(mctx, *sc.family(dt)["empty"])
    Z = A.extract(rows=np.zeros(0, np.int64), space="host")[0]
    try:
        assert Z.shape[0] == 0 and E.nnz == 0 and E.shape[0] == 4
        for src in (Z, E):
            M0 = src.shape[0]
            for space in ("host", "device"):
                cols, pos, st = src.draw(3, positions=True, space=space)
                cols, pos = (cols.cpu().numpy(), pos.cpu().numpy()) if space == "device" else (cols, pos)
                assert cols.shape == (M0, 3) and (cols == -1).all() and (pos == -1).all()
                assert (st["launches"], st["readbacks"], st["rows_without"], st["nnz_out"]) == (0, 0, M0, 3 * M0)
    finally:
        for x in (A, E, Z):
            x.close()


# ---- the pool -----------------------------------------------------------------------------------------------------------------------------
_state = {"digest": None, "stop": None}


def test_the_draw_slice_in_this_process(mctx):
    _state["digest"] = sc.draw_slice_digest(mctx)
    assert _state["digest"][1] == 2 * len(sc.DRAW_SLICE) * len(sc.DRAW_SLICE_DRAWS) * 2


def _child(mode):
    assert not _state["stop"], f"{_state['stop']}: nothing further is started on the GPU"
    assert _state["digest"] is not None, "the in-process run did not finish: no digest to compare with"
    env = dict(os.environ)
    env[mode] = "1"
    try:
        r = subprocess.run([sys.executable, "-m", "tests.scan_cases", "draw"], cwd=sc.ROOT, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _state["stop"] = f"the child under {mode} hung"
        raise
    if r.returncode != 0:
        _state["stop"] = f"the child under {mode} ended with status {r.returncode}"
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("DRAW_SLICE ")]
    assert line == [f"DRAW_SLICE {_state['digest'][0]} calls={_state['digest'][1]}"], r.stdout[-2000:]
    return r


def test_the_draw_slice_in_a_child_under_poison():
    _child("OSP_POISON")


def test_the_draw_slice_in_a_child_under_guard():
    r = _child("OSP_GUARD")
    assert "[osp] OSP_GUARD:" not in r.stderr, r.stderr[-4000:]
