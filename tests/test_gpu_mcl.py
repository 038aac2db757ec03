"""osp_csr_inflate_prune and graph.markov_cluster on the GPU against the numpy model of tests/mcl_model.py: row pointers
and columns equal, values and chaos bit for bit (the header defines the order of additions), on host-built rows made for
every rule of the step and both row classes, on a product's result, through the result's other entry points, and the
whole loop on planted partitions and on an R-MAT graph."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import mcl_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the row length that separates the two row classes (rows longer than it get a workgroup each)
LONG_MIN = int(re.search(r"kMclLongMin\s*=\s*(\d+)", open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_mcl.h")).read()).group(1))
THR = 0.25          # exact in f32 and f64
NCOL = 1 << 18


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    """The session's one library context (conftest.py).  The expansions of the larger runs are multi-GB blocks that its pool
    keeps when they are released: they are given back to the device here, so that the full-size tests of other modules
    find the memory they need."""
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _rows_to_csr(rows, ncol, dt, seed=0):
    """rows: list of value arrays; columns drawn at random (ascending) per row."""
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(rows) + 1, np.int64)
    cols = []
    for i, v in enumerate(rows):
        rowptr[i + 1] = rowptr[i] + len(v)
        cols.append(np.sort(rng.choice(ncol, size=len(v), replace=False)).astype(np.uint32))
    col = np.concatenate(cols) if cols else np.zeros(0, np.uint32)
    val = np.concatenate([np.asarray(v, dt) for v in rows]) if rows else np.zeros(0, dt)
    return rowptr, col, val.astype(dt)


def _trap_rows(dt):
    """(rows, number of long-class rows): one row per rule of the step."""
    rng = np.random.default_rng(7)
    f = np.finfo(dt)
    thr = dt(THR)
    below = np.nextafter(thr, dt(0), dtype=dt)
    u = lambda n: (rng.random(n) * 0.9 + 0.05).astype(dt)
    few = lambda n: rng.choice(np.array([0.125, 0.25, 0.3, 0.5, 0.5, 0.75], dt), size=n)
    den = (rng.integers(1, 50, 40) * f.smallest_subnormal).astype(dt)   # denormals, with ties
    rows = [
        np.zeros(0, dt),                                   # 0  empty
        u(1), u(63), u(64), u(65),                         # 1-4
        u(1 << 17),                                        # 5  long: at least 2^17 entries
        u(LONG_MIN),                                       # 6  the longest one-wave row
        u(LONG_MIN + 1),                                   # 7  the shortest one-workgroup row
        np.full(300, 0.5, dt),                             # 8  all equal: the cap is decided by column alone
        few(500),                                          # 9  few distinct values: the k-th and (k+1)-th largest are equal
        np.where(rng.random(100) < 0.5, thr, below).astype(dt),   # 10 at the threshold (kept) and one ulp below (dropped)
        np.concatenate([u(30) * dt(0.2), np.full(3, 0.2, dt), u(30) * dt(0.2)]).astype(dt),   # 11 nothing reaches the threshold; the largest thrice
        np.concatenate([den, np.array([0.5], dt), den[::-1]]).astype(dt),      # 12 denormals around one normal value
        np.zeros(0, dt),                                   # 13 empty
        np.full(5000, 0.75, dt),                           # 14 long, all equal
        few(10000),                                        # 15 long, few distinct values
        np.concatenate([u(1500) * dt(0.2), np.full(2, 0.2, dt), u(1500) * dt(0.2)]).astype(dt),   # 16 long, rescued, the largest twice
        np.full(64, below, dt),                            # 17 rescued, all equal: the lowest column stays
    ] + [u(int(k)) for k in rng.integers(0, 200, 20)]
    n_long = sum(len(r) > LONG_MIN for r in rows)
    return rows, n_long


_INPUTS = {}


def _trap_input(dt):
    if dt not in _INPUTS:
        rows, n_long = _trap_rows(dt)
        _INPUTS[dt] = (_rows_to_csr(rows, NCOL, dt, seed=11), n_long, rows)
    return _INPUTS[dt]


def _check_against_model(res, st, rowptr, col, val, power, thr, cap, exact=True):
    want_ptr, want_col, want_val, want = model.inflate_prune(rowptr, col, val, power, thr, cap)
    assert res.shape == (len(rowptr) - 1, res.shape[1]) and res.nnz == want["nnz_out"] and res.dtype == val.dtype.type
    assert np.array_equal(res.rowptr, want_ptr)
    assert np.array_equal(res.colidx, want_col)
    for k in ("nnz_in", "nnz_out", "rows_capped", "rows_rescued"):
        assert st[k] == want[k], (k, st[k], want[k])
    if exact:
        assert np.array_equal(_bits(res.vals), _bits(want_val))
        assert st["chaos"] == want["chaos"]
    return want_ptr, want_col, want_val, want


# ---- the step on rows built for its rules ---------------------------------------------------------------------------------
STEPS = [(1.0, 0.0, 0), (2.0, 0.0, 0), (2.0, THR, 0), (2.0, THR, 1), (1.0, THR, 7), (2.0, 0.0, 64), (2.0, THR, 100), (1.0, 0.0, 1000),
         (2.0, 0.0, 1)]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("power,thr,cap", STEPS)
def test_inflate_prune_equals_model_bit_for_bit(mctx, dt, power, thr, cap):
    (rowptr, col, val), n_long, rows = _trap_input(dt)
    src = mctx.merge_csr_parts(len(rowptr) - 1, NCOL, [(rowptr, col, val)])
    try:
        assert np.array_equal(_bits(src.vals), _bits(val))   # the loaded input is the input
        res, st = src.inflate_prune(power, thr, cap)
        try:
            _check_against_model(res, st, rowptr, col, val, power, thr, cap)
            assert st["rows_long"] == n_long == 5
            assert res.info["M"] == len(rowptr) - 1 and res.info["N"] == NCOL and res.info["nnz_c"] == res.nnz
            assert res.info["ms_total"] > 0 and st["ms_total"] > 0 and st["launches"] >= 3
            if thr == 0.0 and cap == 0:
                assert st["nnz_out"] == st["nnz_in"] and st["rows_capped"] == 0 and st["rows_rescued"] == 0
            if thr == THR:
                # rows 11, 16 and 17 hold nothing >= THR by construction (row 12 keeps its 0.5), and a random row may
                assert st["rows_rescued"] == sum(1 for r in rows if len(r) and r.max() < dt(THR)) >= 3
            if cap == 64:
                assert np.diff(res.rowptr)[3] == 64 and np.diff(res.rowptr)[4] == 64    # exactly the length; one more than it
        finally:
            res.close()
    finally:
        src.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_row_class_boundary(mctx, dt):
    rng = np.random.default_rng(3)
    for lengths, n_long in (([LONG_MIN], 0), ([LONG_MIN + 1], 1), ([LONG_MIN, LONG_MIN + 1, 5, 0], 1)):
        rowptr, col, val = _rows_to_csr([rng.random(k).astype(dt) + dt(0.01) for k in lengths], 1 << 14, dt, seed=5)
        src = mctx.merge_csr_parts(len(lengths), 1 << 14, [(rowptr, col, val)])
        res, st = src.inflate_prune(2.0, 0.5, 33)
        try:
            assert st["rows_long"] == n_long
            _check_against_model(res, st, rowptr, col, val, 2.0, 0.5, 33)
        finally:
            res.close()
            src.close()


# ---- a product's result as input ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,scale", [(np.float64, 13), (np.float32, 12)])
def test_step_on_a_products_result(mctx, dt, scale):
    n, r, c, _ = gen.rmat_coo(scale, 8, "g500", seed=5, dtype=dt)
    ones = np.ones(len(r), dt)                       # unit values: the product's entries are small integers, full of ties
    a = S.coo_to_csc(n, r, c, ones)
    b = S.coo_to_csr(n, r, c, ones)
    prod = mctx.spgemm_csc_csr(n, n, n, *a, *b)
    try:
        rowptr, col, val = (x.copy() for x in prod.to_host())
        assert np.diff(rowptr).max() > LONG_MIN      # hub rows: both classes run
        for power, thr, cap in ((2.0, 2.0, 50), (1.0, 0.0, 200), (2.0, 3.0, 0)):
            res, st = prod.inflate_prune(power, thr, cap)
            try:
                _check_against_model(res, st, rowptr, col, val, power, thr, cap)
                assert st["rows_long"] == int((np.diff(rowptr) > LONG_MIN).sum())
            finally:
                res.close()
    finally:
        prod.close()


# ---- a general power ------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_general_power_keeps_the_pattern_of_the_square(mctx, dt):
    (rowptr, col, val), _, _ = _trap_input(dt)
    src = mctx.merge_csr_parts(len(rowptr) - 1, NCOL, [(rowptr, col, val)])
    sq, _ = src.inflate_prune(2.0, THR, 100)
    res, st = src.inflate_prune(1.5, THR, 100)
    try:
        assert np.array_equal(res.rowptr, sq.rowptr) and np.array_equal(res.colidx, sq.colidx)   # pruning precedes inflation
        want_ptr, want_col, want_val, want = _check_against_model(res, st, rowptr, col, val, 1.5, THR, 100, exact=False)
        eps = np.finfo(dt).eps
        m = np.repeat(np.diff(want_ptr), np.diff(want_ptr)).astype(np.float64)
        got = res.vals.astype(np.float64)
        rel = np.abs(got - want_val.astype(np.float64)) / want_val.astype(np.float64)
        print(f"power 1.5 {np.dtype(dt).name}: largest distance to the model {int(_ulps(res.vals, want_val).max())} ulp, "
              f"largest rel/((m+16) eps) {float((rel / ((m + 16) * eps)).max()):.3f}")
        assert np.all(rel <= (m + 16) * eps)
        assert abs(st["chaos"] - want["chaos"]) <= (np.diff(want_ptr).max() + 16) * eps
    finally:
        res.close()
        sq.close()
        src.close()


# ---- arguments ------------------------------------------------------------------------------------------------------------
def _small(mctx, vals, dt=np.float64):
    vals = np.asarray(vals, dt)
    return mctx.merge_csr_parts(1, 8, [(np.array([0, len(vals)], np.int64), np.arange(len(vals), dtype=np.uint32), vals)])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("bad", [-0.5, np.nan, np.inf])
def test_validate_refuses_negative_nan_and_infinite_values(mctx, dt, bad):
    src = _small(mctx, [0.5, bad, 0.25], dt)
    try:
        with pytest.raises(S.OspError) as ei:
            src.inflate_prune(2.0, 0.0, 0, validate=True)
        assert ei.value.status == _lib.ERR_ARG
        ok = _small(mctx, [0.5, 0.0, 0.25], dt)
        res, st = ok.inflate_prune(2.0, 0.0, 0, validate=True)
        assert st["nnz_out"] == 3
        res.close()
        ok.close()
    finally:
        src.close()


def test_bad_step_fields_and_null_arguments(mctx):
    L = _lib.lib()
    src = _small(mctx, [0.5, 0.25])
    try:
        for power, thr in ((0.5, 0.0), (np.nan, 0.0), (2.0, -1.0), (2.0, np.nan)):
            with pytest.raises(S.OspError) as ei:
                src.inflate_prune(power, thr, 0)
            assert ei.value.status == _lib.ERR_ARG
        sentinel = 0x1234
        out = ctypes.c_void_p(sentinel)
        step = _lib.MclStep()
        step.power = 2.0
        step.reserved[3] = 1
        assert L.osp_csr_inflate_prune(src._h, ctypes.byref(step), 0, ctypes.byref(out), None) == _lib.ERR_ARG
        assert out.value == sentinel
        step.reserved[3] = 0
        assert L.osp_csr_inflate_prune(src._h, None, 0, ctypes.byref(out), None) == _lib.ERR_ARG
        assert L.osp_csr_inflate_prune(src._h, ctypes.byref(step), 0, None, None) == _lib.ERR_ARG
        assert out.value == sentinel and L.osp_last_error_string()
        # a null stats pointer is fine
        assert L.osp_csr_inflate_prune(src._h, ctypes.byref(step), 0, ctypes.byref(out), None) == _lib.OSP_OK
        L.osp_result_destroy(out)
    finally:
        src.close()


def test_partials_result_is_refused(mctx):
    n, r, c, v = gen.rmat_coo(6, 4, "mild", seed=2)
    a, b = S.coo_to_csc(n, r, c, v), S.coo_to_csr(n, r, c, v)
    dev = torch.device("cuda", mctx.device)
    keep = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).to(dev) for x in (*a, *b)]
    torch.cuda.synchronize(dev)
    part = mctx.spgemm_partials_device(np.float64, n, n, n, [t.data_ptr() for t in keep])
    try:
        with pytest.raises(S.OspError) as ei:
            part.inflate_prune()
        assert ei.value.status == _lib.ERR_ARG
    finally:
        part.close()


# ---- the output is an ordinary result -------------------------------------------------------------------------------------
def test_output_feeds_the_other_entry_points(mctx, port, tmp_path):
    dt = np.float64
    n, r, c, v = gen.rmat_coo(8, 6, "mild", seed=4, dtype=dt)
    rowptr, col, val = gen.coo_to_csr(n, r, c, v)
    src = mctx.merge_csr_parts(n, n, [(rowptr, col, val)])
    out, st = src.inflate_prune(2.0, 0.6, 5)
    src.close()
    try:
        rp, ci, va = (x.copy() for x in out.to_host())
        # osp_result_coo_rows
        dev = torch.device("cuda", mctx.device)
        rows_t = torch.empty(max(out.nnz, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        out.coo_rows_into(rows_t.data_ptr())
        assert np.array_equal(rows_t.cpu().numpy()[:out.nnz], np.repeat(np.arange(n), np.diff(rp)))
        # osp_csr_bias_relu (no bias: the stored entries, zeros dropped)
        br = out.bias_relu(None, True)
        assert np.array_equal(br.rowptr, rp) and np.array_equal(_bits(br.vals), _bits(va))
        br.close()
        # osp_result_write_mtx
        path = str(tmp_path / "t.mtx")
        out.write_mtx(path)
        nr, nc, mr, mc, mv = S.read_mtx(path)
        assert (nr, nc, len(mr)) == (n, n, out.nnz)
        # a second step on the output, and a product of it (T @ T through the device hand-off), against the oracle
        again, _ = out.inflate_prune(1.0, 0.0, 0)
        assert np.array_equal(again.rowptr, rp)
        again.close()
        torch.cuda.synchronize(dev)
        _, cp, vp = out.device_ptrs()
        ptrs = (rows_t.data_ptr(), cp, vp)
        prod = mctx.spgemm_coo_device(dt, n, n, n, out.nnz, ptrs, out.nnz, ptrs)
        T = sp.csr_matrix((va, ci.astype(np.int64), rp), shape=(n, n))
        Tc = T.tocsc()
        Tc.sort_indices()
        want = port.spgemm(n, n, n, Tc.indptr.astype(np.int64), Tc.indices.astype(np.uint32), Tc.data, rp, ci, va)
        assert np.array_equal(prod.rowptr, want["rowptr"]) and np.array_equal(prod.colidx, want["colidx"])
        assert np.array_equal(_bits(prod.vals), _bits(want["vals"]))
        prod.close()
    finally:
        out.close()


# ---- the loop -------------------------------------------------------------------------------------------------------------
def _port_square(port):
    def square(n, rowptr, colidx, vals):
        Tc = sp.csr_matrix((vals, colidx.astype(np.int64), rowptr), shape=(n, n)).tocsc()
        Tc.sort_indices()
        w = port.spgemm(n, n, n, Tc.indptr.astype(np.int64), Tc.indices.astype(np.uint32), Tc.data.astype(vals.dtype), rowptr, colidx, vals)
        return w["rowptr"], w["colidx"], w["vals"]
    return square


# generator settings and seeds for which the numpy model alone recovers the planted blocks (found by running it on the CPU:
# all of seeds 0..9 at inflation 2 and 3, tests/test_mcl_cpu.py keeps asserting four of them)
@pytest.mark.parametrize("dt,inflation,seed", [(np.float64, 2.0, 0), (np.float64, 2.0, 1), (np.float64, 2.0, 2), (np.float32, 2.0, 3),
                                               (np.float64, 3.0, 1)])
def test_markov_cluster_equals_model_on_planted_partitions(mctx, port, dt, inflation, seed):
    n, rows, cols, truth = model.planted_partition(seed)
    labels, info = graph.markov_cluster(rows, cols, n, inflation=inflation, dtype=dt, ctx=mctx, return_matrix=True)
    want_labels, want_info, (rp, ci, va) = model.markov_cluster(rows, cols, n, inflation=inflation, dtype=dt, square=_port_square(port))
    assert labels.dtype == np.int64 and np.array_equal(labels, want_labels)
    assert info["converged"] and info["iterations"] == want_info["iterations"]
    assert info["nnz_expanded"] == want_info["nnz_expanded"] and info["nnz_kept"] == want_info["nnz_kept"]
    T = info["matrix"]
    assert np.array_equal(T.indptr, rp) and np.array_equal(T.indices, ci.astype(np.int64))
    if inflation == 2.0:
        assert np.array_equal(_bits(T.data), _bits(va))
        assert info["chaos"] == want_info["chaos"]
    assert np.array_equal(labels, truth) and info["n_clusters"] == truth.max() + 1


def test_markov_cluster_weighted_and_isolated_vertices(mctx, port):
    rows = np.array([0, 1, 2, 4, 5, 6, 2], np.int64)
    cols = np.array([1, 2, 0, 5, 6, 4, 4], np.int64)
    w = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.01])
    labels, info = graph.markov_cluster(rows, cols, 8, weights=w, ctx=mctx)          # vertices 3 and 7 are isolated
    want, _, _ = model.markov_cluster(rows, cols, 8, weights=w, square=_port_square(port))
    assert np.array_equal(labels, want)
    assert labels.tolist() == [0, 0, 0, 1, 2, 2, 2, 3]


def test_markov_cluster_rmat_scale_16(mctx):
    n, r, c, _ = gen.rmat_coo(16, 16, "g500", seed=1)
    try:
        labels, info = graph.markov_cluster(torch.from_numpy(r.astype(np.int64)), torch.from_numpy(c.astype(np.int64)), n, ctx=mctx,
                                            return_matrix=True)
    finally:
        mctx.trim()      # (its second expansion alone holds 1.4 G entries)
    print({k: v for k, v in info.items() if k != "matrix"})
    assert info["converged"] and 1 <= info["iterations"] <= 100
    T = info["matrix"]
    assert np.all(np.abs(np.asarray(T.sum(1)).ravel() - 1.0) <= 1000 * np.finfo(np.float64).eps)
    # a partition of [0, n), numbered in ascending order of the clusters' smallest vertices
    assert labels.shape == (n,) and labels.min() == 0
    _, first = np.unique(labels, return_index=True)
    assert len(first) == labels.max() + 1 == info["n_clusters"] and np.all(np.diff(first) > 0)
    assert len(info["nnz_expanded"]) == len(info["nnz_kept"]) == len(info["ms_product"]) == len(info["ms_prune"]) == info["iterations"]
    for e, k in zip(info["nnz_expanded"], info["nnz_kept"]):
        assert k <= min(e, n * 1000)
