"""The masked product C<M> = A*B (osp_spgemm_masked) and triangle_count on the GPU: bit for bit against the oracle's
unmasked product filtered by the mask, against the library's own unmasked product, on the rounding traps the kernel's
rules exist for, on skewed inputs that run both slot classes, and through the result's other entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import graph
from outerspace_amd import spgemm as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _csc(M, K, rows, cols, vals):
    A = sp.csc_matrix((vals, (rows, cols)), shape=(M, K))
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data


def _csr(K, N, rows, cols, vals):
    B = sp.csr_matrix((vals, (rows, cols)), shape=(K, N))
    B.sort_indices()
    return B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data


def _operands(M, K, N, da, db, dt, seed):
    ar, ac, av = gen.random_coo(M, K, da, seed=seed, dtype=dt)
    br, bc, bv = gen.random_coo(K, N, db, seed=seed + 1, dtype=dt)
    av = (av - dt(0.5)).astype(dt)   # signs of both kinds: sums that partly cancel
    bv = (bv - dt(0.5)).astype(dt)
    return _csc(M, K, ar, ac, av), _csr(K, N, br, bc, bv)


def _filtered(want, M, N, m_rowptr, m_colidx):
    """The oracle's product restricted to the mask: (rowptr, colidx, vals)."""
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(want["rowptr"]))
    key = rows * N + want["colidx"].astype(np.int64)
    mrows = np.repeat(np.arange(M, dtype=np.int64), np.diff(m_rowptr))
    mkey = mrows * N + m_colidx.astype(np.int64)
    keep = np.isin(key, mkey)
    rowptr = np.zeros(M + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    return rowptr, want["colidx"][keep], want["vals"][keep]


def _products(M, K, N, a, b, m_rowptr, m_colidx):
    """numpy/scipy count of products formed at the mask: sum over (i, j) of |{k : A[i,k], B[k,j] stored}|."""
    Ap = sp.csc_matrix((np.ones(len(a[1]), np.int64), a[1], a[0]), shape=(M, K)).tocsr()
    Bp = sp.csr_matrix((np.ones(len(b[1]), np.int64), b[1], b[0]), shape=(K, N))
    Mp = sp.csr_matrix((np.ones(len(m_colidx), np.int64), m_colidx, m_rowptr), shape=(M, N))
    return int((Ap @ Bp).multiply(Mp).sum())


def _random_mask(M, N, density, seed, extra=None):
    rng = np.random.default_rng(seed)
    nnz = int(round(density * M * N))
    key = np.sort(rng.choice(M * N, size=nnz, replace=False)).astype(np.int64)
    if extra is not None:
        key = np.union1d(key, extra)
    rows, cols = key // N, key % N
    rowptr = np.zeros(M + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return rowptr, cols.astype(np.uint32)


def _dev(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(DEV) if x.size else torch.empty(1, dtype=torch.from_numpy(x[:0]).dtype, device=DEV)


def _masked(ctx, M, K, N, a, b, m_rowptr, m_colidx, space="host", validate=True):
    if space == "host":
        return ctx.spgemm_masked(M, K, N, *a, *b, m_rowptr, m_colidx, validate=validate)
    ts = [_dev(x) for x in (*a, *b, m_rowptr, m_colidx)]
    torch.cuda.synchronize(DEV)
    res = ctx.spgemm_masked_device(a[2].dtype, M, K, N, [t.data_ptr() for t in ts[:6]], [t.data_ptr() for t in ts[6:]],
                                   validate=validate)
    res.to_host()
    return res


def _check(res, M, K, N, a, b, m_rowptr, m_colidx, want):
    rp, ci, va = _filtered(want, M, N, m_rowptr, m_colidx)
    assert np.array_equal(res.rowptr, rp)
    assert np.array_equal(res.colidx, ci)
    assert np.array_equal(_bits(res.vals), _bits(va))
    info = res.info
    assert info["partials"] == _products(M, K, N, a, b, m_rowptr, m_colidx)
    assert (info["M"], info["K"], info["N"], info["row_begin"], info["row_end"]) == (M, K, N, 0, M)
    assert (info["nnz_a"], info["nnz_b"], info["nnz_c"]) == (len(a[1]), len(b[1]), len(ci))
    assert info["heavy_rows"] == 0 and info["panels"] == 0 and info["rank_atomic"] == 0 and info["ms_symbolic"] == 0
    assert info["ms_total"] > 0


@pytest.fixture(scope="module")
def mctx():
    return S.default_context()


# ---- oracle parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("density", [0.0, 0.002, 0.03, 0.3, "product"])
def test_masked_equals_filtered_oracle(port, mctx, dt, space, density):
    M, K, N = 150, 90, 170
    a, b = _operands(M, K, N, 0.05, 0.06, dt, seed=11)
    want = port.spgemm(M, K, N, *a, *b)
    if density == "product":
        m_rowptr, m_colidx = want["rowptr"].astype(np.int64), want["colidx"].astype(np.uint32)
    else:
        m_rowptr, m_colidx = _random_mask(M, N, density, seed=7)
    res = _masked(mctx, M, K, N, a, b, m_rowptr, m_colidx, space)
    _check(res, M, K, N, a, b, m_rowptr, m_colidx, want)
    if density not in (0.0, "product"):   # random masks hold positions without a product: they stay absent
        assert res.nnz < len(m_colidx)
    if density == 0.0:
        assert res.nnz == 0 and not np.any(res.rowptr)
    res.close()


def test_masked_with_empty_operands(port, mctx):
    M, K, N = 20, 0, 30
    a = (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    b = (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    m_rowptr, m_colidx = _random_mask(M, N, 0.2, seed=1)
    res = mctx.spgemm_masked(M, K, N, *a, *b, m_rowptr, m_colidx)
    assert res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(M + 1, np.int64)) and res.info["partials"] == 0
    res.close()


def test_mask_of_the_product_pattern_equals_the_product(ctx):
    """Mask = the product's own pattern: the masked product IS the product, bit for bit, in every formulation."""
    n, r, c, v = gen.rmat_coo(10, 8, "g500", seed=4)
    a = _csc(n, n, r, c, v)
    b = _csr(n, n, c, r, v)   # B = A^T, the reference CLI's flow
    full = ctx.spgemm_csc_csr(n, n, n, *a, *b)
    res = ctx.spgemm_masked(n, n, n, *a, *b, full.rowptr, full.colidx)
    assert np.array_equal(res.rowptr, full.rowptr)
    assert np.array_equal(res.colidx, full.colidx)
    assert np.array_equal(_bits(res.vals), _bits(full.vals))
    assert res.info["partials"] == full.info["partials"]   # every product lands in the pattern
    full.close()
    res.close()


# ---- known traps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_lone_negative_zero_product_stays_negative_zero(port, mctx, dt):
    """0 * -1 = -0.0, the only product: a sum started at +0.0 would turn it into +0.0."""
    K = 1
    av = np.array([0.0], dt)
    bv = np.array([-1.0], dt)
    ap, ai = np.array([0, 1], np.int64), np.array([0], np.uint32)
    res = mctx.spgemm_masked(1, K, 1, ap, ai, av, ap, ai, bv, np.array([0, 1], np.int64), np.array([0], np.uint32))
    want = port.spgemm(1, K, 1, ap, ai, av, ap, ai, bv)
    assert res.nnz == 1
    assert np.signbit(res.vals[0]) and res.vals[0] == 0
    assert _bits(res.vals)[0] == _bits(want["vals"])[0]
    res.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_cancelling_sum_stays_an_explicit_zero(port, mctx, dt):
    ap, ai, av = np.array([0, 1, 2], np.int64), np.array([0, 0], np.uint32), np.array([1.0, 1.0], dt)
    bp, bi, bv = np.array([0, 1, 2], np.int64), np.array([0, 0], np.uint32), np.array([1.0, -1.0], dt)
    res = mctx.spgemm_masked(1, 2, 1, ap, ai, av, bp, bi, bv, np.array([0, 1], np.int64), np.array([0], np.uint32))
    want = port.spgemm(1, 2, 1, ap, ai, av, bp, bi, bv)
    assert res.nnz == 1 and res.vals[0] == 0 and not np.signbit(res.vals[0])
    assert _bits(res.vals)[0] == _bits(want["vals"])[0]
    assert res.info["partials"] == 2
    res.close()


def test_no_contraction_in_the_sum(port, mctx):
    """k = 0 gives -(1 + 2^-29), k = 1 gives (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60, rounded to 1 + 2^-29: the sum is exactly
    0.0.  An FMA would add the exact square and give 2^-60."""
    e29, e30 = 2.0 ** -29, 2.0 ** -30
    ap, ai, av = np.array([0, 1, 2], np.int64), np.array([0, 0], np.uint32), np.array([1.0, 1.0 + e30])
    bp, bi, bv = np.array([0, 1, 2], np.int64), np.array([0, 0], np.uint32), np.array([-(1.0 + e29), 1.0 + e30])
    res = mctx.spgemm_masked(1, 2, 1, ap, ai, av, bp, bi, bv, np.array([0, 1], np.int64), np.array([0], np.uint32))
    want = port.spgemm(1, 2, 1, ap, ai, av, bp, bi, bv)
    assert want["vals"][0] == 0.0
    assert res.nnz == 1 and res.vals[0] == 0.0
    assert _bits(res.vals)[0] == _bits(want["vals"])[0]
    res.close()


# ---- skew -------------------------------------------------------------------------------------------------------------------
def test_rmat_g500_mask_is_pattern_of_a(port, mctx):
    n, r, c, v = gen.rmat_coo(14, 16, "g500", seed=5)
    a = _csc(n, n, r, c, v)
    b = _csr(n, n, r, c, v)   # A * A
    want = port.spgemm(n, n, n, *a, *b)
    m = _csr(n, n, r, c, v)
    res = mctx.spgemm_masked(n, n, n, *a, *b, m[0], m[1])
    _check(res, n, n, n, a, b, m[0], m[1], want)
    res.close()


def _heavy_case(dt, seed):
    """Rows of A and columns of B beside a few long ones: row 0 of A and column 0 of B share ~3000 of their 6000 k (min far
    above the heavy threshold, 2048), row 1 and column 1 are long against short partners (light walks that gallop)."""
    rng = np.random.default_rng(seed)
    M, K, N = 64, 20000, 80
    ar, ac = [], []
    br, bc = [], []
    ka = np.sort(rng.choice(K, 6000, replace=False))
    kb = np.sort(np.concatenate([rng.choice(ka, 3000, replace=False), rng.choice(np.setdiff1d(np.arange(K), ka), 3000, replace=False)]))
    ar += [0] * len(ka); ac += list(ka)
    bc += [0] * len(kb); br += list(kb)
    k1 = np.sort(rng.choice(K, 9000, replace=False))   # long row 1 of A
    ar += [1] * len(k1); ac += list(k1)
    k2 = np.sort(rng.choice(K, 2500, replace=False))   # column 2 of B: 2500 > 2048 against row 0's 6000: heavy too
    bc += [2] * len(k2); br += list(k2)
    for i in range(2, M):
        ks = rng.choice(K, int(rng.integers(1, 40)), replace=False)
        ar += [i] * len(ks); ac += list(ks)
    for j in list(range(3, N)) + [1]:
        ks = rng.choice(K, int(rng.integers(1, 60)), replace=False)
        bc += [j] * len(ks); br += list(ks)
    av = (rng.random(len(ar)) - 0.5).astype(dt)
    bv = (rng.random(len(br)) - 0.5).astype(dt)
    return M, K, N, _csc(M, K, np.array(ar), np.array(ac), av), _csr(K, N, np.array(br), np.array(bc), bv)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("space", ["host", "device"])
def test_heavy_and_light_slots(port, mctx, dt, space):
    M, K, N, a, b = _heavy_case(dt, seed=3)
    want = port.spgemm(M, K, N, *a, *b)
    m_rowptr, m_colidx = _random_mask(M, N, 0.3, seed=2, extra=np.array([0, 2, 1 * N + 0, 1 * N + 1, 1 * N + 2, 5 * N + 0], np.int64))
    res = _masked(mctx, M, K, N, a, b, m_rowptr, m_colidx, space)
    _check(res, M, K, N, a, b, m_rowptr, m_colidx, want)
    assert res.info["multiply_launches"] == 2   # both slot classes ran
    res.close()


def test_hub_column_against_many_short_rows(port, mctx):
    rng = np.random.default_rng(9)
    M, K, N = 3000, 120000, 4
    hub = np.arange(0, K, 1)[: 100000]
    br = np.concatenate([hub, rng.choice(K, 50, replace=False)])
    bc = np.concatenate([np.zeros(len(hub), np.int64), np.ones(50, np.int64)])
    ar = np.repeat(np.arange(M), 5)
    ac = rng.integers(0, K, len(ar))
    key = np.unique(ar * K + ac)
    ar, ac = key // K, key % K
    a = _csc(M, K, ar, ac, rng.random(len(ar)))
    b = _csr(K, N, br, bc, rng.random(len(br)))
    want = port.spgemm(M, K, N, *a, *b)
    m_rowptr = np.arange(0, 2 * M + 1, 2, dtype=np.int64)
    m_colidx = np.tile(np.array([0, 1], np.uint32), M)
    res = mctx.spgemm_masked(M, K, N, *a, *b, m_rowptr, m_colidx)
    _check(res, M, K, N, a, b, m_rowptr, m_colidx, want)
    res.close()


def test_weight_gradient_shape_on_the_fc1_pattern(port, mctx, golden_dir):
    """(delta^T . X) restricted to a pruned layer's pattern: out x batch times batch x in, at fc1's (100 x 784) pattern."""
    nrow, ncol, wr, wc, _ = S.read_mtx(os.path.join(golden_dir, "mlp_fc1_weight.mtx"))
    m_rowptr, m_colidx, _ = gen.coo_to_csr(nrow, wr, wc, np.zeros(len(wr), np.float32))
    batch = 256
    dr, dc, dv = gen.random_coo(nrow, batch, 0.2, seed=21, dtype=np.float32)   # delta^T: out x batch
    xr, xc, xv = gen.random_coo(batch, ncol, 0.15, seed=22, dtype=np.float32)  # X: batch x in
    a = _csc(nrow, batch, dr, dc, dv - np.float32(0.5))
    b = _csr(batch, ncol, xr, xc, xv)
    want = port.spgemm(nrow, batch, ncol, *a, *b)
    res = mctx.spgemm_masked(nrow, batch, ncol, *a, *b, m_rowptr, m_colidx)
    _check(res, nrow, batch, ncol, a, b, m_rowptr, m_colidx, want)
    assert res.nnz <= len(wr)
    res.close()


# ---- triangle counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 7, 30])
def test_triangles_of_complete_graph(mctx, n):
    r, c = np.triu_indices(n, 1)
    assert graph.triangle_count(r, c, n, ctx=mctx) == math.comb(n, 3)


def test_triangles_of_a_cycle_and_of_nothing(mctx):
    n = 50
    r = np.arange(n)
    assert graph.triangle_count(r, (r + 1) % n, n, ctx=mctx) == 0
    assert graph.triangle_count(np.zeros(0, np.int64), np.zeros(0, np.int64), 5, ctx=mctx) == 0


@pytest.mark.parametrize("seed", range(4))
def test_triangles_match_dense_trace(mctx, seed):
    g = torch.Generator().manual_seed(seed)
    n = 60 + 20 * seed
    m = 6 * n
    r = torch.randint(0, n, (m,), generator=g)
    c = torch.randint(0, n, (m,), generator=g)
    c[: m // 8] = 0   # a hub vertex, duplicate edges and a self loop or two
    A = torch.zeros(n, n, dtype=torch.float64)
    A[r, c] = 1
    A[c, r] = 1
    A.fill_diagonal_(0)
    want = int(round(torch.trace(A @ A @ A).item() / 6))
    assert graph.triangle_count(r.to(DEV), c.to(DEV), n, ctx=mctx) == want


def test_triangles_rmat_match_scipy(mctx):
    n, r, c, _ = gen.rmat_coo(14, 16, "g500", seed=8)
    A = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    A = ((A + A.T) != 0).astype(np.float64)
    A.setdiag(0)
    A.eliminate_zeros()
    want = int(round((A @ A).multiply(A).sum() / 6))
    assert want > 0
    assert graph.triangle_count(torch.from_numpy(r.astype(np.int64)), torch.from_numpy(c.astype(np.int64)), n, ctx=mctx) == want


# ---- error paths ------------------------------------------------------------------------------------------------------------
def _raw_call(mctx, M, K, N, a, b, m_rowptr, m_colidx, cfg):
    arrs = [np.ascontiguousarray(x) for x in (*a, *b, m_rowptr, m_colidx)]
    ptrs = [ctypes.c_void_p(x.ctypes.data if x.size else 0) for x in arrs]
    out = ctypes.c_void_p()
    st = _lib.lib().osp_spgemm_masked(mctx._h, _lib.OSP_F64, M, K, N, *ptrs, _lib.OSP_HOST, ctypes.byref(cfg), ctypes.byref(out))
    return st, out


def _cfg(**kw):
    cfg = _lib.Config()
    _lib.lib().osp_config_default(ctypes.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


_BAD_MASKS = {
    "unsorted": (np.array([0, 2, 3], np.int64), np.array([3, 1, 0], np.uint32), _lib.ERR_UNSORTED),
    "duplicate": (np.array([0, 2, 3], np.int64), np.array([1, 1, 0], np.uint32), _lib.ERR_DUPLICATE),
    "out_of_range": (np.array([0, 2, 3], np.int64), np.array([1, 4, 0], np.uint32), _lib.ERR_RANGE),
    "non_monotone_rowptr": (np.array([0, 3, 2], np.int64), np.array([0, 1, 2], np.uint32), _lib.ERR_ARG),
}


@pytest.mark.parametrize("case", sorted(_BAD_MASKS))
def test_bad_mask_statuses(mctx, case):
    M, K, N = 2, 3, 4
    a, b = _operands(M, K, N, 0.7, 0.7, np.float64, seed=4)
    m_rowptr, m_colidx, want = _BAD_MASKS[case]
    st, out = _raw_call(mctx, M, K, N, a, b, m_rowptr, m_colidx, _cfg())
    assert st == want, (case, st, _lib.lib().osp_last_error_string())
    assert out.value is None
    with pytest.raises(S.OspError) as ei:
        mctx.spgemm_masked(M, K, N, *a, *b, m_rowptr, m_colidx)
    assert ei.value.status == want


@pytest.mark.parametrize("field", [{"k_begin": 1, "k_end": 2}, {"k_end": 2}, {"row_shard_index": 0, "row_shard_count": 2}])
def test_unsupported_config_fields(mctx, field):
    M, K, N = 2, 3, 4
    a, b = _operands(M, K, N, 0.7, 0.7, np.float64, seed=4)
    st, out = _raw_call(mctx, M, K, N, a, b, np.array([0, 1, 1], np.int64), np.array([2], np.uint32), _cfg(**field))
    assert st == _lib.ERR_ARG and out.value is None


def test_null_mask_with_entries_is_an_argument_error(mctx):
    M, K, N = 2, 3, 4
    a, b = _operands(M, K, N, 0.7, 0.7, np.float64, seed=4)
    arrs = [np.ascontiguousarray(x) for x in (*a, *b)]
    ptrs = [ctypes.c_void_p(x.ctypes.data) for x in arrs]
    m_rowptr = np.array([0, 1, 2], np.int64)
    out = ctypes.c_void_p()
    L = _lib.lib()
    st = L.osp_spgemm_masked(mctx._h, _lib.OSP_F64, M, K, N, *ptrs, ctypes.c_void_p(m_rowptr.ctypes.data), None, _lib.OSP_HOST, None,
                             ctypes.byref(out))
    assert st == _lib.ERR_ARG and out.value is None
    st = L.osp_spgemm_masked(mctx._h, _lib.OSP_F64, M, K, N, *ptrs, None, None, _lib.OSP_HOST, None, ctypes.byref(out))
    assert st == _lib.ERR_ARG and out.value is None


# ---- composition --------------------------------------------------------------------------------------------------------------
def test_masked_result_composes(port, mctx, tmp_path):
    M, K, N = 120, 70, 90
    a, b = _operands(M, K, N, 0.08, 0.08, np.float32, seed=31)
    m_rowptr, m_colidx = _random_mask(M, N, 0.2, seed=5)
    res = mctx.spgemm_masked(M, K, N, *a, *b, m_rowptr, m_colidx)
    C = res.to_scipy()
    # copy_csr into device memory
    rp = torch.empty(M + 1, dtype=torch.int64, device=DEV)
    ci = torch.empty(max(res.nnz, 1), dtype=torch.int32, device=DEV)
    va = torch.empty(max(res.nnz, 1), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    _lib.check(_lib.lib().osp_result_copy_csr(res._h, ctypes.c_void_p(rp.data_ptr()), ctypes.c_void_p(ci.data_ptr()),
                                              ctypes.c_void_p(va.data_ptr()), _lib.OSP_DEVICE))
    assert np.array_equal(rp.cpu().numpy(), res.rowptr)
    assert np.array_equal(ci[:res.nnz].cpu().numpy().view(np.uint32), res.colidx)
    assert np.array_equal(_bits(va[:res.nnz].cpu().numpy()), _bits(res.vals))
    # bias + relu
    bias = (np.random.default_rng(1).random(N) - 0.5).astype(np.float32)
    br = res.bias_relu(bias, relu=True)
    # relu(C + bias) over every column (an absent entry counts as 0), the zeros dropped
    want = sp.csr_matrix(np.maximum(C.toarray() + bias[None, :], np.float32(0)))
    got = br.to_scipy()
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(_bits(got.data.astype(np.float32)), _bits(want.data.astype(np.float32)))
    br.close()
    # write_mtx and read back
    path = tmp_path / "c.mtx"
    res.write_mtx(str(path))
    nrow, ncol, r, c, v = S.read_mtx(str(path))
    assert (nrow, ncol) == (M, N) and len(r) == res.nnz
    back = sp.csr_matrix((v.astype(np.float32), (r, c)), shape=(M, N))
    assert np.array_equal(back.indptr, C.indptr) and np.array_equal(back.indices, C.indices)
    assert np.allclose(back.data, C.data, rtol=1e-6, atol=0)
    res.close()


def test_top_level_spgemm_masked():
    """scipy in, scipy out: A @ B.T at the mask, the entries (explicit zeros included) and bits the unmasked spgemm() gives
    there."""
    A = sp.random(40, 30, density=0.2, random_state=1, format="csr")
    B = sp.random(50, 30, density=0.2, random_state=2, format="csr")
    mask = sp.random(40, 50, density=0.3, random_state=3, format="coo")
    got = S.spgemm_masked(A, B, mask)
    full = S.spgemm(A, B)
    rows = np.repeat(np.arange(40), np.diff(full.indptr))
    keep = np.isin(rows * 50 + full.indices, mask.row.astype(np.int64) * 50 + mask.col)
    rowptr = np.zeros(41, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows[keep], minlength=40))
    assert got.shape == (40, 50)
    assert np.array_equal(got.indptr, rowptr) and np.array_equal(got.indices, full.indices[keep])
    assert np.array_equal(_bits(got.data), _bits(full.data[keep]))
