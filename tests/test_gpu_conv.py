"""The conv stage of a sparse LeNet on the GPU: im2col into CSC (osp_im2col_csc), the conv product (osp_spgemm_conv2d),
max-pool of a CSR activation (osp_csr_maxpool2d) and the device-resident LeNet forward built on them, against torch."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _sparse_input(shape, seed, dt=torch.float32, density_shift=0.3):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(*shape, generator=g, dtype=dt) - density_shift)


def _torch_unfold(x, kernel_size, padding, stride, dilation):
    """get_mtx_files.py:98-133's layout: Unfold -> swapaxes(1, 2) -> reshape(-1, C*kh*kw)."""
    u = torch.nn.Unfold(kernel_size=kernel_size, dilation=dilation, padding=padding, stride=stride)(x)
    u = torch.swapaxes(u, 1, 2)
    return u.reshape(-1, u.shape[-1]).numpy()


def _im2col_raw(ctx, x, dt, kernel_size, padding, stride, dilation):
    """The library's CSC arrays as they come out (colptr, rowidx, vals), plus the nnz the count-only call reported."""
    from outerspace_amd import spgemm as S
    from outerspace_amd import sparse_util as su
    (N, C, H, W), act = su._nhwc_on_device(x, dt, DEV)
    g = S.conv2d_geometry(kernel_size, stride, padding, dilation)
    torch.cuda.synchronize(DEV)
    nnz = ctx.im2col_device(dt, N, C, H, W, act.nnz, su._dev_ptrs(act), g)
    K = C * g.kh * g.kw
    colptr = torch.full((K + 1,), -1, dtype=torch.int64, device=DEV)
    rowidx = torch.empty(max(nnz, 1), dtype=torch.int32, device=DEV)
    vals = torch.empty(max(nnz, 1), dtype=torch.float32 if dt == np.float32 else torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    nnz2 = ctx.im2col_device(dt, N, C, H, W, act.nnz, su._dev_ptrs(act), g, out_ptrs=(colptr.data_ptr(), rowidx.data_ptr(), vals.data_ptr()))
    assert nnz2 == nnz
    return colptr.cpu().numpy(), rowidx[:nnz].cpu().numpy().view(np.uint32), vals[:nnz].cpu().numpy(), nnz


_SWEEP = list(itertools.product((1, 2), (0, 2), (1, 2), (1, 3, 6)))   # stride, pad, dilation, C


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("stride,pad,dil,C", _SWEEP)
def test_im2col_csc_equals_torch_unfold(dt, stride, pad, dil, C):
    """CSC by construction: colptr, row indices (ascending in every column) and values equal torch's unfold's, exactly."""
    from outerspace_amd import spgemm as S
    ctx = S.default_context()
    tdt = torch.float32 if dt == np.float32 else torch.float64
    x = _sparse_input((1, C, 9, 11), seed=stride * 100 + pad * 10 + dil + C, dt=tdt)
    if C > 1:
        x[:, 1] = 0   # an all-zero channel
    want = sp.csc_matrix(_torch_unfold(x, 3, pad, stride, dil))
    colptr, rowidx, vals, nnz = _im2col_raw(ctx, x, dt, 3, pad, stride, dil)
    assert nnz == want.nnz
    assert np.array_equal(colptr, want.indptr)
    assert np.array_equal(rowidx, want.indices)
    assert np.array_equal(vals, want.data)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["zero", "lenet1", "lenet2", "rect"])
def test_unfold_special_cases(dt, case):
    """An all-zero input, LeNet's two geometries (batch 16: several chunks per column) and a non-square kernel, through the
    public unfold() (scipy CSR in get_LeNet's layout)."""
    from outerspace_amd import sparse_util as su
    tdt = torch.float32 if dt == np.float32 else torch.float64
    if case == "zero":
        x, kw = torch.zeros(2, 3, 7, 5, dtype=tdt), dict(kernel_size=3, padding=1)
    elif case == "lenet1":
        x, kw = _sparse_input((16, 1, 28, 28), 5, tdt), dict(kernel_size=5, padding=2)
    elif case == "lenet2":
        x, kw = _sparse_input((16, 6, 14, 14), 6, tdt), dict(kernel_size=5, padding=0)
    else:
        x, kw = _sparse_input((3, 2, 13, 8), 7, tdt), dict(kernel_size=(2, 3), padding=(1, 0), stride=(2, 1), dilation=(3, 1))
    got = su.unfold(x, dtype=dt, **kw)
    ref = _torch_unfold(x, kw["kernel_size"], kw.get("padding", 0), kw.get("stride", 1), kw.get("dilation", 1))
    want = sp.csr_matrix(ref)
    assert got.shape == ref.shape
    assert got.nnz == want.nnz
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, want.data)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_conv2d_product_equals_oracle_on_the_unfold(ctx, port, dt):
    """osp_spgemm_conv2d is bit-identical to the oracle's product of torch's unfold matrix and W^T, in every formulation."""
    from outerspace_amd import spgemm as S
    from outerspace_amd import sparse_util as su
    tdt = torch.float32 if dt == np.float32 else torch.float64
    N, C, H, W, OC, k = 2, 3, 9, 11, 5, 3
    x = _sparse_input((N, C, H, W), 11, tdt)
    w = su.prune_by_magnitude(torch.randn(OC, C * k * k, generator=torch.Generator().manual_seed(12), dtype=tdt), 0.5)
    A = sp.coo_matrix(_torch_unfold(x, k, 1, 1, 1))
    Wc = sp.coo_matrix(w.numpy())
    K = C * k * k
    acsc = S.coo_to_csc(K, A.row, A.col, A.data.astype(dt))
    bcsr = S.coo_to_csr(K, Wc.col, Wc.row, Wc.data.astype(dt))   # B = W^T
    want = port.spgemm(A.shape[0], K, OC, *acsc, *bcsr)
    (_, _, _, _), act = su._nhwc_on_device(x, dt, DEV)
    wr = torch.from_numpy(Wc.row.astype(np.int32)).to(DEV)
    wc = torch.from_numpy(Wc.col.astype(np.int32)).to(DEV)
    wv = torch.from_numpy(Wc.data.astype(dt)).to(DEV)
    torch.cuda.synchronize(DEV)
    got = ctx.spgemm_conv2d_device(dt, N, C, H, W, act.nnz, su._dev_ptrs(act), OC, wv.numel(),
                                   (wr.data_ptr(), wc.data_ptr(), wv.data_ptr()), S.conv2d_geometry(k, 1, 1))
    assert got.shape == (N * H * W, OC)
    assert got.info["partials"] == want["partials"]
    assert np.array_equal(got.rowptr, want["rowptr"])
    assert np.array_equal(got.colidx, want["colidx"])
    assert np.array_equal(got.vals, want["vals"])
    got.close()


@pytest.mark.parametrize("stride,padding,relu", [(1, 0, False), (1, 2, True), (2, 1, True)])
def test_sparse_conv2d_matches_torch_f64(stride, padding, relu):
    """Against F.conv2d on the CPU in f64: another summation order, so within 1e-6 relative, not bit for bit."""
    from outerspace_amd import sparse_util as su
    N, C, H, W, OC, k = 3, 4, 12, 10, 7, 3
    x = _sparse_input((N, C, H, W), 21, torch.float64)
    w = su.prune_by_magnitude(torch.randn(OC, C, k, k, generator=torch.Generator().manual_seed(22), dtype=torch.float64), 0.4)
    b = torch.randn(OC, generator=torch.Generator().manual_seed(23), dtype=torch.float64) * 0.1
    ref = F.conv2d(x, w, b, stride=stride, padding=padding)
    if relu:
        ref = torch.relu(ref)
    got = su.sparse_conv2d(x, w, b, stride=stride, padding=padding, relu=relu, dtype=np.float64)
    OH, OW = ref.shape[2], ref.shape[3]
    assert got.shape == (N * OH * OW, OC)
    assert np.allclose(su.to_nchw(got, N, OC, OH, OW).numpy(), ref.numpy(), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("kernel,stride", [(2, None), (3, 2), ((2, 3), (1, 2))])
def test_sparse_max_pool2d_matches_torch(dt, signed, kernel, stride):
    """Exact: the max over the window of the densified input (an absent entry is a 0 there), zeros dropped."""
    from outerspace_amd import sparse_util as su
    tdt = torch.float32 if dt == np.float32 else torch.float64
    N, C, H, W = 2, 70, 9, 11   # > 64 channels: two wave steps per output row
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N, C, H, W, generator=g, dtype=tdt)
    if signed:
        x = torch.where(torch.rand(N, C, H, W, generator=g) < 0.3, torch.zeros((), dtype=tdt), x)
        x[0, :, :4, :4] = -x[0, :, :4, :4].abs() - 0.5   # windows of only negative entries
    else:
        x = torch.relu(x - 0.5)
    ref = F.max_pool2d(x, kernel, stride)
    got = su.sparse_max_pool2d(x, kernel, stride, dtype=dt)
    PH, PW = ref.shape[2], ref.shape[3]
    assert got.shape == (N * PH * PW, C)
    want = sp.csr_matrix(ref.permute(0, 2, 3, 1).reshape(-1, C).numpy())
    assert got.nnz == want.nnz
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, want.data)


def _lenet_params(seed, dt=torch.float32):
    from outerspace_amd import sparse_util as su
    g = torch.Generator().manual_seed(seed)
    shapes = {"conv1_weight": (6, 1, 5, 5), "conv1_bias": (6,), "conv2_weight": (16, 6, 5, 5), "conv2_bias": (16,),
              "fc1_weight": (120, 400), "fc1_bias": (120,), "fc2_weight": (84, 120), "fc2_bias": (84,),
              "fc3_weight": (10, 84), "fc3_bias": (10,)}
    p = {}
    for name, shp in shapes.items():
        t = torch.randn(*shp, generator=g, dtype=dt)
        if name.endswith("weight"):
            fan_in = int(np.prod(shp[1:]))
            p[name] = su.prune_by_magnitude(t / fan_in ** 0.5, 0.3)
        else:
            p[name] = t * 0.1
    return p


def _dense_lenet(x, p):
    """The dense LeNet forward (conv 5x5 pad 2 -> ReLU -> pool 2 -> conv 5x5 -> ReLU -> pool 2 -> fc 400-120-84-10)."""
    xc1 = torch.relu(F.conv2d(x, p["conv1_weight"], p["conv1_bias"], padding=2))
    xcp1 = F.max_pool2d(xc1, 2)
    xc2 = torch.relu(F.conv2d(xcp1, p["conv2_weight"], p["conv2_bias"]))
    xcp2 = F.max_pool2d(xc2, 2)
    xf0 = xcp2.view(-1, 16 * 5 * 5)
    xf1 = torch.relu(F.linear(xf0, p["fc1_weight"], p["fc1_bias"]))
    xf2 = torch.relu(F.linear(xf1, p["fc2_weight"], p["fc2_bias"]))
    return F.linear(xf2, p["fc3_weight"], p["fc3_bias"]), (xc1, xcp1, xc2, xcp2, xf0, xf1, xf2)


def _check_lenet(got, want, N, tol):
    from outerspace_amd import sparse_util as su
    logits, acts = got
    ref_logits, ref_acts = want
    assert np.allclose(logits.toarray(), ref_logits.numpy(), rtol=tol, atol=tol)
    for i, (a, r) in enumerate(zip(acts, ref_acts)):
        if r.dim() == 4:
            assert a.shape == (N * r.shape[2] * r.shape[3], r.shape[1]), i
            a = su.to_nchw(a, N, r.shape[1], r.shape[2], r.shape[3])
        else:
            assert a.shape == tuple(r.shape), i
            a = torch.from_numpy(a.toarray())
        assert np.allclose(a.numpy(), r.numpy(), rtol=tol, atol=tol), i


def test_lenet_forward_batch64_f32(tmp_path):
    """Every activation and the logits within 1e-5 of the dense forward; the same through get_LeNet's .mtx files (1e-4:
    the values went through 8-digit text)."""
    from outerspace_amd import sparse_util as su
    N = 64
    x = _sparse_input((N, 1, 28, 28), 41, density_shift=0.8)
    p = _lenet_params(42)
    want = _dense_lenet(x, p)
    _check_lenet(su.lenet_forward(x, p), want, N, 1e-5)
    # state_dict names are accepted too
    logits2, _ = su.lenet_forward(x, {k.replace("_", ".", 1): v for k, v in p.items()})
    assert np.allclose(logits2.toarray(), want[0].numpy(), rtol=1e-5, atol=1e-5)
    d = tmp_path / "lenet"
    d.mkdir()
    su.save_tensor_as_mtx(torch.from_numpy(_torch_unfold(x, 5, 2, 1, 1)), str(d / "act_0.mtx"))
    for name, t in p.items():
        t = t.reshape(t.shape[0], -1) if "conv" in name and "weight" in name else t
        su.save_tensor_as_mtx(t.reshape(1, -1) if t.dim() == 1 else t, str(d / f"{name}.mtx"))
    _check_lenet(su.lenet_forward_from_mtx(str(d)), want, N, 1e-4)


def test_lenet_forward_batch1024():
    """One batch-1024 forward completes; conv1's im2col has the nnz the host counts on the input's unfold."""
    from outerspace_amd import spgemm as S
    from outerspace_amd import sparse_util as su
    N = 1024
    x = _sparse_input((N, 1, 28, 28), 51, density_shift=0.8)
    p = _lenet_params(52)
    ctx = S.default_context()
    (_, C, H, W), act = su._nhwc_on_device(x, np.float32, DEV)
    torch.cuda.synchronize(DEV)
    nnz_a = ctx.im2col_device(np.float32, N, C, H, W, act.nnz, su._dev_ptrs(act), S.conv2d_geometry(5, 1, 2))
    assert nnz_a == int(np.count_nonzero(_torch_unfold(x, 5, 2, 1, 1)))
    logits, acts = su.lenet_forward(x, p)
    assert logits.shape == (N, 10) and acts[0].shape == (N * 28 * 28, 6)
    ref_logits, _ = _dense_lenet(x, p)
    assert np.allclose(logits.toarray(), ref_logits.numpy(), rtol=1e-4, atol=1e-4)


def test_conv_error_paths():
    from outerspace_amd import _lib
    from outerspace_amd import spgemm as S
    from outerspace_amd import sparse_util as su
    ctx = S.default_context()
    x = _sparse_input((2, 3, 6, 6), 61)
    (N, C, H, W), act = su._nhwc_on_device(x, np.float32, DEV)
    torch.cuda.synchronize(DEV)
    ptrs = su._dev_ptrs(act)
    bad = [S.conv2d_geometry(0), S.conv2d_geometry(3, stride=0), S.conv2d_geometry(3, dilation=0), S.conv2d_geometry(7),
           S.conv2d_geometry(3, dilation=4)]
    g = S.conv2d_geometry(3)
    g.reserved[2] = 1
    bad.append(g)
    for geom in bad:
        with pytest.raises(S.OspError) as ei:
            ctx.im2col_device(np.float32, N, C, H, W, act.nnz, ptrs, geom)
        assert ei.value.status == _lib.ERR_ARG
    with pytest.raises(S.OspError) as ei:   # a zero size
        ctx.im2col_device(np.float32, N, 0, H, W, act.nnz, ptrs, S.conv2d_geometry(3))
    assert ei.value.status == _lib.ERR_ARG
    with pytest.raises(S.OspError) as ei:   # the input has channels 0..2: C = 2 puts an index outside its dimension
        ctx.im2col_device(np.float32, N, 2, H, W, act.nnz, ptrs, S.conv2d_geometry(3), validate=True)
    assert ei.value.status == _lib.ERR_RANGE
    with pytest.raises(S.OspError) as ei:   # pixels beyond N*H*W
        ctx.im2col_device(np.float32, 1, C, H, W, act.nnz, ptrs, S.conv2d_geometry(3), validate=True)
    assert ei.value.status == _lib.ERR_RANGE
    with pytest.raises(S.OspError) as ei:   # N*OH*OW beyond u32
        ctx.im2col_device(np.float32, 1 << 20, C, 1 << 12, 1 << 12, act.nnz, ptrs, S.conv2d_geometry(1))
    assert ei.value.status == _lib.ERR_RANGE
    # max-pool: the window larger than the input, and an N*H*W that is not the input's row count
    res = ctx.merge_csr_parts(4, 2, [(np.array([0, 1, 1, 2, 2], np.int64), np.array([0, 1], np.uint32), np.ones(2, np.float32))])
    for args in ((1, 2, 2, 3), (2, 2, 2, 2)):
        with pytest.raises(S.OspError) as ei:
            res.maxpool2d(*args)
        assert ei.value.status == _lib.ERR_ARG
    out = res.maxpool2d(1, 2, 2, 2)
    assert out.shape == (1, 2) and np.array_equal(out.to_scipy().toarray(), [[1, 1]])
    out.close()
    res.close()
    # the context still works after the failures
    assert ctx.im2col_device(np.float32, N, C, H, W, act.nnz, ptrs, S.conv2d_geometry(3)) > 0


# ==== the conv stage against tests/conv_model.py, in bits ================================================================================
# Operands carry tests/test_gpu_apply_mask.py's special values at every seventh entry; every output value is a copy, so values
# are compared with ieee_model.assert_same_bits AND as whole bit patterns (a copied NaN keeps its payload).  The inputs are
# tests/conv_cases.py's, which tests/test_conv_model_cpu.py runs against the model with planted defects.
import os
import subprocess
import sys

from outerspace_amd import _lib
from outerspace_amd import spgemm as S
from tests import conv_cases as cc
from tests import conv_model as model
from tests.ieee_model import assert_same_bits
from tests.result_chain import Frame
from tests.test_gpu_parity import assert_same

DTYPES = [np.float32, np.float64]
CHILD_TIMEOUT_S = 120   # a hang guard: a child starts Python, loads the library, creates a context and makes 16 small calls


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _same_copies(got, want):
    assert_same_bits(got, want)
    assert np.array_equal(_bits(got), _bits(want))   # copies: a NaN keeps its sign and payload too


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


# ---- im2col: chunk and wave edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_im2col_chunk_and_wave_edges(mctx, dt):
    """Channels of exactly 0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097 and 0 entries, the COO shuffled."""
    assert model.CHUNK == 2048 and model.WAVE == 64   # a change of kConvChunk fails here, not silently
    assert cc.EDGE_COUNTS == [0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 0] and cc.EDGE_SHAPE == (2, 11, 33, 63)
    N, C, H, W = cc.EDGE_SHAPE
    x = cc.edge_input(dt)
    assert np.bincount(x[1], minlength=C).tolist() == cc.EDGE_COUNTS and np.any(np.diff(x[1].astype(np.int64)) < 0)
    for g in cc.EDGE_GEOMS:
        want = model.im2col(N, C, H, W, x, g)
        colptr, rows, vals, nnz = cc.im2col(mctx, dt, cc.EDGE_SHAPE, x, g)
        assert nnz == len(want[1]) == colptr[-1]       # the count-only call reports the same nnz
        assert np.array_equal(colptr, want[0])
        assert np.array_equal(rows, want[1])
        _same_copies(vals, want[2])


# ---- im2col: caller-owned outputs ------------------------------------------------------------------------------------------------------------
def _framed(fr):
    """(the frame's buffer on the device as bits, the device address of the output inside it)."""
    host = fr.new()
    bits = torch.from_numpy(host.view(np.int32 if host.dtype.itemsize == 4 else np.int64)).to(DEV)
    return bits, bits.data_ptr() + fr.pad * host.dtype.itemsize


def _unframed(name, fr, bits):
    """The output as a host array, the margins checked (result_chain.MarginDamaged) and no element left as the sentinel."""
    b = bits.cpu().numpy().view(fr.sentinel.dtype)
    fr.check(name, b)
    inside = b[fr.pad:fr.pad + fr.n]
    assert not np.any(inside == fr.sentinel), f"{name}: {int(np.sum(inside == fr.sentinel))} elements were never written"
    return fr.interior(b).copy()


@pytest.mark.parametrize("dt", DTYPES)
def test_im2col_writes_exactly_its_outputs(mctx, dt):
    N, C, H, W = cc.EDGE_SHAPE
    x = cc.edge_input(dt)
    ts = cc.upload_coo(x)
    for g in cc.EDGE_GEOMS:
        want = model.im2col(N, C, H, W, x, g)
        frames = {"a_colptr": Frame((len(want[0]),), np.int64), "a_rowidx": Frame((len(want[1]),), np.uint32), "a_vals": Frame((len(want[2]),), dt)}
        dev = {name: _framed(fr) for name, fr in frames.items()}
        torch.cuda.synchronize(DEV)
        nnz = mctx.im2col_device(dt, N, C, H, W, len(x[0]), cc.ptrs(ts), cc.lib_geom(g), out_ptrs=tuple(dev[k][1] for k in ("a_colptr", "a_rowidx", "a_vals")))
        got = {name: _unframed(name, fr, dev[name][0]) for name, fr in frames.items()}
        assert nnz == len(want[1])
        assert np.array_equal(got["a_colptr"], want[0]) and np.array_equal(got["a_rowidx"], want[1])
        _same_copies(got["a_vals"], want[2])


# ---- im2col: index space ---------------------------------------------------------------------------------------------------------------------
def _coo(pix, ch, dt, seed):
    return np.array(pix, np.uint32), np.array(ch, np.uint32), cc.values(len(pix), dt, seed)


@pytest.mark.parametrize("dt", DTYPES)
def test_im2col_at_the_limits_of_the_index_space(mctx, dt):
    g = model.geom(1)
    # pixels at 0, on both sides of bit 31 and the last one, in two channels
    H, W = 65535, 65536
    last = H * W - 1
    x = _coo([last, 1 << 31, 0, (1 << 31) - 1, (1 << 31) + 1, last], [0, 0, 0, 1, 1, 1], dt, 3)
    want = model.im2col(1, 2, H, W, x, g)
    assert want[0].tolist() == [0, 3, 6] and want[1].tolist() == [0, 1 << 31, last, (1 << 31) - 1, (1 << 31) + 1, last]
    colptr, rows, vals, nnz = cc.im2col(mctx, dt, (1, 2, H, W), x, g)
    assert nnz == 6 and np.array_equal(colptr, want[0]) and np.array_equal(rows, want[1])
    _same_copies(vals, want[2])
    # the widest row that is accepted: its last pixel maps to row 2^32 - 3
    W = (1 << 32) - 2
    x = _coo([W - 1, 0, 1 << 31], [0, 0, 0], dt, 4)
    want = model.im2col(1, 1, 1, W, x, g)
    colptr, rows, vals, nnz = cc.im2col(mctx, dt, (1, 1, 1, W), x, g)
    assert nnz == 3 and colptr.tolist() == [0, 3] and rows.tolist() == [0, 1 << 31, (1 << 32) - 3] == want[1].tolist()
    _same_copies(vals, want[2])


def test_im2col_refusals_at_the_limits(mctx):
    dt = np.float32
    ok = _coo([0, 5, 2], [0, 0, 1], dt, 5)
    ts = cc.upload_coo(ok)

    def works():
        colptr, rows, vals, nnz = cc.im2col(mctx, dt, (1, 2, 2, 3), ok, model.geom(1))
        assert nnz == 3 and colptr.tolist() == [0, 2, 3] and rows.tolist() == [0, 5, 2]
        _same_copies(vals, ok[2][[0, 1, 2]][np.lexsort((ok[0], ok[1]))])

    works()
    refused = [((1, 2, 1, (1 << 32) - 1), model.geom(1), _lib.ERR_RANGE),                 # W = 2^32 - 1
               ((1, 2, 1, (1 << 32) - 3), model.geom(1, 1, (0, 1)), _lib.ERR_RANGE)]      # N*OH*OW = 2^32 - 1 exactly
    g = refused[1][1]
    assert model.output_size((1 << 32) - 3, g.kw, g.sw, g.pw, g.dw) == (1 << 32) - 1 and model.output_size(1, g.kh, g.sh, g.ph, g.dh) == 1
    for (N, C, H, W), g, status in refused:
        with pytest.raises(S.OspError) as ei:
            mctx.im2col_device(dt, N, C, H, W, 3, cc.ptrs(ts), cc.lib_geom(g))
        assert ei.value.status == status
        works()                                                                           # the context still works
    dup = _coo([0, 5, 2, 5], [0, 0, 1, 0], dt, 6)
    td = cc.upload_coo(dup)
    with pytest.raises(S.OspError) as ei:
        mctx.im2col_device(dt, 1, 2, 2, 3, 4, cc.ptrs(td), cc.lib_geom(model.geom(1)))
    assert ei.value.status == _lib.ERR_DUPLICATE
    with pytest.raises(ValueError):
        model.im2col(1, 2, 2, 3, dup, model.geom(1))
    works()


# ---- conv2d: parity with the COO product -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geometry", list(cc.CONV_GEOMS))
def test_conv2d_equals_the_coo_product_of_the_models_unfold(ctx, dt, geometry):
    """osp_spgemm_conv2d against osp_spgemm_coo on the model's unfold matrix and W, in the four formulations."""
    g = cc.CONV_GEOMS[geometry]
    N, C, H, W = cc.CONV_SHAPE
    K = C * g.kh * g.kw
    M = N * model.output_size(H, g.kh, g.sh, g.ph, g.dh) * model.output_size(W, g.kw, g.sw, g.pw, g.dw)
    for OC in cc.CONV_OC:
        x, w = cc.conv_input(dt, g, OC)
        assert np.isnan(x[2]).any() and np.isnan(w[2]).any() and np.any(np.diff(w[1].astype(np.int64)) < 0)
        colptr, rows, vals = model.im2col(N, C, H, W, x, g)
        a = (rows, np.repeat(np.arange(K, dtype=np.uint32), np.diff(colptr)), vals)
        ref = ctx.spgemm_coo(M, K, OC, a, (w[1], w[0], w[2]))                           # B = W^T
        got = cc.conv2d(ctx, dt, cc.CONV_SHAPE, x, OC, w, g)
        try:
            assert got.shape == ref.shape == (M, OC) and got.nnz == ref.nnz > 0
            assert_same(got, {"partials": ref.info["partials"], "rowptr": ref.rowptr, "colidx": ref.colidx, "vals": ref.vals})
        finally:
            got.close()
            ref.close()


# ---- max-pool ------------------------------------------------------------------------------------------------------------------------------------
def _pool(mctx, csr, C, N, H, W, kernel, stride, a=None):
    """Pools the uploaded ``a`` (or uploads csr) and compares with the model: structure exact, values as bits, info."""
    want = model.maxpool(csr, C, N, H, W, kernel, stride)
    own = a is None
    a = cc.build(mctx, csr, C) if own else a
    try:
        out = a.maxpool2d(N, H, W, kernel, stride)
        try:
            assert out.dtype == csr[2].dtype.type and out.shape == (len(want[0]) - 1, C)
            assert np.array_equal(out.rowptr, want[0]) and np.array_equal(out.colidx, want[1])
            _same_copies(out.vals, want[2])
            info = out.info
            assert (info["M"], info["N"], info["row_begin"], info["row_end"], info["nnz_c"]) == (len(want[0]) - 1, C, 0, len(want[0]) - 1, len(want[1]))
            assert out.nnz == len(want[1])
        finally:
            out.close()
    finally:
        if own:
            a.close()
    return want


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", cc.POOL_CHANNELS)
def test_maxpool_over_channel_counts_and_geometries(mctx, dt, C):
    assert cc.POOL_CHANNELS == (1, 63, 64, 65, 128, 129)
    N, H, W = cc.POOL_SHAPE
    csr = cc.pool_input(dt, C)
    assert np.isnan(csr[2]).any() and np.any(_bits(csr[2]) == 0) and np.any((csr[2] == 0) & np.signbit(csr[2]))
    a = cc.build(mctx, csr, C)
    try:
        assert np.array_equal(a.rowptr, csr[0]) and np.array_equal(a.colidx, csr[1]) and np.array_equal(_bits(a.vals), _bits(csr[2]))
        for kernel, stride in cc.POOL_GEOMS:
            want = _pool(mctx, csr, C, N, H, W, kernel, stride, a)
            if (kernel, stride) == (2, None):   # all-negative full windows keep a negative maximum; one absent tap: dropped
                lens = np.diff(want[0]).reshape(N, H // 2, W // 2)
                assert lens[0, 0, 0] == lens[0, 1, 1] == C and lens[0, 2, 0] == lens[0, 3, 1] == 0
                assert (want[2][:C] < 0).all()
    finally:
        a.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kh,kw", cc.NAN_WINDOWS)
def test_maxpool_nan_at_every_tap_position(mctx, dt, kh, kw):
    """A NaN at each tap of the window in turn gives that NaN's bits; of two NaNs the first in tap order."""
    csr, N = cc.nan_position_input(dt, kh, kw)
    want = _pool(mctx, csr, 3, N, kh, kw, (kh, kw), None)
    nan_a, nan_b = (int(b) for b in _bits(cc.special(dt)[:2]))
    bits = _bits(want[2]).reshape(N, 3)
    T = kh * kw
    assert [int(b) for b in bits[:T, 0]] == [nan_a] * T and [int(b) for b in bits[T:, 1]] == [nan_b] * T
    assert [int(b) for b in bits[T:, 0]] == [nan_a] * (T - 1) + [nan_b]


@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_of_empty_inputs_and_of_many_channels(mctx, dt):
    empty = (np.zeros(2 * 4 * 6 + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))
    _pool(mctx, empty, 5, 2, 4, 6, 2, None)
    # a result of zero columns, from extract with an empty column list
    a = cc.build(mctx, cc.pool_input(dt, 5), 5)
    try:
        none, _ = a.extract(None, np.zeros(0, np.uint32), space="host")
        try:
            N, H, W = cc.POOL_SHAPE
            assert none.shape == (N * H * W, 0)
            _pool(mctx, (np.zeros(N * H * W + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt)), 0, N, H, W, 2, None, none)
        finally:
            none.close()
    finally:
        a.close()
    # C = 2^20 + 1 on a 2x2 image pooled to one row: the channels at both ends and around a wave step
    C = (1 << 20) + 1
    chans = np.array([0, 63, 64, (1 << 20) - 1, 1 << 20], np.uint32)
    rows = [chans, chans[[0, 2, 4]], chans[[1, 3]], chans[[0, 4]]]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    csr = (rowptr, np.concatenate(rows), cc.values(int(rowptr[-1]), dt, 8))
    want = _pool(mctx, csr, C, 1, 2, 2, 2, None)
    assert len(want[0]) == 2 and 0 < len(want[1]) <= 5


# ---- coo_rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_coo_rows_into_a_frame(mctx, dt):
    for lengths in (cc.ROWS_LENGTHS, [0] * 7):
        csr, ncol = cc.rows_input(dt, lengths)
        a = cc.build(mctx, csr, ncol)
        try:
            want = model.coo_rows(csr[0])
            assert np.array_equal(cc.coo_rows(a), want)
            fr = Frame((len(want),), np.uint32)
            bits, addr = _framed(fr)
            torch.cuda.synchronize(DEV)
            a.coo_rows_into(addr)
            assert np.array_equal(_unframed("rows", fr, bits), want)
        finally:
            a.close()
    assert sorted(set(cc.ROWS_LENGTHS)) == [0, 1, 3, 65, 129]


# ---- the pool ---------------------------------------------------------------------------------------------------------------------------------------
_state = {"digest": None, "stop": None}


def test_the_slice_in_this_process(mctx):
    _state["digest"] = cc.slice_digest(mctx)
    assert _state["digest"][1] == len(DTYPES) * (2 * len(cc.EDGE_GEOMS) + 1 + len(cc.NAN_WINDOWS) + 1)


def _child(mode):
    if _state["stop"]:
        pytest.skip(f"{_state['stop']}: nothing further is started on the GPU")
    assert _state["digest"] is not None, "the in-process run did not finish: no digest to compare with"
    env = dict(os.environ)
    env[mode] = "1"
    try:
        r = subprocess.run([sys.executable, "-m", "tests.conv_cases"], cwd=cc.ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _state["stop"] = f"the child under {mode} hung"
        raise
    if r.returncode != 0:
        _state["stop"] = f"the child under {mode} ended with status {r.returncode}"
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("CONV_SLICE ")]
    assert line == [f"CONV_SLICE {_state['digest'][0]} calls={_state['digest'][1]}"], r.stdout[-2000:]
    return r


def test_the_slice_in_a_child_under_poison():
    _child("OSP_POISON")


def test_the_slice_in_a_child_under_guard():
    r = _child("OSP_GUARD")
    assert "[osp] OSP_GUARD:" not in r.stderr, r.stderr[-4000:]
