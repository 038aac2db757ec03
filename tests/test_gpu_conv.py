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
