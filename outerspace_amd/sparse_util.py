"""NN-side glue: the reference's pruning helpers and `.mtx` hand-off, plus the GPU sparse layers they feed.

Mirrors, name for name, what a user of the reference imports today (all paths under
``/root/reference/NN_models``):

* ``get_sparsity`` / ``get_prune_threshold`` / ``get_sparse_mask`` / ``prune_to_sparsity``
  -- ``sparse_util.py:5-22`` (including the SIGNED mask ``mat > threshold`` of ``:12-15``, which drops every
  negative weight; ``main.py:208-211`` prunes with ``|w| > threshold`` instead -- ``prune_by_magnitude``).
  ``print_parameters_sparsity`` (``:24-30``) is training-side logging and is not mirrored.
* ``save_tensor_as_mtx`` -- ``util.py:61-62`` (``scipy.io.mmwrite`` of the CSR form; byte-identical files).
* ``sparse_linear`` / ``mlp_forward`` / ``mlp_forward_from_mtx`` -- the products the reference hands to its
  simulator one at a time (``get_mtx_files.py:76-96``: ``./simulator act_i.mtx fc{i+1}_weight.mtx`` computes
  ``act_i @ W.T``), here executed by the MI355X SpGEMM and chained with bias + ReLU like ``models.py:17-31``.
* ``weight_chain`` -- the sparse ``W_n ... W_2 W_1`` product of BASELINE.json's configs[4].
* ``unfold`` / ``sparse_conv2d`` / ``sparse_max_pool2d`` / ``lenet_forward`` / ``lenet_forward_from_mtx`` -- the LeNet
  side (``models.py:35-84``): every conv layer is the product ``get_mtx_files.py:98-133`` dumps (the im2col-ed input
  times the ``OC x C*kh*kw`` weight, transposed), here with im2col, bias + ReLU and max-pool on the GPU as well.
  Conv-stage activations are "pixel x channel" CSR matrices, ``(N*H*W) x C`` (NHWC); ``to_nchw`` densifies one.

The helpers are plain torch / scipy plumbing (as in the reference); every matrix product goes through
``outerspace_amd.spgemm`` on the GPU.
"""
import os

import numpy as np
import scipy.io
import scipy.sparse as sp
import torch

from . import spgemm as _S


# ---- the pruning helpers of sparse_util.py:5-22, same names and results (pinned to captured values) -------------------
def get_sparsity(mat):
    """(non-zero count, element count, density) -- the triple ``sparse_util.py:5-7`` returns (count and density as tensors)."""
    nonzero = torch.count_nonzero(mat.abs() > 0)
    total = mat.numel()
    return nonzero, total, nonzero / total


def get_prune_threshold(mat, sparsity_level):
    """The |w| value below which all but a ``sparsity_level`` fraction of the entries lie (``sparse_util.py:9-10``)."""
    return torch.quantile(mat.abs(), 1 - sparsity_level)


def get_sparse_mask(mat, sparsity_level):
    """SIGNED comparison, as ``sparse_util.py:12-15`` does it: negative weights never pass."""
    return mat > get_prune_threshold(mat, sparsity_level)


def prune_to_sparsity(mat, sparsity_level):
    """``sparse_util.py:17-22``: a matrix already at or below the level is returned as it is."""
    _, _, density = get_sparsity(mat)
    return mat if density <= sparsity_level else mat * get_sparse_mask(mat, sparsity_level)


def prune_by_magnitude(mat, sparsity_level):
    """What ``main.py:208-211`` does per layer: keep ``|w| > quantile(|w|, 1 - s)``."""
    return mat * (mat.abs() > get_prune_threshold(mat, sparsity_level))


# ---- util.py:61-62 ------------------------------------------------------------------------------------
def save_tensor_as_mtx(a, save_file):
    scipy.io.mmwrite(save_file, sp.csr_matrix(a.numpy()))


# ---- the products -------------------------------------------------------------------------------------
def _coo_on_device(x, dtype, device):
    """dense tensor / ndarray / scipy sparse -> (nrow, ncol, rows i32, cols i32, vals) torch tensors on the GPU (the file
    order scipy's CSR gives, which is what ``save_tensor_as_mtx`` would have written)."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    if not sp.issparse(x):
        x = sp.csr_matrix(np.asarray(x))
    x = x.tocoo()
    tdt = _S._torch_dtype(dtype)
    return (x.shape[0], x.shape[1], torch.from_numpy(x.row.astype(np.int32)).to(device), torch.from_numpy(x.col.astype(np.int32)).to(device),
            torch.from_numpy(x.data.astype(dtype)).to(device, tdt))


class _DeviceLayerInput:
    """An activation as the next product's A operand, resident on the GPU: COO arrays that either came from the host
    once (the network's input) or ARE the previous layer's result (its colidx / vals arrays plus a row array)."""

    def __init__(self, shape, rows, cols, vals, nnz, keep=()):
        self.shape, self.rows, self.cols, self.vals, self.nnz, self.keep = shape, rows, cols, vals, nnz, keep


def _layer_on_device(ctx, act, weight_coo, bias, relu, dtype, device):
    """relu(act @ W.T + bias) with everything on the GPU: osp_spgemm_coo on device arrays (COO -> CSC / CSR there), then
    osp_csr_bias_relu on the product.  Returns the CsrResult of the layer's output."""
    M, K = act.shape
    out_n, in_n, wr, wc, wv = weight_coo   # W is out x in; B = W^T: rows = in index, cols = out index
    if in_n != K:
        raise _S.OspError(1, f"inner dimensions differ: activation is {M}x{K}, weight is {out_n}x{in_n}")
    torch.cuda.synchronize(device)   # the library works on its own stream
    prod = ctx.spgemm_coo_device(dtype, M, K, out_n, act.nnz, (act.rows.data_ptr() if act.nnz else 0, act.cols.data_ptr() if act.nnz else 0,
                                                              act.vals.data_ptr() if act.nnz else 0),
                                 wv.numel(), (wc.data_ptr() if wv.numel() else 0, wr.data_ptr() if wv.numel() else 0,
                                              wv.data_ptr() if wv.numel() else 0))
    if bias is None and not relu:
        return prod
    b = None
    if bias is not None:
        b = bias.detach().cpu().numpy() if hasattr(bias, "detach") else np.asarray(bias)
        b = b.reshape(-1).astype(dtype)
    out = prod.bias_relu(b, relu)
    prod.close()
    return out


def _result_as_input(res, device):
    """The previous layer's CSR result as the next product's COO operand, without leaving the GPU: its column / value
    arrays are borrowed, the row array is written by the library (osp_result_coo_rows)."""
    from .distributed import _as_tensor
    _, ci, va = res.device_ptrs()
    nnz = res.nnz
    tdt = _S._torch_dtype(res.dtype)
    rows = torch.empty(max(nnz, 1), dtype=torch.int32, device=device)
    torch.cuda.synchronize(device)
    if nnz:
        res.coo_rows_into(rows.data_ptr())
    cols = _as_tensor(ci, nnz, "<i4", device, torch.int32)
    vals = _as_tensor(va, nnz, "<f4" if res.dtype == np.float32 else "<f8", device, tdt)
    return _DeviceLayerInput(res.shape, rows, cols, vals, nnz, keep=(res,))


def sparse_linear(act, weight, bias=None, relu=False, ctx=None, dtype=np.float32):
    """``relu(act @ weight.T + bias)``: product, bias and ReLU on the GPU (osp_spgemm_coo + osp_csr_bias_relu).
    act: (batch x in), weight: (out x in), both dense tensors / arrays or scipy sparse; returns scipy CSR."""
    out, _ = mlp_forward(act, [(weight, bias)], ctx=ctx, dtype=dtype, relu_last=relu)
    return out


def mlp_forward(x, layers, ctx=None, dtype=np.float32, relu_last=False):
    """layers = [(W1, b1), (W2, b2), ...]; ReLU after every layer but the last (``models.py:17-31``).
    Returns (logits CSR, [activation CSRs]) like ``MLP1.forward`` returns ``(x3, (x1, x2))``.
    The activations never leave the GPU between layers: a layer's result (CSR in HBM) is the next product's operand as it
    stands; only what is returned is copied to the host, at the end."""
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    M, K, r, c, v = _coo_on_device(x, dtype, device)
    cur = _DeviceLayerInput((M, K), r, c, v, v.numel())
    results = []
    for li, (w, b) in enumerate(layers):
        last = li == len(layers) - 1
        res = _layer_on_device(ctx, cur, _coo_on_device(w, dtype, device), b, relu_last if last else True, dtype, device)
        results.append(res)
        if not last:
            cur = _result_as_input(res, device)
    outs = [r_.to_scipy() for r_ in results]
    for r_ in results:
        r_.close()
    return outs[-1], outs[:-1]


def mlp_forward_from_mtx(directory, nlayers=3, ctx=None, dtype=np.float32):
    """Run the chain on the files ``get_MLP1`` dumps: ``act_0.mtx``, ``fc{i}_weight.mtx``, ``fc{i}_bias.mtx``."""
    def load(name):
        nr, nc, r, c, v = _S.read_mtx(os.path.join(directory, name))
        return sp.csr_matrix((v.astype(dtype), (r, c)), shape=(nr, nc))
    layers = []
    for i in range(1, nlayers + 1):
        bias_path = os.path.join(directory, f"fc{i}_bias.mtx")
        bias = load(f"fc{i}_bias.mtx").toarray().reshape(-1) if os.path.exists(bias_path) else None
        layers.append((load(f"fc{i}_weight.mtx"), bias))
    return mlp_forward(load("act_0.mtx"), layers, ctx=ctx, dtype=dtype)


def weight_chain(weights, ctx=None, dtype=np.float32):
    """``W_n @ ... @ W_2 @ W_1`` for ``nn.Linear`` weights (each out x in), sparse x sparse on the GPU."""
    acc = weights[0]
    for w in weights[1:]:
        acc = _S.spgemm(w, acc, transpose_b=False, ctx=ctx, dtype=dtype)
    return acc if sp.issparse(acc) else sp.csr_matrix(np.asarray(acc))


# ---- the conv stage of LeNet (models.py:35-84, get_mtx_files.py:98-133) ---------------------------------------------
def _dev_ptrs(act):
    """(rows, cols, vals) device addresses of a _DeviceLayerInput (0 when it has no entries)."""
    if not act.nnz:
        return 0, 0, 0
    return act.rows.data_ptr(), act.cols.data_ptr(), act.vals.data_ptr()


def _nhwc_on_device(x, dtype, device):
    """NCHW tensor / array -> ((N, C, H, W), the "pixel x channel" matrix (row n*H*W + y*W + x, column c) as device COO)."""
    t = x.detach().cpu() if hasattr(x, "detach") else torch.from_numpy(np.asarray(x))
    N, C, H, W = t.shape
    M, K, r, c, v = _coo_on_device(t.permute(0, 2, 3, 1).reshape(N * H * W, C), dtype, device)
    return (N, C, H, W), _DeviceLayerInput((M, K), r, c, v, v.numel())


def _host_bias(b, dtype):
    if b is None:
        return None
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else (b.toarray() if sp.issparse(b) else np.asarray(b))
    return b.reshape(-1).astype(dtype)


def _conv_product(ctx, act, shape, weight, geom, dtype, device):
    """im2col(act) * W^T on the device (osp_spgemm_conv2d); weight: OC x (C*kh*kw) (dense, ndarray or scipy).
    Returns the (N*OH*OW) x OC CsrResult."""
    N, C, H, W = shape
    OC, K, wr, wc, wv = _coo_on_device(weight, dtype, device)
    if K != C * geom.kh * geom.kw:
        raise _S.OspError(1, f"weight has {K} columns, the input's unfold has C*kh*kw = {C * geom.kh * geom.kw}")
    torch.cuda.synchronize(device)   # the library works on its own stream
    w_ptrs = (wr.data_ptr(), wc.data_ptr(), wv.data_ptr()) if wv.numel() else (0, 0, 0)
    return ctx.spgemm_conv2d_device(dtype, N, C, H, W, act.nnz, _dev_ptrs(act), OC, wv.numel(), w_ptrs, geom)


def to_nchw(csr, N, C, H, W):
    """A "pixel x channel" activation ((N*H*W) x C CSR) as the dense N x C x H x W tensor torch's layers produce."""
    return torch.from_numpy(np.asarray(csr.toarray()).reshape(N, H, W, C)).permute(0, 3, 1, 2).contiguous()


def unfold(x, kernel_size, padding=0, stride=1, dilation=1, ctx=None, dtype=np.float32):
    """im2col of an NCHW input on the GPU (osp_im2col_csc), as scipy CSR in get_LeNet's layout: ``torch.nn.Unfold(...)(x)
    .swapaxes(1, 2).reshape(-1, C*kh*kw)`` -- row n*OH*OW + oy*OW + ox, column c*kh*kw + ky*kw + kx -- with the zeros
    dropped (``get_mtx_files.py:98-133``)."""
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    (N, C, H, W), act = _nhwc_on_device(x, dtype, device)
    g = _S.conv2d_geometry(kernel_size, stride, padding, dilation)
    OH = _S.conv2d_output_size(H, g.kh, g.stride_h, g.pad_h, g.dil_h)
    OW = _S.conv2d_output_size(W, g.kw, g.stride_w, g.pad_w, g.dil_w)
    K = C * g.kh * g.kw
    torch.cuda.synchronize(device)
    nnz = ctx.im2col_device(dtype, N, C, H, W, act.nnz, _dev_ptrs(act), g)
    tdt = _S._torch_dtype(dtype)
    colptr = torch.empty(K + 1, dtype=torch.int64, device=device)
    rowidx = torch.empty(max(nnz, 1), dtype=torch.int32, device=device)
    vals = torch.empty(max(nnz, 1), dtype=tdt, device=device)
    torch.cuda.synchronize(device)
    ctx.im2col_device(dtype, N, C, H, W, act.nnz, _dev_ptrs(act), g, out_ptrs=(colptr.data_ptr(), rowidx.data_ptr(), vals.data_ptr()))
    a = sp.csc_matrix((vals[:nnz].cpu().numpy(), rowidx[:nnz].cpu().numpy().view(np.uint32).astype(np.int64), colptr.cpu().numpy()),
                      shape=(N * OH * OW, K))
    return a.tocsr()


def sparse_conv2d(x, weight, bias=None, stride=1, padding=0, relu=False, dilation=1, ctx=None, dtype=np.float32):
    """``relu(F.conv2d(x, weight, bias, stride, padding, dilation))`` on the GPU: im2col + product (osp_spgemm_conv2d), then
    bias + ReLU (osp_csr_bias_relu).  x: NCHW, weight: OC x C x kh x kw.  Returns the "pixel x channel" activation,
    scipy CSR (N*OH*OW) x OC (``to_nchw`` densifies it)."""
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    shape, act = _nhwc_on_device(x, dtype, device)
    w = weight.detach().cpu() if hasattr(weight, "detach") else torch.from_numpy(np.asarray(weight))
    g = _S.conv2d_geometry((w.shape[2], w.shape[3]), stride, padding, dilation)
    prod = _conv_product(ctx, act, shape, w.reshape(w.shape[0], -1), g, dtype, device)
    out = prod.bias_relu(_host_bias(bias, dtype), relu) if (bias is not None or relu) else prod
    if out is not prod:
        prod.close()
    res = out.to_scipy()
    out.close()
    return res


def sparse_max_pool2d(x, kernel_size, stride=None, ctx=None, dtype=np.float32):
    """``F.max_pool2d(x, kernel_size, stride)`` of an NCHW input on the GPU (osp_csr_maxpool2d; no padding, floor mode):
    the "pixel x channel" activation, scipy CSR (N*PH*PW) x C, an absent entry of x counting as 0."""
    ctx = ctx or _S.default_context()
    t = x.detach().cpu() if hasattr(x, "detach") else torch.from_numpy(np.asarray(x))
    N, C, H, W = t.shape
    m = sp.csr_matrix(t.permute(0, 2, 3, 1).reshape(N * H * W, C).numpy().astype(dtype))
    m.sort_indices()
    # the activation as a library CSR result: the merge of ONE part is the part itself
    res = ctx.merge_csr_parts(N * H * W, C, [(m.indptr, m.indices, m.data)])
    out = res.maxpool2d(N, H, W, kernel_size, stride)
    res.close()
    pooled = out.to_scipy()
    out.close()
    return pooled


def _lenet_tail(ctx, prod1, N, H, W, p, dtype, device):
    """LeNet.forward (models.py:54-84) from conv1's product on, every step on the device: conv1 bias + ReLU -> pool ->
    conv2 + bias + ReLU -> pool -> flatten -> fc1 -> fc2 -> fc3.  Returns (logits, (xc1, xcp1, xc2, xcp2, xf0, xf1, xf2))."""
    res = [prod1]
    try:
        xc1 = prod1.bias_relu(_host_bias(p["conv1_bias"], dtype), True)
        res.append(xc1)
        xcp1 = xc1.maxpool2d(N, H, W, 2)
        res.append(xcp1)
        H2, W2 = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        w2 = p["conv2_weight"]
        w2 = w2.reshape(w2.shape[0], -1) if len(w2.shape) == 4 else w2
        C2 = xcp1.shape[1]
        k2 = int(round((w2.shape[1] // C2) ** 0.5))
        prod2 = _conv_product(ctx, _result_as_input(xcp1, device), (N, C2, H2, W2), w2, _S.conv2d_geometry(k2), dtype, device)
        res.append(prod2)
        OH2, OW2 = H2 - k2 + 1, W2 - k2 + 1
        xc2 = prod2.bias_relu(_host_bias(p["conv2_bias"], dtype), True)
        res.append(xc2)
        xcp2 = xc2.maxpool2d(N, OH2, OW2, 2)
        res.append(xcp2)
        # flatten = xcp2.view(-1, C*PH*PW) in NCHW order: entry (n*PH*PW + q, c) -> (n, c*PH*PW + q), index arithmetic only
        q = ((OH2 - 2) // 2 + 1) * ((OW2 - 2) // 2 + 1)
        a = _result_as_input(xcp2, device)
        r = a.rows[:a.nnz].long()
        rows = (r // q).to(torch.int32)
        cols = (a.cols[:a.nnz].long() * q + r % q).to(torch.int32)
        xf0 = _DeviceLayerInput((N, xcp2.shape[1] * q), rows, cols, a.vals[:a.nnz], a.nnz, keep=(a,))
        cur, fcs = xf0, []
        for i in (1, 2, 3):
            out = _layer_on_device(ctx, cur, _coo_on_device(p[f"fc{i}_weight"], dtype, device), p.get(f"fc{i}_bias"), i < 3, dtype,
                                   device)
            res.append(out)
            fcs.append(out)
            if i < 3:
                cur = _result_as_input(out, device)
        xf0_host = sp.csr_matrix((xf0.vals.cpu().numpy(), (rows.cpu().numpy(), cols.cpu().numpy())), shape=xf0.shape)
        acts = (xc1.to_scipy(), xcp1.to_scipy(), xc2.to_scipy(), xcp2.to_scipy(), xf0_host, fcs[0].to_scipy(), fcs[1].to_scipy())
        return fcs[2].to_scipy(), acts
    finally:
        torch.cuda.synchronize(device)   # torch's reads of borrowed result arrays are done before they go back to the pool
        for r_ in res:
            r_.close()


def _lenet_params(params):
    """state_dict names (``conv1.weight``) or get_LeNet's file names (``conv1_weight``) -> the latter."""
    return {k.replace(".", "_"): v for k, v in dict(params).items()}


def lenet_forward(x, params, ctx=None, dtype=np.float32):
    """``LeNet.forward`` (models.py:54-84) with every layer on the GPU and the activations kept there between layers.
    x: N x 1 x 28 x 28 (NCHW); params: the model's weights and biases (``model.state_dict()`` or get_LeNet's names).
    Returns ``(logits, (xc1, xcp1, xc2, xcp2, xf0, xf1, xf2))`` as scipy CSR: the conv-stage activations "pixel x channel",
    (N*H*W) x C (``to_nchw``), the fc-stage ones batch x features."""
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)
    p = _lenet_params(params)
    shape, act = _nhwc_on_device(x, dtype, device)
    N, C, H, W = shape
    w1 = p["conv1_weight"]
    w1 = w1.detach().cpu() if hasattr(w1, "detach") else torch.from_numpy(np.asarray(w1))
    g1 = _S.conv2d_geometry((w1.shape[2], w1.shape[3]), 1, 2)   # Conv2d(1, 6, kernel_size=5, stride=1, padding=2)
    prod1 = _conv_product(ctx, act, shape, w1.reshape(w1.shape[0], -1), g1, dtype, device)
    OH = _S.conv2d_output_size(H, g1.kh, 1, 2)
    OW = _S.conv2d_output_size(W, g1.kw, 1, 2)
    return _lenet_tail(ctx, prod1, N, OH, OW, p, dtype, device)


def lenet_forward_from_mtx(directory, image_size=28, ctx=None, dtype=np.float32):
    """Run the chain on the files ``get_LeNet`` dumps: ``act_0.mtx`` (the input, already unfolded: conv1 is exactly the
    reference CLI's ``act_0 * conv1_weight^T``), ``conv{1,2}_weight.mtx`` (OC x C*kh*kw), ``conv{1,2}_bias.mtx``,
    ``fc{1,2,3}_weight.mtx``, ``fc{1,2,3}_bias.mtx``.  Returns what ``lenet_forward`` returns."""
    ctx = ctx or _S.default_context()
    device = torch.device("cuda", ctx.device)

    def load(name):
        nr, nc, r, c, v = _S.read_mtx(os.path.join(directory, name))
        return sp.csr_matrix((v.astype(dtype), (r, c)), shape=(nr, nc))
    names = ["conv1_bias", "conv2_weight", "conv2_bias"] + [f"fc{i}_{t}" for i in (1, 2, 3) for t in ("weight", "bias")]
    p = {n: load(n + ".mtx") for n in names}
    for n in names:
        if n.endswith("bias"):
            p[n] = p[n].toarray().reshape(-1)
    act0 = load("act_0.mtx")
    M, K, r, c, v = _coo_on_device(act0, dtype, device)
    # conv1 (padding 2) keeps the image size: the product's rows are the N*28*28 output pixels
    prod1 = _layer_on_device(ctx, _DeviceLayerInput((M, K), r, c, v, v.numel()), _coo_on_device(load("conv1_weight.mtx"), dtype, device),
                             None, False, dtype, device)
    N = M // (image_size * image_size)
    return _lenet_tail(ctx, prod1, N, image_size, image_size, p, dtype, device)
