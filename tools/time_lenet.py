#!/usr/bin/env python3
"""Times the conv stage of the sparse LeNet (models.py:35-84) at batch 1024, f32, per layer and per step: im2col
(osp_im2col_csc, host clock around the synchronous call), the conv product (osp_spgemm_conv2d: ms_total less ms_ingest,
device events), the bias + ReLU epilogue and the max-pool (their ms_total), with dense torch F.conv2d on the same GPU
beside them for context; then one whole lenet_forward against the dense forward (host clock, both ending in a synchronise).
Input: relu(randn - 0.8) images (about 21 % non-zero), weights pruned by magnitude to 30 %."""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import spgemm as S  # noqa: E402
from outerspace_amd import sparse_util as su  # noqa: E402

N, REPS = 1024, 8
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(1)
x = torch.relu(torch.randn(N, 1, 28, 28, generator=g) - 0.8)
shapes = {"conv1_weight": (6, 1, 5, 5), "conv1_bias": (6,), "conv2_weight": (16, 6, 5, 5), "conv2_bias": (16,),
          "fc1_weight": (120, 400), "fc1_bias": (120,), "fc2_weight": (84, 120), "fc2_bias": (84,), "fc3_weight": (10, 84), "fc3_bias": (10,)}
p = {}
for name, shp in shapes.items():
    t = torch.randn(*shp, generator=g)
    p[name] = su.prune_by_magnitude(t / float(np.prod(shp[1:])) ** 0.5, 0.3) if name.endswith("weight") else t * 0.1


def med(v):
    return float(np.median(v[2:] if len(v) > 4 else v))


def dense_ms(fn):
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    return med(ms)


ctx = S.default_context()
xd = x.to(dev)
w1d, b1d = p["conv1_weight"].to(dev), p["conv1_bias"].to(dev)
w2d, b2d = p["conv2_weight"].to(dev), p["conv2_bias"].to(dev)
xcp1_dense = F.max_pool2d(torch.relu(F.conv2d(xd, w1d, b1d, padding=2)), 2)
layers = [("conv1", x, (1, 28, 28), p["conv1_weight"], p["conv1_bias"], 2, lambda: F.conv2d(xd, w1d, b1d, padding=2)),
          ("conv2", xcp1_dense.cpu(), (6, 14, 14), p["conv2_weight"], p["conv2_bias"], 0, lambda: F.conv2d(xcp1_dense, w2d, b2d))]
for name, inp, (C, H, W), w, b, pad, dense in layers:
    shape, act = su._nhwc_on_device(inp, np.float32, dev)
    geom = S.conv2d_geometry(5, 1, pad)
    OC = w.shape[0]
    _, _, wr, wc, wv = su._coo_on_device(w.reshape(OC, -1), np.float32, dev)
    torch.cuda.synchronize(dev)
    xp = su._dev_ptrs(act)
    wp = (wr.data_ptr(), wc.data_ptr(), wv.data_ptr())
    t_im2col, t_prod, t_epi, t_pool = [], [], [], []
    K = C * 25
    colptr = torch.empty(K + 1, dtype=torch.int64, device=dev)
    nnz_a = ctx.im2col_device(np.float32, N, C, H, W, act.nnz, xp, geom)
    rowidx = torch.empty(max(nnz_a, 1), dtype=torch.int32, device=dev)
    vals = torch.empty(max(nnz_a, 1), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(REPS):
        t0 = time.perf_counter()
        ctx.im2col_device(np.float32, N, C, H, W, act.nnz, xp, geom)
        ctx.im2col_device(np.float32, N, C, H, W, act.nnz, xp, geom, out_ptrs=(colptr.data_ptr(), rowidx.data_ptr(), vals.data_ptr()))
        t_im2col.append((time.perf_counter() - t0) * 1e3)
        r = ctx.spgemm_conv2d_device(np.float32, N, C, H, W, act.nnz, xp, OC, wv.numel(), wp, geom)
        t_prod.append(r.info["ms_total"] - r.info["ms_ingest"])
        e = r.bias_relu(b.numpy(), True)
        t_epi.append(e.info["ms_total"])
        q = e.maxpool2d(N, H - 4 + 2 * pad, W - 4 + 2 * pad, 2)
        t_pool.append(q.info["ms_total"])
        info = (r.info, e.nnz, q.nnz)
        for h in (q, e, r):
            h.close()
    print(f"{name}: N={N} nnz_x={act.nnz} nnz_A={nnz_a} P={info[0]['partials']} nnz_out={info[0]['nnz_c']} relu_nnz={info[1]} pool_nnz={info[2]} | "
          f"im2col (count + write calls, host clock) {med(t_im2col):.3f} ms, in-product ingest {info[0]['ms_ingest']:.3f} ms, "
          f"product {med(t_prod):.3f} ms, bias+relu {med(t_epi):.3f} ms, pool {med(t_pool):.3f} ms | dense F.conv2d {dense_ms(dense):.3f} ms",
          flush=True)

wall, dense_wall = [], []
for _ in range(REPS):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    su.lenet_forward(x, p, ctx=ctx)
    wall.append((time.perf_counter() - t0) * 1e3)
pd = {k: v.to(dev) for k, v in p.items()}


def dense_forward():
    h = F.max_pool2d(torch.relu(F.conv2d(xd, pd["conv1_weight"], pd["conv1_bias"], padding=2)), 2)
    h = F.max_pool2d(torch.relu(F.conv2d(h, pd["conv2_weight"], pd["conv2_bias"])), 2).view(-1, 400)
    h = torch.relu(F.linear(h, pd["fc1_weight"], pd["fc1_bias"]))
    h = torch.relu(F.linear(h, pd["fc2_weight"], pd["fc2_bias"]))
    return F.linear(h, pd["fc3_weight"], pd["fc3_bias"])


print(f"lenet_forward N={N}: {med(wall):.1f} ms per call (host clock, host input and scipy outputs included) | "
      f"dense torch forward on the device {dense_ms(dense_forward):.3f} ms", flush=True)
