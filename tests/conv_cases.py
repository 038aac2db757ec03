"""What tests/test_gpu_conv.py, tests/test_conv_model_cpu.py and the child processes share: the inputs of the conv stage's
edge cases (host arrays only: the CPU test runs them against the model), the calls that take them to the device, and a
fixed slice whose outputs are hashed.  A helper, not a test file.

``python -m tests.conv_cases`` runs the slice on a context of its own and prints ``CONV_SLICE <sha256> calls=<n>``: the test
starts it under OSP_POISON=1 and under OSP_GUARD=1 (both are read once per process) and compares the digest with the one of
its own process.  Any exception ends the child at once with DEVICE_ERROR_STATUS: it starts nothing more on the GPU."""
import hashlib
import os
import sys
import traceback

import numpy as np

from tests import conv_model as model
from tests import test_gpu_apply_mask as am   # the special values, _dev and DEV only

ROOT = model.ROOT
CHUNK, WAVE = model.CHUNK, model.WAVE
DEVICE_ERROR_STATUS = 3
DTYPES = (np.float32, np.float64)

special = am._special   # NaNs with payloads, infinities, both zeros, denormals, the largest number and 1


def values(n, dt, seed):
    """Random values, every seventh entry a special one."""
    val = np.random.default_rng(seed).standard_normal(n).astype(dt)
    val[::7] = np.resize(np.roll(special(dt), seed), len(val[::7]))
    return val


def shuffled(coo, seed):
    order = np.random.default_rng(seed).permutation(len(coo[0]))
    return tuple(np.ascontiguousarray(a[order]) for a in coo)


# ---- im2col: chunk and wave edges ----------------------------------------------------------------------------------------------------
EDGE_SHAPE = (2, 11, 33, 63)                                                   # N, C, H, W: 4158 pixels
EDGE_COUNTS = [0, 1, WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 0]   # entries per channel
EDGE_GEOMS = [model.geom(3, 1, 1), model.geom(3, 2, 1, 2)]                     # 3x3 pad 1 stride 1; 3x3 pad 1 stride 2 dilation 2


def edge_input(dt):
    """x as a shuffled COO (pixels, channels, values) whose channels hold exactly EDGE_COUNTS entries."""
    N, C, H, W = EDGE_SHAPE
    assert len(EDGE_COUNTS) == C and max(EDGE_COUNTS) <= N * H * W
    rng = np.random.default_rng(71)
    pix = np.concatenate([np.sort(rng.choice(N * H * W, k, replace=False)) for k in EDGE_COUNTS]).astype(np.uint32)
    ch = np.repeat(np.arange(C, dtype=np.uint32), EDGE_COUNTS)
    return shuffled((pix, ch, values(len(pix), dt, 72)), 73)


# ---- conv2d ----------------------------------------------------------------------------------------------------------------------------
CONV_SHAPE = (2, 3, 9, 11)
CONV_GEOMS = {"stride2-pad2": model.geom(3, 2, 2), "dilation2": model.geom(3, 1, 0, 2), "rect": model.geom((2, 3), (2, 1))}
CONV_OC = (1, 5)


def conv_input(dt, g, OC, seed=81):
    """(x, w): both shuffled COO lists with special values; x over CONV_SHAPE's pixels and channels, w of OC x (C*kh*kw)."""
    N, C, H, W = CONV_SHAPE
    rng = np.random.default_rng(seed)
    on = np.flatnonzero(rng.random(N * H * W * C) < 0.5)
    x = shuffled(((on // C).astype(np.uint32), (on % C).astype(np.uint32), values(len(on), dt, seed + 1)), seed + 2)
    K = C * g.kh * g.kw
    won = np.flatnonzero(rng.random(OC * K) < 0.6)
    wv = values(len(won), dt, seed + 3)
    wv[1:3] = special(dt)[:2]                      # (a W of one short row still holds both NaNs)
    w = shuffled(((won // K).astype(np.uint32), (won % K).astype(np.uint32), wv), seed + 4)
    return x, w


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------------
POOL_SHAPE = (2, 9, 11)                                                        # N, H, W
POOL_CHANNELS = (1, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE, 2 * WAVE + 1)
# (kernel, stride): gaps between the windows; one window, the whole image; the input minus its stored zeros; a remainder row
# and column (9 x 11 by 2); two that fit exactly and overlap
POOL_GEOMS = [(2, 3), ((9, 11), None), (1, 1), (2, None), (3, 2), ((2, 3), (1, 2))]


def pool_input(dt, C, seed=91):
    """A CSR activation of POOL_SHAPE with C channels, about half its entries stored, special values (stored +0 and -0, NaNs,
    infinities) among them; image 0's rows 0..3 x columns 0..3 are all present and negative in every channel, its rows 4..7 x
    columns 0..3 likewise but for ONE absent tap per 2x2 window (the window's maximum is then the absent +0: dropped)."""
    N, H, W = POOL_SHAPE
    rng = np.random.default_rng([seed, C])
    on = rng.random((N * H * W, C)) < 0.5
    neg = np.array([y * W + x for y in range(8) for x in range(4)])
    on[neg] = True
    on[[y * W + x for y in (4, 6) for x in (1, 2)]] = False
    rowptr = np.concatenate([[0], np.cumsum(on.sum(1))]).astype(np.int64)
    col = np.nonzero(on)[1].astype(np.uint32)
    val = values(len(col), dt, seed + C)
    for r in neg:
        seg = slice(rowptr[r], rowptr[r + 1])
        val[seg] = -np.abs(rng.standard_normal(rowptr[r + 1] - rowptr[r]).astype(dt)) - dt(0.5)
    return rowptr, col, val


def nan_position_input(dt, kh, kw):
    """One (kh, kw) window per image, 2 * kh * kw images, 3 channels; pooled with kernel = stride = (kh, kw).
    Image t < T = kh*kw: channel 0 holds a NaN (payload A) at tap t among finite values of both signs, channel 1 the same NaN
    with every other tap ABSENT, channel 2 finite values only.  Image T + t: channel 0 holds NaN A at tap t and NaN B (another
    payload, the other sign) at tap (t + 1) % T, so that each is the window's first once; channel 1 a NaN B at tap t under
    a stored +inf at tap 0 (t > 0).  Returns (csr, N): the result of the rule is the window's first NaN in tap order."""
    T = kh * kw
    sp_ = special(dt)
    nan_a, nan_b, inf = sp_[0], sp_[1], sp_[2]
    assert np.isnan(nan_a) and np.isnan(nan_b) and am._bits(sp_[:2])[0] != am._bits(sp_[:2])[1] and np.isposinf(inf)
    rng = np.random.default_rng(95)
    lists = []                                   # per pixel row: [(channel, value)]
    for img in range(2 * T):
        t = img % T
        for tap in range(T):
            fin = rng.standard_normal(2).astype(dt) * dt(3)
            row = [(0, fin[0]), (2, fin[1])]
            if tap == t:
                row[0] = (0, nan_a)
                row.insert(1, (1, nan_a if img < T else nan_b))
            elif img >= T and tap == (t + 1) % T:
                row[0] = (0, nan_b)
            if img >= T and tap == 0 and t > 0:
                row.insert(1, (1, inf))
            lists.append(sorted(row, key=lambda cv: cv[0]))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    col = np.array([c for r in lists for c, _ in r], np.uint32)
    val = np.array([am._bits(np.array([v], dt))[0] for r in lists for _, v in r], am._bits(sp_).dtype).view(dt)
    return (rowptr, col, val), 2 * T


NAN_WINDOWS = [(2, 2), (2, 3)]


# ---- coo_rows ---------------------------------------------------------------------------------------------------------------------------
ROWS_LENGTHS = [0, 0, 0, 1, WAVE + 1, 0, 0, 2 * WAVE + 1, 0, 3, 0, 0]           # runs of empty rows, a row of 65 and of 129 entries


def rows_input(dt, lengths=ROWS_LENGTHS):
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.arange(k) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.uint32)
    return (rowptr, col, values(len(col), dt, 97)), max(max(lengths), 1)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
def lib_geom(g):
    from outerspace_amd import spgemm as S
    return S.conv2d_geometry((g.kh, g.kw), (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw))


def upload_coo(coo):
    """The three arrays of a COO list as device tensors (every byte kept), the device synchronised."""
    import torch
    ts = [am._dev(a) for a in coo]
    torch.cuda.synchronize(am.DEV)
    return ts


def ptrs(ts):
    return tuple(t.data_ptr() for t in ts)


def build(ctx, csr, ncol):
    """The CSR as a library result through ``Context.build(dup="error")``; its three arrays come back bit for bit."""
    rowptr, col, val = csr
    return ctx.build(len(rowptr) - 1, ncol, model.coo_rows(rowptr), col, val, dup="error", dtype=val.dtype.type, space="host")[0]


def im2col(ctx, dt, shape, x, g):
    """osp_im2col_csc on the raw device COO ``x``: (colptr, rowidx, vals, the nnz of the count-only call)."""
    import torch
    N, C, H, W = shape
    ts = upload_coo(x)
    lg = lib_geom(g)
    nnz = ctx.im2col_device(dt, N, C, H, W, len(x[0]), ptrs(ts), lg)
    colptr = torch.full((C * g.kh * g.kw + 1,), -1, dtype=torch.int64, device=am.DEV)
    rowidx = torch.full((max(nnz, 1),), -1, dtype=torch.int32, device=am.DEV)
    vals = torch.zeros(max(nnz, 1), dtype=torch.float32 if dt == np.float32 else torch.float64, device=am.DEV)
    torch.cuda.synchronize(am.DEV)
    nnz2 = ctx.im2col_device(dt, N, C, H, W, len(x[0]), ptrs(ts), lg, out_ptrs=ptrs((colptr, rowidx, vals)))
    assert nnz2 == nnz
    return colptr.cpu().numpy(), rowidx[:nnz].cpu().numpy().view(np.uint32), vals[:nnz].cpu().numpy(), nnz


def conv2d(ctx, dt, shape, x, OC, w, g):
    """osp_spgemm_conv2d on raw device COO lists; the caller closes the result."""
    N, C, H, W = shape
    xs, ws = upload_coo(x), upload_coo(w)
    return ctx.spgemm_conv2d_device(dt, N, C, H, W, len(x[0]), ptrs(xs), OC, len(w[0]), ptrs(ws), lib_geom(g))


def coo_rows(res):
    """osp_result_coo_rows into a device array of res.nnz entries."""
    import torch
    rows = torch.full((max(res.nnz, 1),), -1, dtype=torch.int32, device=am.DEV)
    torch.cuda.synchronize(am.DEV)
    res.coo_rows_into(rows.data_ptr())
    return rows[:res.nnz].cpu().numpy().view(np.uint32)


# ---- the slice that the children repeat -------------------------------------------------------------------------------------------------
def slice_digest(ctx):
    """sha256 over the outputs of the chunk-edge im2col (both geometries), one conv2d, the NaN-position pools and coo_rows,
    in both dtypes, and the number of library calls that made them."""
    h = hashlib.sha256()
    calls = 0

    def add(*arrays):
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())

    for dt in DTYPES:
        x = edge_input(dt)
        for g in EDGE_GEOMS:
            colptr, rows, vals, nnz = im2col(ctx, dt, EDGE_SHAPE, x, g)
            add(colptr, rows, vals)
            h.update(repr(nnz).encode())
            calls += 2
        g = CONV_GEOMS["rect"]
        cx, cw = conv_input(dt, g, CONV_OC[-1])
        res = conv2d(ctx, dt, CONV_SHAPE, cx, CONV_OC[-1], cw, g)
        try:
            add(*res.to_host())
            h.update(repr((res.shape, res.nnz, res.info["partials"])).encode())
        finally:
            res.close()
        calls += 1
        for kh, kw in NAN_WINDOWS:
            csr, N = nan_position_input(dt, kh, kw)
            a = build(ctx, csr, 3)
            try:
                out = a.maxpool2d(N, kh, kw, (kh, kw))
                try:
                    add(*out.to_host())
                    h.update(repr((out.shape, out.nnz)).encode())
                finally:
                    out.close()
            finally:
                a.close()
            calls += 1
        csr, ncol = rows_input(dt)
        a = build(ctx, csr, ncol)
        try:
            add(coo_rows(a))
        finally:
            a.close()
        calls += 1
    return h.hexdigest(), calls


def main():
    try:
        from outerspace_amd import spgemm as S
        ctx = S.Context(0)
        digest, calls = slice_digest(ctx)
        ctx.close()
    except BaseException:   # a device or runtime error, or anything else: nothing further is started on the GPU
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(DEVICE_ERROR_STATUS)
    print(f"CONV_SLICE {digest} calls={calls}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
