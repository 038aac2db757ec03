"""A plain numpy model of the conv stage (osp_conv.h): im2col into CSC, max-pool of a CSR activation and the row index of
every entry of a CSR.  No torch: tests/test_conv_model_cpu.py ties it to torch.nn.Unfold and F.max_pool2d, and
tests/test_gpu_conv.py compares the library with it, values as bits.  A helper, not a test file.

Activations are "pixel x channel" matrices: row n*H*W + y*W + x, column c.  Values are only ever copied, so every output
value has the bits of an input value (a NaN keeps its payload, a zero its sign)."""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "outerspace_amd", "csrc")
# the input entries of one channel that one wave of im2col takes, and the lanes of a wave (a wave step of max-pool takes
# that many channels)
CHUNK = int(re.search(r"kConvChunk\s*=\s*(\d+)", open(os.path.join(_CSRC, "osp_conv.h")).read()).group(1))
WAVE = int(re.search(r"kWave\s*=\s*(\d+)", open(os.path.join(_CSRC, "osp_prims.h")).read()).group(1))

Geom = collections.namedtuple("Geom", "kh kw sh sw ph pw dh dw")


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def geom(kernel_size, stride=1, padding=0, dilation=1):
    """torch-style arguments (an int or an (h, w) pair each) as a Geom."""
    return Geom(*_pair(kernel_size), *_pair(stride), *_pair(padding), *_pair(dilation))


def output_size(size, k, stride, pad, dil):
    span = size + 2 * pad - dil * (k - 1) - 1
    return span // stride + 1 if span >= 0 else 0


def by_channel(C, npix, coo):
    """The COO (pixel, channel, value) of x in any order -> (channel, pixel, value) sorted by channel, then pixel.  Raises
    ValueError on an index outside its dimension or a coordinate given twice."""
    pix, ch, val = (np.asarray(a) for a in coo)
    pix, ch = pix.astype(np.int64), ch.astype(np.int64)
    if len(pix) and (pix.min() < 0 or pix.max() >= npix or ch.min() < 0 or ch.max() >= C):
        raise ValueError("x (COO): an index outside its dimension")
    order = np.lexsort((pix, ch))
    ch, pix, val = ch[order], pix[order], val[order]
    if np.any((np.diff(ch) == 0) & (np.diff(pix) == 0)):
        raise ValueError("x (COO): duplicate coordinate")
    return ch, pix, val


def unfold_sorted(N, C, H, W, sorted_x, g):
    """im2col of entries already grouped by channel with ascending pixels (by_channel's output)."""
    ch, pix, val = sorted_x
    OH, OW = output_size(H, g.kh, g.sh, g.ph, g.dh), output_size(W, g.kw, g.sw, g.pw, g.dw)
    khkw = g.kh * g.kw
    n, rem = np.divmod(pix, H * W)
    y, x = np.divmod(rem, W)
    ks, rows, vals = [], [], []
    for ky in range(g.kh):
        for kx in range(g.kw):
            ty, tx = y + g.ph - ky * g.dh, x + g.pw - kx * g.dw
            keep = (ty >= 0) & (tx >= 0) & (ty % g.sh == 0) & (tx % g.sw == 0)
            oy, ox = ty // g.sh, tx // g.sw
            keep &= (oy < OH) & (ox < OW)
            ks.append(ch[keep] * khkw + ky * g.kw + kx)
            rows.append(((n * OH + oy) * OW + ox)[keep])
            vals.append(val[keep])
    k, row, v = np.concatenate(ks), np.concatenate(rows), np.concatenate(vals)
    order = np.argsort(k, kind="stable")      # a column's entries stay in pixel order: its rows ascend by the map itself
    K = C * khkw
    colptr = np.concatenate([[0], np.cumsum(np.bincount(k, minlength=K))]).astype(np.int64)
    row = row[order]
    assert all(np.all(np.diff(row[colptr[j]:colptr[j + 1]]) > 0) for j in range(K))
    return colptr, row.astype(np.uint32), np.ascontiguousarray(v[order])


def im2col(N, C, H, W, coo, g):
    """The unfold matrix A of x in CSC: (colptr, rowidx, vals), (N*OH*OW) x (C*kh*kw).  coo = (pixels, channels, values) in
    any order.  Column k = (c, ky, kx) holds every STORED entry of channel c -- a stored +0 or -0 like any value -- whose
    pixel (n, y, x) reaches an output row (n, oy, ox) through that tap: oy = (y + ph - ky*dh) / sh an exact quotient below
    OH, likewise ox.  Rows ascend within each column."""
    return unfold_sorted(N, C, H, W, by_channel(C, N * H * W, coo), g)


def fold_first_nan(v, w):
    """One step of the pooling fold over a whole row of channels: v unless it is no NaN and w is larger or a NaN."""
    with np.errstate(invalid="ignore"):
        take = ~np.isnan(v) & (np.isnan(w) | (w > v))
    return np.where(take, w, v)


def maxpool(csr, C, N, H, W, kernel, stride=None, fold=fold_first_nan):
    """MaxPool2d (no padding, no dilation, floor mode) of the CSR activation: (rowptr, col, val) of (N*PH*PW) x C.  Per
    window and channel, over the taps in order (ky outer, kx inner), an absent tap counting as +0: the window's first NaN
    if it holds one, else its maximum; a result that is a zero of either sign is dropped, a NaN is kept."""
    rowptr, col, val = csr
    kh, kw = _pair(kernel)
    sh, sw = _pair(kernel if stride is None else stride)
    assert len(rowptr) == N * H * W + 1 and H >= kh and W >= kw
    PH, PW = (H - kh) // sh + 1, (W - kw) // sw + 1
    lens, cols, vals = [], [], []
    for n in range(N):
        for py in range(PH):
            for px in range(PW):
                taps = [(n * H + py * sh + ky) * W + px * sw + kx for ky in range(kh) for kx in range(kw)]
                segs = [slice(rowptr[t], rowptr[t + 1]) for t in taps]
                present = np.unique(np.concatenate([col[s] for s in segs]))
                win = np.zeros((len(taps), len(present)), val.dtype)         # +0 where a tap has no entry
                for i, s in enumerate(segs):
                    win[i, np.searchsorted(present, col[s])] = val[s]
                v = win[0].copy()
                for i in range(1, len(taps)):
                    v = fold(v, win[i])
                keep = v != 0                                                # (a NaN is no zero)
                lens.append(int(keep.sum()))
                cols.append(present[keep])
                vals.append(v[keep])
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return out_ptr, np.concatenate(cols + [np.zeros(0, np.uint32)]).astype(np.uint32), np.concatenate(vals + [np.zeros(0, val.dtype)])


def coo_rows(rowptr):
    """The row index of every entry of a CSR."""
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.uint32), np.diff(rowptr))
