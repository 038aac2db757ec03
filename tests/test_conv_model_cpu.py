"""tests/conv_model.py against torch on the CPU (torch.nn.Unfold, F.max_pool2d), its refusals, and two planted defects run
against the case lists of tests/conv_cases.py -- the ones tests/test_gpu_conv.py runs on the device -- to show that the cases
contain what bites."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cc
from tests import conv_model as model
from tests.ieee_model import assert_same_bits

DTYPES = [np.float32, np.float64]


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _tdt(dt):
    return torch.float32 if dt == np.float32 else torch.float64


def test_the_constants_are_read_from_the_sources():
    assert (model.CHUNK, model.WAVE) == (2048, 64)
    assert cc.EDGE_COUNTS == [0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 0]
    assert cc.POOL_CHANNELS == (1, 63, 64, 65, 128, 129)
    assert sum(cc.EDGE_COUNTS) == 14530


# ---- unfold ---------------------------------------------------------------------------------------------------------------------------
def _torch_unfold(x, g):
    """Unfold -> swapaxes(1, 2) -> reshape(-1, C*kh*kw), as tests/test_gpu_conv.py's _torch_unfold does."""
    u = torch.nn.Unfold(kernel_size=(g.kh, g.kw), dilation=(g.dh, g.dw), padding=(g.ph, g.pw), stride=(g.sh, g.sw))(x)
    u = torch.swapaxes(u, 1, 2)
    return u.reshape(-1, u.shape[-1]).numpy()


def _dense_without_zeros(shape, dt, seed):
    """A dense NCHW input, about half of it zero and no stored zero in its COO: (tensor, shuffled COO)."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(dt)
    x[rng.random(shape) < 0.5] = 0
    x[x == 0] = 0                                        # (no -0 either)
    nhwc = x.transpose(0, 2, 3, 1).reshape(N * H * W, C)
    pix, ch = np.nonzero(nhwc)
    return torch.from_numpy(x), cc.shuffled((pix.astype(np.uint32), ch.astype(np.uint32), nhwc[pix, ch]), seed + 1)


def _assert_is_unfold(shape, g, dt, seed):
    N, C, H, W = shape
    x, coo = _dense_without_zeros(shape, dt, seed)
    colptr, rows, vals = model.im2col(N, C, H, W, coo, g)
    ref = _torch_unfold(x, g)
    assert ref.shape == (N * model.output_size(H, g.kh, g.sh, g.ph, g.dh) * model.output_size(W, g.kw, g.sw, g.pw, g.dw), C * g.kh * g.kw)
    wr, wc = np.nonzero(ref.T)                           # column-major: CSC order, rows ascending in every column
    assert np.array_equal(colptr, np.concatenate([[0], np.cumsum(np.bincount(wr, minlength=ref.shape[1]))]))
    assert np.array_equal(rows, wc)
    assert np.array_equal(_bits(vals), _bits(ref.T[wr, wc]))
    return ref


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("stride,pad,dil,C", list(itertools.product((1, 2), (0, 2), (1, 2), (1, 3, 6))))
def test_im2col_equals_torch_unfold(dt, stride, pad, dil, C):
    _assert_is_unfold((2, C, 9, 11), model.geom(3, stride, pad, dil), dt, stride * 100 + pad * 10 + dil + C)


@pytest.mark.parametrize("dt", DTYPES)
def test_im2col_equals_torch_unfold_at_the_odd_geometries(dt):
    # a rectangular kernel with another stride and dilation per axis
    _assert_is_unfold((3, 2, 13, 8), model.geom((2, 3), (2, 1), (1, 0), (3, 1)), dt, 1)
    # padding larger than the kernel: whole output rows (and columns) come from padding alone
    g = model.geom(2, 1, 4)
    ref = _assert_is_unfold((1, 2, 5, 4), g, dt, 2)
    OW = model.output_size(4, 2, 1, 4, 1)
    assert not ref[:3 * OW].any() and not ref[-3 * OW:].any() and ref.any()
    # stride larger than the kernel: pixels between two windows reach no output
    _assert_is_unfold((2, 3, 11, 10), model.geom(2, 3), dt, 3)
    for g in cc.CONV_GEOMS.values():
        _assert_is_unfold(cc.CONV_SHAPE, g, dt, 4)
    for g in cc.EDGE_GEOMS:
        _assert_is_unfold((1, 2, 33, 63), g, dt, 5)


def test_im2col_copies_stored_zeros_and_takes_any_order():
    g = model.geom(3, 1, 1)
    for dt in DTYPES:
        x = cc.edge_input(dt)
        N, C, H, W = cc.EDGE_SHAPE
        got = model.im2col(N, C, H, W, x, g)
        order = np.lexsort((x[0], x[1]))
        again = model.im2col(N, C, H, W, tuple(a[order] for a in x), g)
        for a, b in zip(got, again):
            assert np.array_equal(_bits(a) if a.dtype.kind == "f" else a, _bits(b) if b.dtype.kind == "f" else b)
        # the centre tap of a 3x3 pad-1 stride-1 unfold is the channel itself: every stored value, zeros and NaNs too
        for c in range(C):
            k = c * 9 + 4
            mine = x[1][order] == c
            assert np.array_equal(got[1][got[0][k]:got[0][k + 1]], x[0][order][mine])
            assert np.array_equal(_bits(got[2][got[0][k]:got[0][k + 1]]), _bits(x[2][order][mine]))
        zeros = got[2] == 0
        assert zeros.any() and np.signbit(got[2][zeros]).any() and not np.signbit(got[2][zeros]).all() and np.isnan(got[2]).any()


def test_im2col_refuses_duplicates_and_indices_outside():
    g = model.geom(1)
    one = np.ones(2, np.float32)
    with pytest.raises(ValueError, match="duplicate"):
        model.im2col(1, 2, 3, 3, (np.array([4, 4], np.uint32), np.array([1, 1], np.uint32), one), g)
    with pytest.raises(ValueError, match="outside"):
        model.im2col(1, 2, 3, 3, (np.array([4, 9], np.uint32), np.array([1, 1], np.uint32), one), g)
    with pytest.raises(ValueError, match="outside"):
        model.im2col(1, 2, 3, 3, (np.array([4, 5], np.uint32), np.array([1, 2], np.uint32), one), g)
    colptr, rows, vals = model.im2col(1, 2, 3, 3, (np.array([4, 4], np.uint32), np.array([1, 0], np.uint32), one), g)
    assert colptr.tolist() == [0, 1, 2] and rows.tolist() == [4, 4]


# ---- max-pool -------------------------------------------------------------------------------------------------------------------------
def _torch_pool(csr, C, N, H, W, kernel, stride):
    """F.max_pool2d on the densified input, the zeros dropped: (rowptr, col, val)."""
    rowptr, col, val = csr
    dense = np.zeros((N * H * W, C), val.dtype)
    dense[model.coo_rows(rowptr), col] = val
    x = torch.from_numpy(dense.reshape(N, H, W, C)).permute(0, 3, 1, 2).contiguous()
    ref = F.max_pool2d(x, kernel, stride).permute(0, 2, 3, 1).reshape(-1, C).numpy()
    r, c = np.nonzero(ref)                                # (a NaN is no zero)
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=ref.shape[0]))]), c, ref[r, c]


def _assert_is_torch_pool(csr, C, N, H, W, kernel, stride):
    got = model.maxpool(csr, C, N, H, W, kernel, stride)
    want = _torch_pool(csr, C, N, H, W, kernel, stride)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert_same_bits(got[2], want[2])                     # NaNs by position: torch keeps another payload
    return got


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [1, 65])
def test_maxpool_equals_torch(dt, C):
    N, H, W = cc.POOL_SHAPE
    csr = cc.pool_input(dt, C)
    assert np.isnan(csr[2]).any() and (csr[2] == 0).any() and np.isinf(csr[2]).any()
    for kernel, stride in cc.POOL_GEOMS:
        got = _assert_is_torch_pool(csr, C, N, H, W, kernel, stride)
        if (kernel, stride) == (1, 1):                    # the input minus its stored zeros
            keep = csr[2] != 0
            assert np.array_equal(got[1], csr[1][keep]) and np.array_equal(_bits(got[2]), _bits(csr[2][keep]))
        if (kernel, stride) == (2, None):
            # the all-negative full windows keep a negative maximum; one absent tap makes the maximum +0: dropped
            PW = W // 2
            for py, px, kept in ((0, 0, True), (1, 1, True), (2, 0, False), (3, 1, False), (2, 1, False)):
                r = py * PW + px
                seg = got[2][got[0][r]:got[0][r + 1]]
                assert (len(seg) == C and (seg < 0).all()) if kept else len(seg) == 0, (py, px)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kh,kw", cc.NAN_WINDOWS)
def test_maxpool_carries_the_first_nan_of_the_window(dt, kh, kw):
    csr, N = cc.nan_position_input(dt, kh, kw)
    T = kh * kw
    got = _assert_is_torch_pool(csr, 3, N, kh, kw, (kh, kw), None)
    nan_a, nan_b = (int(b) for b in _bits(cc.special(dt)[:2]))
    assert np.array_equal(np.diff(got[0]), [3] * N)       # every window keeps all three channels
    bits = _bits(got[2]).reshape(N, 3)
    assert not np.isnan(got[2].reshape(N, 3)[:, 2]).any()
    for img in range(N):
        t = img % T
        if img < T:
            assert (int(bits[img, 0]), int(bits[img, 1])) == (nan_a, nan_a), img
        else:                                            # A at tap t, B at tap (t + 1) % T: the earlier tap wins
            assert (int(bits[img, 0]), int(bits[img, 1])) == (nan_a if t < (t + 1) % T else nan_b, nan_b), img


def test_maxpool_of_nothing():
    for dt in DTYPES:
        empty = (np.zeros(2 * 4 * 6 + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))
        for C in (0, 5):
            rowptr, col, val = model.maxpool(empty, C, 2, 4, 6, 2, None)
            assert rowptr.tolist() == [0] * (2 * 2 * 3 + 1) and len(col) == 0 and val.dtype == dt


def test_coo_rows():
    (rowptr, col, _), _ = cc.rows_input(np.float32)
    rows = model.coo_rows(rowptr)
    assert rows.dtype == np.uint32 and len(rows) == len(col)
    assert all(rowptr[r] <= p < rowptr[r + 1] for p, r in enumerate(rows))
    assert len(model.coo_rows(np.zeros(5, np.int64))) == 0


# ---- planted defects: the GPU case lists against a model that is wrong the way a kernel could be --------------------------------------
def _fold_first_tap_only(v, w):
    """The fold before the rule was written down: ``w > v ? w : v`` -- a NaN off the first tap loses every comparison."""
    with np.errstate(invalid="ignore"):
        return np.where(w > v, w, v)


def _pool_cases():
    """(name, csr, C, N, H, W, kernel, stride) of every pooling case the GPU tests run, but the C = 2^20 + 1 one."""
    for dt in DTYPES:
        for kh, kw in cc.NAN_WINDOWS:
            csr, N = cc.nan_position_input(dt, kh, kw)
            yield f"nan-{kh}x{kw}-{np.dtype(dt).name}", csr, 3, N, kh, kw, (kh, kw), None
        for C in (1, 65):
            csr = cc.pool_input(dt, C)
            for kernel, stride in cc.POOL_GEOMS:
                yield f"pool-C{C}-{kernel}-{stride}-{np.dtype(dt).name}", csr, C, *cc.POOL_SHAPE, kernel, stride


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(_bits(x) if x.dtype.kind == "f" else x, _bits(y) if y.dtype.kind == "f" else y)
               for x, y in zip(a, b))


def test_planted_defect_a_nan_off_the_first_tap_is_ignored():
    caught = [name for name, csr, C, N, H, W, kernel, stride in _pool_cases()
              if _differs(model.maxpool(csr, C, N, H, W, kernel, stride), model.maxpool(csr, C, N, H, W, kernel, stride, fold=_fold_first_tap_only))]
    print(f"planted defect (a NaN off the first tap is ignored): caught by {len(caught)} cases: {caught}")
    # every NaN-position case catches it, and so does the general input wherever a window is larger than one tap
    assert {f"nan-{kh}x{kw}-{np.dtype(dt).name}" for kh, kw in cc.NAN_WINDOWS for dt in DTYPES} <= set(caught)
    assert any(name.startswith("pool-") for name in caught)
    assert not any("-1-1-" in name for name in caught)    # (a 1x1 window has no second tap: both folds agree)


def _im2col_losing_the_last_entry_of_a_chunk(N, C, H, W, coo, g):
    """A write pass whose last lane of the last wave step never stores: entry CHUNK - 1 of every full chunk of a channel."""
    ch, pix, val = model.by_channel(C, N * H * W, coo)
    start = np.concatenate([[0], np.cumsum(np.bincount(ch, minlength=C))])[ch]
    keep = (np.arange(len(ch)) - start) % model.CHUNK != model.CHUNK - 1
    return model.unfold_sorted(N, C, H, W, (ch[keep], pix[keep], val[keep]), g)


def test_planted_defect_im2col_loses_the_last_entry_of_a_chunk():
    N, C, H, W = cc.EDGE_SHAPE
    caught = []
    for dt in DTYPES:
        x = cc.edge_input(dt)
        assert np.bincount(x[1], minlength=C).tolist() == cc.EDGE_COUNTS
        for g in cc.EDGE_GEOMS:
            good, bad = model.im2col(N, C, H, W, x, g), _im2col_losing_the_last_entry_of_a_chunk(N, C, H, W, x, g)
            if _differs(good, bad):
                caught.append((np.dtype(dt).name, tuple(g)))
            # the channels below a full chunk are untouched, every channel with one loses entries
            lens_good, lens_bad = (np.diff(a[0]).reshape(C, 9).sum(1) for a in (good, bad))
            full = np.array(cc.EDGE_COUNTS) >= model.CHUNK
            assert np.array_equal(lens_good[~full], lens_bad[~full])
    print(f"planted defect (im2col loses the last entry of a chunk): caught by {len(caught)} cases: {caught}")
    # at stride 1 every stored entry reaches the output through the centre tap, so a lost entry always shows there; the
    # strided, dilated geometry keeps one pixel in four, and a lost entry on another pixel was never going to be written
    assert {(np.dtype(dt).name, tuple(cc.EDGE_GEOMS[0])) for dt in DTYPES} <= set(caught)
    # the conv2d inputs are below one chunk per channel: they cannot see it, the edge input is what does
    for g in cc.CONV_GEOMS.values():
        x, _ = cc.conv_input(np.float64, g, 1)
        assert not _differs(model.im2col(*cc.CONV_SHAPE, x, g), _im2col_losing_the_last_entry_of_a_chunk(*cc.CONV_SHAPE, x, g))
