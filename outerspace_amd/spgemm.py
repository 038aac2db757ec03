"""Host-side Python surface of the MI355X outer-product SpGEMM.

Mirrors the reference's call surface for this path:

* ``spgemm_mtx(a, b)``            -- ``./simulator A.mtx B.mtx`` (``simulator/SimSpGEMM.cpp:819-894``):
  two MatrixMarket files in, the second operand transposed by default (``:852-856``), CSR out.
* ``spgemm_csc_csr(...)``         -- ``cscMulcsr(csc, csr)`` + sort/sum (``:265-281``, ``:519-535``).
* ``spgemm(A, B, transpose_b)``   -- the entry point SURVEY.md section 0 places beside
  ``NN_models/sparse_util.py``: dense/scipy operands as ``get_mtx_files.py`` dumps them
  (activation ``batch x in``, ``nn.Linear`` weight ``out x in``) -> ``act @ W.T`` as scipy CSR.
* ``read_mtx`` / ``coo_to_csr`` / ``coo_to_csc`` -- ``readcoo`` (``:55-100``), ``coo2csr`` (``:102-152``).

All numeric work happens in ``libouterspace_spgemm.so`` on the GPU; nothing here computes.
"""
import ctypes as C
import math
import os
import weakref

import numpy as np

from . import _lib
from ._lib import OspError  # noqa: F401  (re-export)

_DT = {np.dtype(np.float32): _lib.OSP_F32, np.dtype(np.float64): _lib.OSP_F64}


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a.size else 0)


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


# ---- argument helpers the methods below share ------------------------------------------------------------
def _enum(table, value, what):
    """``table[value]``, or the ValueError of a name the table does not hold."""
    if value not in table:
        raise ValueError(f"{what} must be one of {' '.join(table)} (got {value!r})")
    return table[value]


def _space(space):
    """``OSP_HOST`` / ``OSP_DEVICE`` of a ``space`` argument."""
    if space not in ("device", "host"):
        raise ValueError('space must be "device" or "host"')
    return _lib.OSP_HOST if space == "host" else _lib.OSP_DEVICE


def _dptrs(ptrs, null=False):
    """Addresses (ints) as pointer arguments; ``null=True`` passes a zero or absent address as NULL."""
    return [None if null and not p else C.c_void_p(int(p)) for p in ptrs]


def _torch_dtype(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _call(ctx, name, *args, stats=None, keep=()):
    """The frame of every entry point that makes a result: ``name(*args, &handle[, &stats])``, ``_lib.check``, the handle
    wrapped as a ``CsrResult`` of ``ctx``.  Returns the result, or (result, stats dict) when a stats struct is passed.
    ``keep`` holds the objects the addresses in ``args`` point into: it is an argument so that they outlive the call."""
    h = C.c_void_p()
    tail = (C.byref(h),) if stats is None else (C.byref(h), C.byref(stats))
    _lib.check(getattr(_lib.lib(), name)(*args, *tail))
    res = CsrResult(ctx, h)
    return res if stats is None else (res, stats.as_dict())


def _dense_arg(v, shape, dtype, space, what, floating=False):
    """A dense argument of the ``osp_csr_*`` functions that take one -- a vector ``(n,)`` or a row-major matrix ``(rows, k)``
    -- as (pointer, keep-alive); the pointer is never null.  ``space="host"``: an array-like of that shape, converted to
    ``dtype``; ``space="device"``: a device address, which carries no shape (the caller vouches for it), or an object with
    ``data_ptr()`` (a contiguous torch tensor of ``dtype``, floating point when ``floating``: the caller has synchronised
    its stream)."""
    if v is None:
        return None, None
    vector, size = len(shape) == 1, math.prod(shape)
    if space == "host" or (vector and size == 0):   # (an empty vector on the device: nothing is read, v is not looked at)
        a = np.ascontiguousarray(v, dtype) if space == "host" else np.zeros(0, dtype)
        if a.shape != shape:
            raise OspError(_lib.ERR_ARG, f"{what} must have {size} entries (got shape {a.shape})" if vector else
                           f"{what} must have shape ({shape[0]}, {shape[1]}) (got {a.shape})")
        a = a if a.size else np.zeros(1, dtype)   # (never a null pointer)
        return C.c_void_p(a.ctypes.data), a
    if hasattr(v, "data_ptr"):
        fits = v.numel() == size if vector else tuple(v.shape) == shape
        if not fits or v.element_size() != np.dtype(dtype).itemsize or (floating and not v.is_floating_point()) or not v.is_contiguous():
            raise OspError(_lib.ERR_ARG, f"{what} must be a contiguous tensor of {size} values of {np.dtype(dtype)}" if vector else
                           f"{what} must be a contiguous ({shape[0]}, {shape[1]}) tensor of {np.dtype(dtype)}")
        if size == 0:
            a = np.zeros(1, dtype)
            return C.c_void_p(a.ctypes.data), a
        return C.c_void_p(v.data_ptr()), v
    return C.c_void_p(int(v)), None


def _u32_list(v, space, what):
    """An index list of ``extract`` and ``build``: (address, count, keep-alive); the address of an empty list is 0, and what
    that says is the caller's convention.  ``space="host"``: an array-like of integers in [0, 2^32); ``space="device"``: a
    torch tensor of 4-byte integers (the caller has synchronised its stream) or an ``(address, count)`` pair."""
    if space == "host":
        a = np.atleast_1d(np.asarray(v))
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise OspError(_lib.ERR_ARG, f"{what} must be a one-dimensional list of integers")
        a = a.astype(np.int64) if a.size else np.zeros(0, np.int64)
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise OspError(_lib.ERR_ARG, f"{what} holds an index outside [0, 2^32)")
        a = np.ascontiguousarray(a, np.uint32)
        return (a.ctypes.data if a.size else 0), int(a.size), a
    if hasattr(v, "data_ptr"):
        if v.dim() != 1 or v.element_size() != 4 or v.is_floating_point() or not v.is_contiguous():
            raise OspError(_lib.ERR_ARG, f"{what} must be a contiguous one-dimensional tensor of 4-byte integers")
        return (v.data_ptr() if v.numel() else 0), int(v.numel()), v
    return int(v[0]), int(v[1]), None


def _index_arg(v, space, what):
    """An index list of ``extract``: (pointer, count, keep-alive, ascending).  None takes every row / column (a null
    pointer), so an empty list never passes one.  ``ascending`` says whether the list is strictly ascending -- numpy on the
    host, one torch comparison on the device -- and is None for a bare address, which nothing here can read."""
    if v is None:
        return None, 0, None, True
    addr, n, keep = _u32_list(v, space, what)
    if n == 0:   # (nothing is read: any non-null pointer says "an empty list")
        keep = np.zeros(1, np.uint32)
        return C.c_void_p(keep.ctypes.data), 0, keep, True
    if keep is None:
        return C.c_void_p(addr), n, None, None
    w = keep if space == "host" else keep.long() & 0xffffffff   # (an int32 tensor holds a uint32 list's bits)
    return C.c_void_p(addr), n, keep, bool((w[1:] > w[:-1]).all())


def conv2d_geometry(kernel_size, stride=1, padding=0, dilation=1):
    """``osp_conv2d_geometry_t`` from torch-style arguments (an int or an (h, w) pair each)."""
    g = _lib.Conv2dGeometry()
    g.kh, g.kw = _pair(kernel_size)
    g.stride_h, g.stride_w = _pair(stride)
    g.pad_h, g.pad_w = _pair(padding)
    g.dil_h, g.dil_w = _pair(dilation)
    return g


def conv2d_output_size(size, kernel, stride=1, padding=0, dilation=1):
    """Output extent of one axis: ``(size + 2*padding - dilation*(kernel - 1) - 1) // stride + 1`` (torch.nn.Conv2d's
    formula, floor mode); 0 when the dilated kernel does not fit the padded input."""
    span = size + 2 * padding - dilation * (kernel - 1) - 1
    return span // stride + 1 if span >= 0 else 0


class CsrResult:
    """Library-owned CSR result.  ``rowptr``/``colidx``/``vals`` copy to the host on first use."""

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle
        ctx._results.add(self)  # a context closes its results before it goes away
        info = _lib.ResultInfo()
        _lib.check(_lib.lib().osp_result_info(handle, C.byref(info)))
        self.info = info.as_dict()
        self.shape = (info.M, info.N)
        self.nnz = info.nnz_c
        self.dtype = np.float32 if info.dtype == _lib.OSP_F32 else np.float64
        self._host = None

    def to_host(self):
        if self._host is None:
            rowptr = np.empty(self.shape[0] + 1, np.int64)
            colidx = np.empty(self.nnz, np.uint32)
            vals = np.empty(self.nnz, self.dtype)
            _lib.check(_lib.lib().osp_result_copy_csr(self._h, _ptr(rowptr), _ptr(colidx), _ptr(vals), _lib.OSP_HOST))
            self._host = (rowptr, colidx, vals)
        return self._host

    rowptr = property(lambda self: self.to_host()[0])
    colidx = property(lambda self: self.to_host()[1])
    vals = property(lambda self: self.to_host()[2])

    def partials_ptrs(self):
        """Result of ``spgemm_partials_device``: (rowptr, records) device addresses -- int64 record offsets per row, packed
        ``{u32 col; T val}`` records -- valid until ``close()``."""
        r, rec = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().osp_result_partials(self._h, C.byref(r), C.byref(rec)))
        return r.value or 0, rec.value or 0

    def device_ptrs(self):
        """(rowptr, colidx, vals) device addresses, valid until ``close()``."""
        r, c, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().osp_result_device_ptrs(self._h, C.byref(r), C.byref(c), C.byref(v)))
        return r.value or 0, c.value or 0, v.value or 0

    def bias_relu(self, bias=None, relu=True):
        """``relu(C + bias)`` with the zeros dropped, as a new CSR result on the device (``osp_csr_bias_relu``): what
        ``models.py:17-31`` does between two layers.  bias: N values (numpy, C's dtype) or None."""
        b = None if bias is None else np.ascontiguousarray(bias, self.dtype)
        if b is not None and b.shape != (self.shape[1],):
            raise ValueError(f"bias must have {self.shape[1]} entries")
        return _call(self._ctx, "osp_csr_bias_relu", self._h, _ptr(b) if b is not None else None, _lib.OSP_HOST, int(bool(relu)), keep=b)

    def maxpool2d(self, N, H, W, kernel_size, stride=None):
        """MaxPool2d of this CSR read as a "pixel x channel" activation of N images of H x W pixels (row n*H*W + y*W + x):
        a new (N*PH*PW) x C CSR result on the device (``osp_csr_maxpool2d``).  An absent entry counts as 0 and zeros are
        dropped, so it equals ``F.max_pool2d`` on the densified input.  No padding, no dilation, floor mode; stride
        defaults to the kernel size, as in torch.

        The rule: a window that holds a NaN gives a NaN wherever in the window it lies (as torch does); the entry is kept
        (``NaN != 0``) and, values being copied and never recomputed, carries the bits of the window's first NaN in tap
        order (``ky`` outer, ``kx`` inner).  Otherwise the entry is the window's maximum with an absent tap counting as
        +0: a window whose maximum is a zero of either sign is dropped, and an all-present, all-negative window keeps its
        negative maximum."""
        kh, kw = _pair(kernel_size)
        sh, sw = _pair(kernel_size if stride is None else stride)
        return _call(self._ctx, "osp_csr_maxpool2d", self._h, int(N), int(H), int(W), kh, kw, sh, sw)

    def inflate_prune(self, power=2.0, threshold=0.0, max_per_row=0, validate=False):
        """One Markov-clustering step on this CSR, row by row, as a new CSR result on the device
        (``osp_csr_inflate_prune``): keep the entries ``>= threshold`` (a row that keeps nothing keeps its largest), of
        those at most the ``max_per_row`` largest (0: no cap; ties to the lower column), raise them to ``power`` and
        divide by the row's sum.  Returns (result, stats dict): nnz_in, nnz_out, rows_capped, rows_rescued, rows_long,
        chaos, ms_total, ms_select_kernel, launches.  validate=True refuses negative, NaN and infinite values."""
        step = _lib.MclStep()
        step.power, step.threshold, step.max_per_row = float(power), float(threshold), int(max_per_row)
        return _call(self._ctx, "osp_csr_inflate_prune", self._h, C.byref(step), int(bool(validate)), stats=_lib.MclStats())

    def apply_mask(self, mask, *, complement=False, validate=False, space="device"):
        """The entries of this CSR that are in ``mask`` (``complement=True``: that are NOT in it) as a new CSR result on the
        device (``osp_csr_apply_mask``); values keep their bits.  ``mask`` is a CSR pattern of this result's shape:
        ``(rowptr, colidx)`` as device addresses (``space="device"``) or numpy arrays (``space="host"``), or another
        ``CsrResult`` (its pattern, on the device).  Returns (result, stats dict): nnz_in, nnz_mask, nnz_out, ms_total,
        launches.  validate=True checks the mask as ``spgemm_masked`` does."""
        M, N = self.shape
        if isinstance(mask, CsrResult):
            if mask.shape != self.shape:
                raise OspError(_lib.ERR_ARG, f"the mask's shape {mask.shape} differs from the result's {self.shape}")
            rp, ci = (C.c_void_p(p) for p in mask.device_ptrs()[:2])
            sp_, keep = _lib.OSP_DEVICE, None
        elif space == "host":
            r, c = np.ascontiguousarray(mask[0], np.int64), np.ascontiguousarray(mask[1], np.uint32)
            if len(r) != M + 1:
                raise OspError(_lib.ERR_ARG, f"the mask's row pointers must have M+1={M + 1} entries (got {len(r)})")
            rp, ci, sp_, keep = C.c_void_p(r.ctypes.data), _ptr(c), _lib.OSP_HOST, (r, c)
        elif space == "device":
            rp, ci, sp_, keep = C.c_void_p(int(mask[0])), C.c_void_p(int(mask[1])), _lib.OSP_DEVICE, None
        else:
            raise ValueError('space must be "device" or "host"')
        return _call(self._ctx, "osp_csr_apply_mask", self._h, M, N, rp, ci, sp_, int(bool(complement)), int(bool(validate)),
                     stats=_lib.ApplyMaskStats(), keep=keep)

    def select(self, op, threshold=0.0, *, diag=0, fill=None):
        """The entries of this CSR that pass a predicate as a new CSR result on the device (``osp_csr_select``).  ``op`` is
        ``"lt" "le" "gt" "ge" "eq" "ne"`` -- value ``op`` ``threshold``, compared as doubles under IEEE rules (a NaN passes
        ``"ne"`` only) -- or ``"tril" "triu" "diag" "offdiag"`` -- column ``<=``, ``>=``, ``==``, ``!=`` row + ``diag``.
        ``fill=None``: kept entries keep their value bits; otherwise every kept entry's value is ``fill``.  Returns
        (result, stats dict): nnz_in, nnz_out, ms_total, launches."""
        sel = _lib.Select()
        sel.op, sel.threshold, sel.diag = _enum(_lib.SELECT_OPS, op, "op"), float(threshold), int(diag)
        if fill is not None:
            sel.fill, sel.fill_value = 1, float(fill)
        return _call(self._ctx, "osp_csr_select", self._h, C.byref(sel), stats=_lib.SelectStats())

    def _same_family(self, other, *, shape=False, context=True):
        """The checks of a second operand: a ``CsrResult``, of this result's context, shape (``shape=True``) and dtype."""
        if not isinstance(other, CsrResult):
            raise TypeError("other must be a CsrResult")
        if context and other._ctx is not self._ctx:
            raise OspError(_lib.ERR_ARG, "the operands belong to different contexts")
        if shape and other.shape != self.shape:
            raise OspError(_lib.ERR_ARG, f"the operands' shapes differ: {self.shape} and {other.shape}")
        if other.dtype != self.dtype:
            raise OspError(_lib.ERR_ARG, f"the operands' dtypes differ: {np.dtype(self.dtype)} and {np.dtype(other.dtype)}")

    def ewise(self, other, mode, op):
        """This CSR combined with ``other`` entry by entry as a new CSR result on the device (``osp_csr_ewise``); nothing is
        sorted.  ``mode`` ``"union"``: the pattern is the union, a coordinate in both gets ``op(self, other)``, one in a
        single operand keeps that operand's value bits.  ``mode`` ``"intersect"``: the common pattern, every value
        ``op(self, other)``.  ``op`` is ``"plus" "times" "min" "max" "first" "second"``, and for an intersection also
        ``"minus" "div"``: one IEEE operation in the results' dtype.  ``other`` is a ``CsrResult`` of the same context, shape
        and dtype (``self`` itself is allowed).  Returns (result, stats dict): nnz_a, nnz_b, nnz_both, nnz_out, ms_total,
        launches."""
        ew = _lib.Ewise()
        ew.mode, ew.op = _enum(_lib.EWISE_MODES, mode, "mode"), _enum(_lib.EWISE_OPS, op, "op")
        self._same_family(other, shape=True, context=False)   # (the context is not checked here: the library refuses a foreign operand)
        return _call(self._ctx, "osp_csr_ewise", self._h, other._h, C.byref(ew), stats=_lib.EwiseStats())

    def union(self, other, op="plus"):
        """``ewise(other, "union", op)``: the accumulation ``self (+) other``."""
        return self.ewise(other, "union", op)

    def intersect(self, other, op="times"):
        """``ewise(other, "intersect", op)``: ``op`` on the common pattern."""
        return self.ewise(other, "intersect", op)

    def mxm(self, other, add="plus", mul="times", *, mask=None, complement=False):
        """This CSR (M x K) times ``other`` (K x N) under the semiring ``(add, mul)`` as a new M x N CSR result on the device
        (``osp_csr_mxm``): a row-wise product of two results, nothing is ingested or transposed.  An output entry (i, j)
        exists when some k has a stored ``self[i, k]`` and a stored ``other[k, j]``; its value is the products
        ``mul(self[i, k], other[k, j])`` folded with ``add`` left to right in ascending k, starting AS the first product.
        ``add`` is ``"plus" "min" "max" "first"``, ``mul`` is ``"times" "plus" "min" "max" "first" "second"``: one IEEE
        operation each, as ``ewise`` defines them.  ``("plus", "times")`` equals ``spgemm_coo_device`` of the same operands
        bit for bit; ``("min", "plus")`` relaxes a frontier of distances.  ``other`` is a ``CsrResult`` of the same context and
        dtype (``self`` itself is allowed).  Returns (result, stats dict): nnz_a, nnz_b, products, nnz_out, short_rows,
        long_rows, batches, launches, ms_total.

        ``mask`` (a ``CsrResult`` of shape (M, N) on the same context; only its pattern is read, its dtype is free; ``self``
        and ``other`` are allowed) computes the product AT the mask (``osp_csr_mxm_masked``): the entries whose coordinate the
        mask holds, or with ``complement=True`` does not hold -- the same three arrays, bit for bit, as
        ``self.mxm(other, add, mul)[0].apply_mask(mask, complement=complement)``, but a product the mask rejects is dropped
        where it is formed and is neither sorted, folded nor written.  The stats dict is then nnz_a, nnz_b, nnz_mask,
        products (formed), products_kept, nnz_out, short_rows, long_rows, batches, launches, ms_total.
        ``complement=True`` without a mask is a ValueError.  When it pays (MEASUREMENTS.md section 0w, MI355X, 64-source BFS
        on R-MAT scale 16 and 19): the fused call costs a bisection per formed product and saves the sort, the fold and the
        write of every rejected one.  With a third of the products kept it takes 0.14 to 0.24 of the two calls' time, with
        a few per cent kept 0.06 to 0.27, ``(A A)<A>`` (nearly all rows long, 4 to 8 % kept) 0.52; the break-even is
        "nearly everything kept" (0.99 kept: 0.92 to 0.98, level within the spread), and no measured case was slower."""
        sr = _lib.Semiring()
        sr.add, sr.mul = _enum(_lib.MXM_ADD_OPS, add, "add"), _enum(_lib.MXM_MUL_OPS, mul, "mul")
        if mask is None and complement:
            raise ValueError("complement=True needs a mask")
        self._same_family(other)
        if mask is None:
            return _call(self._ctx, "osp_csr_mxm", self._h, other._h, C.byref(sr), stats=_lib.MxmStats())
        if not isinstance(mask, CsrResult):
            raise TypeError("mask must be a CsrResult")
        if mask._ctx is not self._ctx:
            raise OspError(_lib.ERR_ARG, "the mask belongs to a different context")
        return _call(self._ctx, "osp_csr_mxm_masked", self._h, other._h, mask._h, int(bool(complement)), C.byref(sr),
                     stats=_lib.MxmMaskedStats())

    def kron(self, other, op="times"):
        """The Kronecker product ``self (x) other`` as a new CSR result on the device (``osp_csr_kron``): with this result
        ``mA x nA`` and ``other`` ``mB x nB`` it is ``(mA mB) x (nA nB)`` and holds ``op(self[ia, ja], other[ib, jb])`` at
        ``(ia mB + ib, ja nB + jb)`` for every pair of stored entries, this result's value first.  ``op`` is ``"times" "plus"
        "min" "max" "first" "second"``: one IEEE operation in the results' dtype or a copy of one operand's bits, as ``ewise``
        defines them.  The product is structural (an explicit zero makes entries).  Its whole structure is closed form:
        nothing is sorted, scanned or read back, and the only allocations are the result's arrays.  ``other`` is a
        ``CsrResult`` of the same context and dtype (``self`` itself is allowed).  A product of 2^32 - 1 entries or more is
        ``OspError(ERR_CAPACITY)``, a shape beyond a result's limits ``OspError(ERR_ARG)``.  Returns (result, stats dict):
        nnz_a, nnz_b, nnz_out, ms_total, launches, readbacks."""
        kr = _lib.Kron()
        kr.op = _enum(_lib.KRON_OPS, op, "op")
        self._same_family(other)
        return _call(self._ctx, "osp_csr_kron", self._h, other._h, C.byref(kr), stats=_lib.KronStats())

    def select_k(self, k, order="largest", *, seed=0):
        """Of every row of this CSR the ``k`` entries that rank first under ``order``, as a new CSR result on the device
        (``osp_csr_select_k``): a row of at most ``k`` entries is kept whole.  ``order`` ``"largest"`` / ``"smallest"``: by
        value under IEEE comparison, -0.0 equal to +0.0, every NaN after every number, ties to the lower column (the tie
        rule of ``inflate_prune``'s ``max_per_row``).  ``"random"``: by a 64-bit hash of (``seed``, row, column) -- values are
        not read, no two entries tie, and a row's choice depends on the seed, the row's number and its columns alone; over
        seeds every k-subset of a row is equally likely.  Kept entries keep their value bits and columns stay ascending.
        Selecting with ``k`` and then with ``k2 <= k`` (same order and seed) equals selecting with ``k2``.  ``k`` is an int
        in [1, 2^32 - 1], ``seed`` an int in [0, 2^64): anything else is a ValueError.  Returns (result, stats dict):
        nnz_in, nnz_out, rows_capped, rows_long, ms_total, launches, readbacks."""
        sk = _lib.SelectK()
        sk.order = _enum(_lib.SELECT_K_ORDERS, order, "order")
        for name, v, lo, hi in (("k", k, 1, 0xffffffff), ("seed", seed, 0, 0xffffffffffffffff)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}] (got {v!r})")
        sk.k, sk.seed = int(k), int(seed)
        return _call(self._ctx, "osp_csr_select_k", self._h, C.byref(sk), stats=_lib.SelectKStats())

    def scan(self, op="plus"):
        """The inclusive scan of every row of this CSR under ``op`` (``"plus"``, ``"min"``, ``"max"``: a running sum,
        minimum or maximum along ascending columns), as a new CSR result with this pattern on the device
        (``osp_csr_scan``).  The order is defined to the bit: a row is cut into blocks of 32 entries, scanned
        sequentially inside (from ``reduce``'s identity), the blocks' totals are scanned sequentially across the row, and an
        entry's value is (carry into its block) ``op`` (its local scan).  A row of at most 32 entries is ``numpy.cumsum``
        in the dtype, except that a leading -0.0 reads +0.0; min and max never take a NaN (the identity until a number
        arrives); plus propagates one to the end of its row; on non-negative input the running sum never decreases, and a
        zero entry beyond the first repeats the value before it bit for bit.  A row's scan depends on its values alone.
        Nothing is read back.  Returns (result, stats dict): nnz_in, nnz_out, blocks (nnz // 32 + M: the bound the
        kernels are launched for), ms_total, launches, readbacks (0)."""
        sc = _lib.Scan()
        sc.op = _enum(_lib.SCAN_OPS, op, "op")
        return _call(self._ctx, "osp_csr_scan", self._h, C.byref(sc), stats=_lib.ScanStats())

    def draw(self, draws=1, *, seed=0, out=None, out_pos=None, positions=False, space="device"):
        """``draws`` weighted draws from every row of this CSR, with replacement (``osp_csr_draw``): row i's draw d picks an
        entry with probability (its weight) / (the row's total weight) and returns its column; an entry's weight is its
        value where that is positive and finite, and 0 otherwise (zeros, negatives, NaNs and infinities are never drawn).
        The CDF is ``scan("plus")`` of the weights to the bit, the random number a 64-bit hash of (``seed``, i, d) -- the
        draw is the first entry whose running sum exceeds (hash as a fraction in [0, 1)) * total -- so for a fixed seed a
        row's draws depend on the row's number and values alone.  A row that is empty, has no positive finite weight or whose
        total overflows gives -1.  ``draws`` is an int in [1, 2^32 - 1], ``seed`` an int in [0, 2^64): anything else is a
        ValueError.  ``out`` / ``out_pos``: None, or (M, draws) int64 values to fill -- a device address or torch tensor, a
        numpy array with ``space="host"``; ``positions=True`` (or an ``out_pos``) also returns every picked entry's index in
        this result's arrays.  Returns (cols, stats dict) or (cols, pos, stats dict): torch int64 tensors (M, draws) on
        the context's device, or numpy arrays (``space="host"``).  Stats: nnz_in, nnz_out (M * draws), rows_without,
        ms_total, launches, readbacks (1: rows_without)."""
        for name, v, lo, hi in (("draws", draws, 1, 0xffffffff), ("seed", seed, 0, 0xffffffffffffffff)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}] (got {v!r})")
        sp = _space(space)
        dr = _lib.Draw()
        dr.draws, dr.seed = int(draws), int(seed)
        M = self.shape[0]
        if M * int(draws) > 1 << 40:
            raise OspError(_lib.ERR_ARG, "M * draws must be at most 2^40")
        positions = positions or out_pos is not None
        cp, cbuf, cret = self._out_arg(out, (M, int(draws)), space, np.int64, "out")
        pp, pbuf, pret = self._out_arg(out_pos, (M, int(draws)), space, np.int64, "out_pos") if positions else (None, None, None)
        stats = _lib.DrawStats()
        _lib.check(_lib.lib().osp_csr_draw(self._h, C.byref(dr), cp, pp, sp, C.byref(stats)))   # (cbuf and pbuf live until here)
        return (cret, pret, stats.as_dict()) if positions else (cret, stats.as_dict())

    def transpose(self):
        """This CSR (M x N) transposed as a new N x M CSR result on the device (``osp_csr_transpose``): entry (j, i) exists
        iff this result has (i, j), columns ascend in every row, values keep their bits, and transposing twice gives the same
        three arrays back.  A result of at most 64 rows takes the row-mask path (nothing is sorted), everything else a
        stable radix sort by column.  A non-empty result of 2^32 - 256 columns and more is ``OspError(ERR_ARG)``: the new N + 1 row
        pointers take a thread each.  Returns (result, stats dict): nnz, path (0 nothing launched, 1 row mask, 2 sort),
        passes, launches, ms_total."""
        return _call(self._ctx, "osp_csr_transpose", self._h, None, stats=_lib.TransposeStats())

    def matmul(self, other, *, self_transposed=False, validate=False, partial_capacity=0):
        """This CSR (M x K) times ``other`` (K x N) with + and x through the outer-product pipeline
        (``osp_spgemm_csc_csr``), as a new M x N CSR result: this result is transposed on the device -- the CSR arrays of the
        transpose ARE this result's CSC arrays, which the pipeline takes for its left operand -- and the temporary is closed.
        ``self_transposed=True`` computes ``self^T @ other`` instead (self K x M), with no transpose at all: self's own CSR
        arrays are the CSC of ``self^T``.  Equals ``mxm(other, "plus", "times")`` in row pointers, columns and value bits.
        ``other`` is a ``CsrResult`` of the same context and dtype (``self`` itself is allowed)."""
        self._same_family(other)
        M, K = (self.shape[1], self.shape[0]) if self_transposed else self.shape
        if K != other.shape[0]:
            raise OspError(_lib.ERR_DIM, f"the inner dimensions differ: {K} and {other.shape[0]}")
        at = self if self_transposed else self.transpose()[0]
        try:
            return self._ctx.spgemm_csc_csr_device(self.dtype, M, K, other.shape[1], (*at.device_ptrs(), *other.device_ptrs()),
                                                   validate=validate, partial_capacity=partial_capacity)
        finally:
            if at is not self:
                at.close()

    def _out_arg(self, out, shape, space, dtype=None, what="out"):
        """The output of ``mxv`` (``shape`` (M,)) and ``mxd`` ((M, k)), and with ``dtype=np.int64`` the positions of
        ``mxv_arg`` and the (M, draws) columns and positions of ``draw`` (the one 2-D output that is not floating point):
        (pointer, buffer the pointer points into, what the method returns).  ``out=None`` allocates -- numpy on
        the host, torch on the context's device --, else ``out`` is checked and filled.  The pointer is never null."""
        size = math.prod(shape)
        dtype = self.dtype if dtype is None else dtype
        if out is None and space == "host":
            ret = np.empty(shape, dtype)
            buf = ret if size else np.empty(1, dtype)
            return C.c_void_p(buf.ctypes.data), buf, ret
        if out is None:
            import torch
            tdt = torch.int64 if np.dtype(dtype) == np.int64 else _torch_dtype(dtype)
            buf = torch.empty(max(size, 1), dtype=tdt, device=f"cuda:{self._ctx.device}")
            return C.c_void_p(buf.data_ptr()), buf, buf[:size].view(shape)
        if space == "host":
            if not (isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == shape and out.flags.c_contiguous):
                raise OspError(_lib.ERR_ARG, f"{what} must be a contiguous numpy array of {size} values of {np.dtype(dtype)}" if len(shape) == 1
                               else f"{what} must be a contiguous ({shape[0]}, {shape[1]}) numpy array of {np.dtype(dtype)}")
            buf = out if size else np.empty(1, dtype)
            return C.c_void_p(buf.ctypes.data), buf, out
        if np.dtype(dtype) == np.int64 and hasattr(out, "is_floating_point") and out.is_floating_point():
            raise OspError(_lib.ERR_ARG, f"{what} must be a contiguous tensor of {size} values of int64")
        ptr, buf = _dense_arg(out, shape, dtype, "device", what, floating=len(shape) == 2 and np.dtype(dtype) != np.int64)
        return ptr, buf, out

    def reduce(self, axis, op, out=None):
        """One value per row (``axis="rows"``, M values) or per column (``"cols"``, N values) of this CSR
        (``osp_csr_reduce``): ``op`` ``"plus"``, ``"min"``, ``"max"`` or ``"count"``, in this result's dtype, in an order that
        is defined to the bit and depends on the segment's length alone.  An empty row gives +0.0,
        +inf, -inf, 0.  ``out=None``: returns (numpy array on the host, stats dict); ``out`` a device address (or a torch
        tensor of that many values of this dtype): fills it and returns (out, stats dict).  Stats: nnz_in, nnz_out,
        long_segments, ms_total, launches."""
        ax, rop = _enum(_lib.AXES, axis, "axis"), _enum(_lib.REDUCE_OPS, op, "op")
        n = self.shape[ax]
        stats = _lib.VectorStats()
        if out is None:
            buf = np.empty(max(n, 1), self.dtype)   # (never a null pointer)
            ptr, space, ret = C.c_void_p(buf.ctypes.data), _lib.OSP_HOST, buf[:n]
        else:
            ptr, buf = _dense_arg(out, (n,), self.dtype, "device", "out")
            space, ret = _lib.OSP_DEVICE, out
        _lib.check(_lib.lib().osp_csr_reduce(self._h, ax, rop, ptr, space, C.byref(stats)))
        return ret, stats.as_dict()

    def mxv(self, x, add="plus", mul="times", out=None, space="device"):
        """This CSR (M x N) times the dense vector ``x`` (N values) under the semiring ``(add, mul)`` (``osp_csr_mxv``):
        ``y[i]`` is the reduction, in ``reduce``'s bit-defined order, of ``mul(self[i, j], x[j])`` over row i's entries, in
        one fused pass -- equal in bits to ``apply_vectors(cols=x, col_op=mul)`` followed by ``reduce("rows", add)``.  ``add``
        is ``"plus" "min" "max"``, ``mul`` is ``"times" "plus" "min" "max" "first" "second"``; ``"first"`` reads no ``x``
        (which may be None), ``"second"`` no value of this result.  An empty row gives +0.0, +inf, -inf.  ``x``: a device
        address / torch tensor (``space="device"``) or an array-like (``space="host"``).  ``out=None``: returns (torch
        tensor on the context's device, stats dict), or (numpy array, stats dict) with ``space="host"``; ``out`` a device
        address or torch tensor of M values (a numpy array of this dtype with ``space="host"``): fills and returns it.
        ``out is x`` is allowed on a square result.  Stats: nnz_in, nnz_out, long_segments, group, launches, ms_total."""
        sr = _lib.Semiring()
        sr.add, sr.mul = _enum(_lib.MXV_ADD_OPS, add, "add"), _enum(_lib.MXM_MUL_OPS, mul, "mul")
        sp = _space(space)
        M, N = self.shape
        if x is None and mul != "first":
            raise OspError(_lib.ERR_ARG, 'x may be None only when mul is "first"')
        xp, keep_x = _dense_arg(x if mul != "first" else None, (N,), self.dtype, space, "x")
        yp, buf, ret = self._out_arg(out, (M,), space)
        stats = _lib.MxvStats()
        _lib.check(_lib.lib().osp_csr_mxv(self._h, C.byref(sr), xp, yp, sp, C.byref(stats)))   # (keep_x and buf live until here)
        return ret, stats.as_dict()

    def mxv_arg(self, x, add="min", mul="times", out=None, out_arg=None, space="device", values=True):
        """``mxv`` under ``add`` ``"min"`` or ``"max"`` together with WHERE the winner is (``osp_csr_mxv_arg``): ``y`` is
        ``mxv(x, add, mul)`` bit for bit, and ``arg[i]`` is the smallest column j among row i's products
        ``mul(self[i, j], x[j])`` that are not NaN and that no other non-NaN product beats under the IEEE comparison (so
        -0.0 and +0.0 tie, and the tie goes to the smaller column); -1 for a row that is empty or whose products are all NaN.
        ``arg`` depends neither on the order of the reduction nor on ``OSP_MXV_GROUP``.  ``mul`` is ``"times" "plus" "min"
        "max" "first" "second"``; with ``"first"`` ``x`` may be None and the call is the arg-reduce of this result's rows.
        ``x``, ``out`` and ``space`` as in ``mxv``; ``out_arg``: None, or M int64 values to fill -- a device address or torch
        tensor, a numpy array with ``space="host"``; ``values=False`` asks for positions only (``out`` must be None).  For the
        column axis, ``transpose()`` first.  Returns (y or None, arg, stats dict): ``arg`` is a torch int64 tensor on the
        context's device or a numpy int64 array (``space="host"``).  Stats: nnz_in, nnz_out, long_segments, rows_without
        (rows whose arg is -1), group, launches, ms_total."""
        sr = _lib.Semiring()
        sr.add, sr.mul = _enum(_lib.MXV_ARG_ADD_OPS, add, "add"), _enum(_lib.MXM_MUL_OPS, mul, "mul")
        sp = _space(space)
        M, N = self.shape
        if x is None and mul != "first":
            raise OspError(_lib.ERR_ARG, 'x may be None only when mul is "first"')
        if not values and out is not None:
            raise OspError(_lib.ERR_ARG, "values=False returns no y: out must be None")
        xp, keep_x = _dense_arg(x if mul != "first" else None, (N,), self.dtype, space, "x")
        yp, buf, ret = self._out_arg(out, (M,), space) if values else (None, None, None)
        ap, abuf, aret = self._out_arg(out_arg, (M,), space, np.int64, "out_arg")
        stats = _lib.MxvArgStats()
        _lib.check(_lib.lib().osp_csr_mxv_arg(self._h, C.byref(sr), xp, yp, ap, sp, C.byref(stats)))   # (keep_x, buf and abuf live until here)
        return ret, aret, stats.as_dict()

    def mxd(self, X, add="plus", mul="times", out=None, space="device", k=None):
        """This CSR (M x N) times the dense matrix ``X`` (N x k, row-major, contiguous) under the semiring ``(add, mul)``
        (``osp_csr_mxd``): column c of the M x k result equals ``mxv(X[:, c], add, mul)`` BIT FOR BIT, in one pass over this
        result per 64 columns instead of k.  ``add`` is ``"plus" "min" "max"``, ``mul`` is ``"times" "plus" "min" "max"
        "first" "second"``; ``"first"`` reads no ``X`` (which may be None: then ``k`` names the number of columns),
        ``"second"`` no value of this result.  An empty row gives +0.0, +inf, -inf.  ``X``: a 2-D torch tensor or a device
        address (``space="device"``; an address carries no shape, so ``k`` is needed) or an array-like (``space="host"``).
        ``out=None``: returns (torch tensor (M, k) on the context's device, stats dict), or (numpy array, stats dict) with
        ``space="host"``; ``out`` a device address or torch tensor of shape (M, k) (a numpy array of this dtype with
        ``space="host"``): fills and returns it.  ``out is X`` is allowed on a square result.  Stats: nnz_in, nnz_out, cols,
        long_segments, lanes_per_row, launches, ms_total."""
        sr = _lib.Semiring()
        sr.add, sr.mul = _enum(_lib.MXV_ADD_OPS, add, "add"), _enum(_lib.MXM_MUL_OPS, mul, "mul")
        sp = _space(space)
        M, N = self.shape
        if X is None and mul != "first":
            raise OspError(_lib.ERR_ARG, 'X may be None only when mul is "first"')
        if k is None:
            shape = None if X is None else tuple(X.shape) if hasattr(X, "shape") else np.shape(X) if space == "host" else None
            if shape is None or len(shape) != 2:
                raise OspError(_lib.ERR_ARG, "X must be 2-D (N x k); with X None or a device address, pass k")
            k = shape[1]
        k = int(k)
        if not 0 <= k <= _lib.MXD_MAX_COLS:
            raise OspError(_lib.ERR_ARG, f"k must lie in [0, {_lib.MXD_MAX_COLS}] (got {k})")
        xp, keep_x = _dense_arg(X if mul != "first" else None, (N, k), self.dtype, space, "X", floating=True)
        yp, buf, ret = self._out_arg(out, (M, k), space)
        stats = _lib.MxdStats()
        _lib.check(_lib.lib().osp_csr_mxd(self._h, C.byref(sr), xp, k, yp, sp, C.byref(stats)))   # (keep_x and buf live until here)
        return ret, stats.as_dict()

    def sddmm(self, X, Y, add="plus", mul="times", accum="second", space="device", k=None):
        """The sampled dense-dense product on this CSR's (M x N) pattern as a new CSR result on the device
        (``osp_csr_sddmm``): entry (i, j) gets ``accum(c, d)`` with c this result's value there and d the reduction, in
        ``reduce``'s bit-defined order, of ``mul(X[i, c], Y[j, c])`` over c in [0, k) -- equal in bits to ``mxv`` of the
        one-row CSR that holds ``X[i, :]`` with the vector ``Y[j, :]``.  ``X`` is M x k and ``Y`` N x k, row-major and
        contiguous (``Y is X`` is allowed): 2-D torch tensors or device addresses (``space="device"``; an address carries no
        shape, so ``k`` is needed) or array-likes (``space="host"``).  ``add`` is ``"plus" "min" "max"``, ``mul`` is ``"times"
        "plus" "min" "max" "first" "second"``; ``"first"`` reads no ``Y`` and ``"second"`` no ``X`` (which may then be None).
        ``accum`` is ``"plus" "times" "minus" "div" "min" "max" "second"`` with this result's value in a's place, or None,
        which means ``"second"``: the value is d alone and no value of this result is read.  k == 0 gives the identity of
        ``add`` for d.  Returns (result, stats dict): nnz_in, nnz_out, cols, lanes_per_entry, launches, ms_total."""
        sr = _lib.Semiring()
        sr.add, sr.mul = _enum(_lib.MXV_ADD_OPS, add, "add"), _enum(_lib.MXM_MUL_OPS, mul, "mul")
        acc = _lib.VECTOR_NONE if accum is None else _enum(_lib.SDDMM_ACCUM_OPS, accum, "accum")
        sp = _space(space)
        M, N = self.shape
        if X is None and mul != "second":
            raise OspError(_lib.ERR_ARG, 'X may be None only when mul is "second"')
        if Y is None and mul != "first":
            raise OspError(_lib.ERR_ARG, 'Y may be None only when mul is "first"')
        X, Y = (None if mul == "second" else X), (None if mul == "first" else Y)   # (an operand mul does not read is not looked at)
        ks = {}   # the number of columns of every operand that carries a shape
        for what, v, n in (("X", X, "M"), ("Y", Y, "N")):
            shape = None if v is None else tuple(v.shape) if hasattr(v, "shape") else np.shape(v) if space == "host" else None
            if shape is not None and len(shape) != 2:
                raise OspError(_lib.ERR_ARG, f"{what} must be 2-D ({n} x k)")
            if shape is not None:
                ks[what] = shape[1]
        if len(set(ks.values())) > 1:
            raise OspError(_lib.ERR_ARG, f"X and Y must have the same number of columns (got {ks['X']} and {ks['Y']})")
        if k is None:
            if not ks:
                raise OspError(_lib.ERR_ARG, "X and Y must be 2-D; with device addresses, pass k")
            k = next(iter(ks.values()))
        elif ks and next(iter(ks.values())) != int(k):
            raise OspError(_lib.ERR_ARG, f"k = {k} differs from the operands' number of columns")
        k = int(k)
        if not 0 <= k <= _lib.MXD_MAX_COLS:
            raise OspError(_lib.ERR_ARG, f"k must lie in [0, {_lib.MXD_MAX_COLS}] (got {k})")
        xp, keep_x = _dense_arg(X, (M, k), self.dtype, space, "X", floating=True)
        # (Y is X: one conversion, and the library sees one address)
        yp, keep_y = (xp, keep_x) if Y is X and M == N else _dense_arg(Y, (N, k), self.dtype, space, "Y", floating=True)
        return _call(self._ctx, "osp_csr_sddmm", self._h, C.byref(sr), acc, xp, yp, k, sp, stats=_lib.SddmmStats(), keep=(keep_x, keep_y))

    def apply_vectors(self, rows=None, row_op=None, cols=None, col_op=None, space="device"):
        """This CSR's pattern with every value ``col_op(row_op(c, rows[i]), cols[j])`` as a new CSR result on the device
        (``osp_csr_apply_vectors``).  Each op is ``"plus" "times" "minus" "div" "min" "max" "second"`` -- one IEEE operation
        with the entry in a's place and the vector's element in b's, as ``ewise`` defines them -- or None to skip that side
        (at least one side is needed).  ``rows``: M values, ``cols``: N values of this dtype, device addresses / torch
        tensors (``space="device"``) or array-likes (``space="host"``).  Returns (result, stats dict): nnz_in, nnz_out,
        long_segments, ms_total, launches."""
        ap = _lib.VectorApply()
        for side, op in (("row_op", row_op), ("col_op", col_op)):
            if op is not None and op not in _lib.VECTOR_APPLY_OPS:
                raise ValueError(f"{side} must be None or one of {' '.join(_lib.VECTOR_APPLY_OPS)} (got {op!r})")
            setattr(ap, side, _lib.VECTOR_NONE if op is None else _lib.VECTOR_APPLY_OPS[op])
        sp = _space(space)
        M, N = self.shape
        x, keep_x = _dense_arg(rows if row_op is not None else None, (M,), self.dtype, space, "rows")
        y, keep_y = _dense_arg(cols if col_op is not None else None, (N,), self.dtype, space, "cols")
        return _call(self._ctx, "osp_csr_apply_vectors", self._h, C.byref(ap), x, y, sp, stats=_lib.VectorStats(), keep=(keep_x, keep_y))

    def select_vertices(self, keep_rows=None, keep_cols=None, space="device"):
        """The entries (i, j) of this CSR with ``keep_rows[i] != 0`` and ``keep_cols[j] != 0`` as a new CSR result on the
        device (``osp_csr_select_vertices``); a vector given as None keeps everything on its side (one of them is needed).
        The shape stays: a removed vertex is an empty row or column.  ``keep_rows``: M bytes, ``keep_cols``: N bytes (uint8 /
        bool), device addresses / torch tensors (``space="device"``) or array-likes (``space="host"``).  Returns (result,
        stats dict): nnz_in, nnz_out, long_segments, ms_total, launches."""
        sp = _space(space)
        M, N = self.shape
        kr, keep_r = _dense_arg(keep_rows, (M,), np.uint8, space, "keep_rows")
        kc, keep_c = _dense_arg(keep_cols, (N,), np.uint8, space, "keep_cols")
        return _call(self._ctx, "osp_csr_select_vertices", self._h, kr, kc, sp, stats=_lib.VectorStats(), keep=(keep_r, keep_c))

    def extract(self, rows=None, cols=None, space="device"):
        """The submatrix ``out[i, k] = self[rows[i], cols[k]]``, renumbered, as a new ``len(rows) x len(cols)`` CSR result
        on the device (``osp_csr_extract``); a list given as None takes every row / column.  ``rows``: any order, duplicates
        allowed.  ``cols``: None or strictly ascending lists go to the library directly; any other list (a permutation,
        duplicates) is computed by composition -- ``T = self.transpose(); Y = T.extract(rows=cols); Z = Y.transpose();
        out = Z.extract(rows=rows)`` (with ``rows`` None, Z itself) -- a row gather keeps the order inside a row and the
        transpose sorts stably, so the result has ascending columns, the copies of a repeated column next to each other in
        list order.  Lists are torch
        tensors of 4-byte integers or ``(device address, count)`` pairs (``space="device"``: the caller has synchronised; a
        bare address is taken as ascending) or array-likes (``space="host"``).  An index beyond its dimension is
        ``OspError(ERR_ARG)`` on either path.  Values keep their bits.  Returns (result, stats dict): nnz_in, nnz_gathered,
        nnz_out, ms_total, launches, readbacks, composed (the composed path: the sums over its calls)."""
        sp = _space(space)
        rp, nr, keep_r, _ = _index_arg(rows, space, "rows")
        cp, nc, keep_c, ascending = _index_arg(cols, space, "cols")
        if ascending is False:
            made = []
            try:
                T, st_t = self.transpose()
                made.append(T)
                Y, st_y = T.extract(rows=cols, space=space)
                made.append(Y)
                Z, st_z = Y.transpose()
                parts = [st_t, st_y, st_z]
                if rows is None:   # (every row: Z is the result, a fourth call would only copy it)
                    out = Z
                else:
                    made.append(Z)
                    out, st = Z.extract(rows=rows, space=space)
                    parts.append(st)
            finally:
                for t in made:
                    t.close()
            stats = {"nnz_in": self.nnz, "nnz_gathered": out.nnz if rows is None else st["nnz_gathered"], "nnz_out": out.nnz,
                     "ms_total": sum(p["ms_total"] for p in parts), "launches": sum(p["launches"] for p in parts),
                     "readbacks": st_y["readbacks"] + (0 if rows is None else st["readbacks"]), "composed": True}
            return out, stats
        ex = _lib.Extract()
        ex.rows, ex.n_rows, ex.cols, ex.n_cols, ex.space = rp, nr, cp, nc, sp
        out, stats = _call(self._ctx, "osp_csr_extract", self._h, C.byref(ex), stats=_lib.ExtractStats(), keep=(keep_r, keep_c))
        return out, dict(stats, composed=False)

    def permute(self, perm, space="device"):
        """``extract(perm, perm)`` on a square result: vertex ``perm[i]`` becomes vertex i."""
        if self.shape[0] != self.shape[1]:
            raise OspError(_lib.ERR_DIM, f"permute needs a square result (got {self.shape[0]} x {self.shape[1]})")
        return self.extract(perm, perm, space)

    def assign(self, a, rows=None, cols=None, accum=None, space="device"):
        """This result with the region ``rows x cols`` assigned from ``a``, as a new CSR result of this result's shape on the
        device (``osp_csr_assign``), the inverse of ``extract``: ``a[i, k]`` stands at ``(rows[i], cols[k])``; a list given as
        None is every row / column.  ``accum=None`` replaces the region (an entry of ``self`` inside it that ``a`` does not
        hold is deleted); ``accum`` ``"plus" "times" "min" "max" "first" "second"`` combines: ``op(self, a)`` where both hold
        a coordinate, the one value's bits where one does.  Outside the region the entries are ``self``'s, bit for bit.
        ``a`` is a ``CsrResult`` of ``len(rows) x len(cols)``, this result's context and dtype (``self`` itself is allowed).
        ``rows``: any order, distinct.  ``cols``: None or strictly ascending lists go to the library directly; any other
        list is handled by composition -- with ``o = argsort(cols)``, ``a.extract(cols=o)`` is assigned with ``cols[o]`` --
        and a repeated column then fails in the library as not strictly ascending.  Lists are as ``extract`` takes them.
        Returns (result, stats dict): nnz_c, nnz_a, nnz_region, nnz_both, nnz_out, ms_total, launches, readbacks, composed
        (the composed path: ms_total, launches and readbacks are the sums over its calls)."""
        sp = _space(space)
        acc = _lib.ASSIGN_NO_ACCUM if accum is None else _enum(_lib.ASSIGN_ACCUM_OPS, accum, "accum")
        rp, nr, keep_r, _ = _index_arg(rows, space, "rows")
        cp, nc, keep_c, ascending = _index_arg(cols, space, "cols")
        self._same_family(a, context=False)   # (the context is not checked here: the library refuses a foreign operand)
        sorted_a, st_x = None, None
        if ascending is False:
            if a.shape[1] != nc:
                raise OspError(_lib.ERR_DIM, f"a must have {nc} columns (got {a.shape[1]})")
            if space == "host":
                w = np.asarray(keep_c, np.int64)
                order = np.argsort(w, kind="stable")
                by_rank = w[order]
            else:
                import torch
                w = keep_c.long() & 0xffffffff
                order = torch.argsort(w, stable=True)
                order, by_rank = order.to(torch.int32).contiguous(), w[order].to(torch.int32).contiguous()   # (the low 32 bits)
                torch.cuda.synchronize(keep_c.device)   # the library works on its own stream
            cp, nc, keep_c, _ = _index_arg(by_rank, space, "cols")   # (a repeated column is the library's to refuse)
            sorted_a, st_x = a.extract(cols=order, space=space)
            a = sorted_a
        spec = _lib.Assign()
        spec.rows, spec.n_rows, spec.cols, spec.n_cols, spec.space, spec.accum = rp, nr, cp, nc, sp, acc
        try:
            out, stats = _call(self._ctx, "osp_csr_assign", self._h, a._h, C.byref(spec), stats=_lib.AssignStats(), keep=(keep_r, keep_c))
        finally:
            if sorted_a is not None:
                sorted_a.close()
        if st_x is not None:
            for key in ("ms_total", "launches", "readbacks"):
                stats[key] += st_x[key]
        return out, dict(stats, composed=st_x is not None)

    def embed(self, shape, rows=None, cols=None, space="device"):
        """This result placed in an otherwise empty result of ``shape``: ``out[rows[i], cols[k]] = self[i, k]``, the inverse
        of ``extract`` -- an empty result from ``Context.build`` with empty lists, then ``assign`` into it.  Returns
        ``assign``'s (result, stats dict)."""
        _space(space)
        _index_arg(rows, space, "rows")
        _index_arg(cols, space, "cols")
        M, N = (int(d) for d in shape)
        empty, _ = self._ctx.build(M, N, [], [], dtype=self.dtype, space="host")
        try:
            return empty.assign(self, rows, cols, None, space)
        finally:
            empty.close()

    def coo_rows_into(self, rows_device_ptr):
        """Row index of every entry into caller-owned DEVICE memory (nnz u32 values): with ``device_ptrs()[1:]`` the COO
        form ``Context.spgemm_coo_device`` takes (``osp_result_coo_rows``)."""
        _lib.check(_lib.lib().osp_result_coo_rows(self._h, C.c_void_p(int(rows_device_ptr))))

    def to_scipy(self):
        import scipy.sparse as sp
        rowptr, colidx, vals = self.to_host()
        return sp.csr_matrix((vals, colidx.astype(np.int64), rowptr), shape=self.shape)

    def write_mtx(self, path):
        _lib.check(_lib.lib().osp_result_write_mtx(self._h, os.fsencode(path)))

    def close(self):
        if self._h is not None:
            _lib.lib().osp_result_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ALGORITHMS = {"outer": 0, "rowwise": 1}  # osp_algorithm_t


def aos_dtype(value_dtype):
    """numpy view of the reference's packed ``CSRElement{index_t idx; value_t val}`` (``common.h:10-16``)."""
    return np.dtype([("idx", "<u4"), ("val", np.dtype(value_dtype).newbyteorder("<"))], align=False)


def _config(validate, partial_capacity, k_range=None, row_shard=None, algorithm=None):
    """``osp_config_t``: the library's defaults with the given fields set."""
    cfg = _lib.Config()
    _lib.lib().osp_config_default(C.byref(cfg))
    cfg.validate = int(bool(validate))
    cfg.partial_capacity = int(partial_capacity or 0)
    if k_range is not None:
        cfg.k_begin, cfg.k_end = int(k_range[0]), int(k_range[1])
    if row_shard is not None:
        cfg.row_shard_index, cfg.row_shard_count = int(row_shard[0]), int(row_shard[1])
    if algorithm is not None:
        cfg.algorithm = ALGORITHMS[algorithm]
    return cfg


def _csc_csr_arrays(K, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals):
    """The six host operands of a product A(CSC) * B(CSR) as contiguous arrays of the ABI's types: (value dtype, arrays)."""
    dt = np.dtype(a_vals.dtype)
    if dt not in _DT or np.dtype(b_vals.dtype) != dt:
        raise TypeError("values must both be float32 or both float64")
    arrs = [np.ascontiguousarray(a_colptr, np.int64), np.ascontiguousarray(a_rowidx, np.uint32), np.ascontiguousarray(a_vals, dt),
            np.ascontiguousarray(b_rowptr, np.int64), np.ascontiguousarray(b_colidx, np.uint32), np.ascontiguousarray(b_vals, dt)]
    if len(arrs[0]) != K + 1 or len(arrs[3]) != K + 1:
        # reference: assert(csc.pos.size() == csr.pos.size()), SimSpGEMM.cpp:267
        raise OspError(_lib.ERR_DIM, f"pointer arrays must have K+1={K + 1} entries (got {len(arrs[0])} and {len(arrs[3])})")
    return dt, arrs


class Context:
    """One GPU + one HIP stream + a buffer pool (``osp_context_t``)."""

    def __init__(self, device=0, stream=None):
        self._h = None
        self._results = weakref.WeakSet()
        h = C.c_void_p()
        if stream is None:
            _lib.check(_lib.lib().osp_context_create(device, C.byref(h)))
        else:
            _lib.check(_lib.lib().osp_context_create_on_stream(device, C.c_void_p(stream), C.byref(h)))
        self._h = h
        self.device = device
        #: "outer" (default) or "rowwise": which formulation the products of this context use (osp_config_t.algorithm)
        self.algorithm = "outer"

    def close(self):
        if self._h is not None:
            for r in list(self._results):
                r.close()
            _lib.lib().osp_context_destroy(self._h)
            self._h = None

    def trim(self):
        _lib.check(_lib.lib().osp_context_trim(self._h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _config(self, validate, partial_capacity, k_range, row_shard=None):
        return _config(validate, partial_capacity, k_range, row_shard, self.algorithm)

    def spgemm_csc_csr(self, M, K, N, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals, *,
                       validate=True, partial_capacity=0, k_range=None, row_shard=None):
        """C = A(CSC) * B(CSR) with numpy (host) operands.  row_shard=(i, G): only the i-th of G output-row ranges
        (balanced by partial products; ``result.info['row_begin'/'row_end']`` say which rows came back)."""
        dt, arrs = _csc_csr_arrays(K, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals)
        cfg = self._config(validate, partial_capacity, k_range, row_shard)
        return _call(self, "osp_spgemm_csc_csr", self._h, _DT[dt], M, K, N, *[_ptr(a) for a in arrs], _lib.OSP_HOST, C.byref(cfg), keep=arrs)

    def spgemm_csc_csr_aos(self, M, K, N, a_pos, a_data, b_pos, b_data, *, validate=True, partial_capacity=0):
        """The reference's in-memory operands as they stand (``osp_spgemm_csc_csr_aos``): ``pos`` = ``CSRMatrix::pos``
        (K+1 uint64 offsets), ``data`` = ``CSRMatrix::data`` as a packed structured array ``aos_dtype(value dtype)`` =
        ``[('idx', '<u4'), ('val', '<f4' | '<f8')]`` (``common.h:10-16``: 8 or 12 bytes per record)."""
        vdt = np.dtype(a_data.dtype.fields["val"][0])
        want = aos_dtype(vdt)
        if a_data.dtype != want or b_data.dtype != want:
            raise TypeError(f"data arrays must both have dtype {want}")
        ap, bp = np.ascontiguousarray(a_pos, np.uint64), np.ascontiguousarray(b_pos, np.uint64)
        if len(ap) != K + 1 or len(bp) != K + 1:
            raise OspError(_lib.ERR_DIM, f"pos arrays must have K+1={K + 1} entries (got {len(ap)} and {len(bp)})")
        ad, bd = np.ascontiguousarray(a_data), np.ascontiguousarray(b_data)
        cfg = self._config(validate, partial_capacity, None)
        return _call(self, "osp_spgemm_csc_csr_aos", self._h, _DT[vdt], M, K, N, _ptr(ap), _ptr(ad), _ptr(bp), _ptr(bd), _lib.OSP_HOST,
                     C.byref(cfg), keep=(ap, ad, bp, bd))

    def alloc(self, nbytes):
        """Device memory from the context's buffer pool (``osp_context_alloc``); give it back with ``free``."""
        p = C.c_void_p()
        _lib.check(_lib.lib().osp_context_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value or 0

    def free(self, ptr):
        if self._h is not None and ptr:
            _lib.check(_lib.lib().osp_context_free(self._h, C.c_void_p(int(ptr))))

    def spgemm_coo(self, M, K, N, a, b, *, partial_capacity=0):
        """C = A * B from COO triples a = (rows, cols, vals), b = (rows, cols, vals) in any order (numpy, host):
        ``coo2csr<true>(A)`` / ``coo2csr(B)`` (SimSpGEMM.cpp:102-152) run on the GPU; duplicates raise 233."""
        dt = np.dtype(a[2].dtype)
        if dt not in _DT or np.dtype(b[2].dtype) != dt:
            raise TypeError("values must both be float32 or both float64")
        arrs = [np.ascontiguousarray(a[0], np.uint32), np.ascontiguousarray(a[1], np.uint32), np.ascontiguousarray(a[2], dt),
                np.ascontiguousarray(b[0], np.uint32), np.ascontiguousarray(b[1], np.uint32), np.ascontiguousarray(b[2], dt)]
        cfg = self._config(True, partial_capacity, None)
        return _call(self, "osp_spgemm_coo", self._h, _DT[dt], M, K, N, len(arrs[0]), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                     len(arrs[3]), _ptr(arrs[3]), _ptr(arrs[4]), _ptr(arrs[5]), _lib.OSP_HOST, C.byref(cfg), keep=arrs)

    def stream_copy_gbps(self, nbytes=2 << 30, reps=10):
        """What a plain 16-bytes-per-lane copy reaches on this device, read + written bytes per second in GB/s
        (``osp_stream_copy_probe``): the measured roof beside the data sheet's."""
        g = C.c_double()
        _lib.check(_lib.lib().osp_stream_copy_probe(self._h, int(nbytes), int(reps), C.byref(g)))
        return g.value

    def spgemm_coo_device(self, dtype, M, K, N, nnz_a, a_ptrs, nnz_b, b_ptrs, *, partial_capacity=0, k_range=None):
        """``spgemm_coo`` on DEVICE arrays: a_ptrs / b_ptrs = (rows, cols, vals) addresses (u32, u32, dtype), entries in any
        order.  ``result.info['ms_ingest']`` is the device time of the two COO -> CSC / CSR conversions.  ``k_range``
        restricts the PRODUCT behind the conversions to a slab of k (the conversions always take the whole operands)."""
        cfg = self._config(True, partial_capacity, k_range)
        return _call(self, "osp_spgemm_coo", self._h, _DT[np.dtype(dtype)], M, K, N, int(nnz_a), *_dptrs(a_ptrs), int(nnz_b), *_dptrs(b_ptrs),
                     _lib.OSP_DEVICE, C.byref(cfg))

    def im2col_device(self, dtype, N, C_, H, W, nnz_x, x_ptrs, geom, *, out_ptrs=None, validate=True):
        """im2col of a "pixel x channel" activation into CSC (``osp_im2col_csc``).  x_ptrs = (rows, cols, vals) DEVICE
        addresses of the input's COO (row n*H*W + y*W + x, column c; any order), geom = ``conv2d_geometry(...)``.  Without
        ``out_ptrs`` only nnz(A) is computed; with out_ptrs = (colptr, rowidx, vals) device addresses of C*kh*kw + 1,
        nnz(A) and nnz(A) entries A is written there.  Returns nnz(A)."""
        n = C.c_uint64()
        outs = [None, None, None] if out_ptrs is None else _dptrs(out_ptrs, null=True)
        _lib.check(_lib.lib().osp_im2col_csc(self._h, _DT[np.dtype(dtype)], int(N), int(C_), int(H), int(W), int(nnz_x),
                                             *_dptrs(x_ptrs, null=True), _lib.OSP_DEVICE, C.byref(geom), int(bool(validate)), C.byref(n), *outs))
        return n.value

    def spgemm_conv2d_device(self, dtype, N, C_, H, W, nnz_x, x_ptrs, OC, nnz_w, w_ptrs, geom, *, validate=True, partial_capacity=0):
        """A conv layer as the CLI's product im2col(x) * W^T (``osp_spgemm_conv2d``): x as in ``im2col_device``, W the
        OC x (C*kh*kw) weight as (rows, cols, vals) DEVICE addresses.  Returns the (N*OH*OW) x OC CSR result (NHWC)."""
        cfg = self._config(validate, partial_capacity, None)
        return _call(self, "osp_spgemm_conv2d", self._h, _DT[np.dtype(dtype)], int(N), int(C_), int(H), int(W), int(nnz_x),
                     *_dptrs(x_ptrs, null=True), int(OC), int(nnz_w), *_dptrs(w_ptrs, null=True), _lib.OSP_DEVICE, C.byref(geom), C.byref(cfg))

    def spgemm_csc_csr_device(self, dtype, M, K, N, ptrs, *, validate=False, partial_capacity=0, k_range=None, row_shard=None):
        """Same with six DEVICE addresses (ints): a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals.
        The arrays must be COMPLETE when this is called: the context works on a stream of its own (or the one it was
        created on) and does not wait for kernels other streams -- e.g. torch's -- still have in flight on them."""
        cfg = self._config(validate, partial_capacity, k_range, row_shard)
        return _call(self, "osp_spgemm_csc_csr", self._h, _DT[np.dtype(dtype)], M, K, N, *_dptrs(ptrs), _lib.OSP_DEVICE, C.byref(cfg))

    def spgemm_masked(self, M, K, N, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals, m_rowptr, m_colidx, *, validate=True):
        """C<mask> = A(CSC) * B(CSR) with numpy (host) operands (``osp_spgemm_masked``): the entries of the product at the
        mask's pattern (M x N, CSR, no values) where at least one product exists, the same bits as the unmasked product
        there.  ``result.info['partials']`` is the number of products formed.  The call holds N + 1 offsets of B's column
        view on the device, and M, K or N of 2^32 - 256 and more is ``OspError(ERR_ARG)``."""
        dt, arrs = _csc_csr_arrays(K, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals)
        mr, mc = np.ascontiguousarray(m_rowptr, np.int64), np.ascontiguousarray(m_colidx, np.uint32)
        if len(mr) != M + 1:
            raise OspError(_lib.ERR_ARG, f"the mask's row pointers must have M+1={M + 1} entries (got {len(mr)})")
        cfg = self._config(validate, 0, None)
        return _call(self, "osp_spgemm_masked", self._h, _DT[dt], M, K, N, *[_ptr(a) for a in arrs], C.c_void_p(mr.ctypes.data), _ptr(mc),
                     _lib.OSP_HOST, C.byref(cfg), keep=(arrs, mr, mc))

    def spgemm_masked_device(self, dtype, M, K, N, ptrs, mask_ptrs, *, validate=False):
        """Same with DEVICE addresses (ints): ``ptrs`` as in ``spgemm_csc_csr_device``, ``mask_ptrs`` = (m_rowptr, m_colidx).
        The arrays must be complete when this is called (see ``spgemm_csc_csr_device``)."""
        cfg = self._config(validate, 0, None)
        return _call(self, "osp_spgemm_masked", self._h, _DT[np.dtype(dtype)], M, K, N, *_dptrs(ptrs), *_dptrs(mask_ptrs), _lib.OSP_DEVICE,
                     C.byref(cfg))

    def spgemm_partials_device(self, dtype, M, K, N, ptrs, *, k_range=None):
        """The multiply phase alone (``osp_spgemm_partials``): the product's partial products, unmerged, as packed records
        grouped by output row.  ``ptrs`` = six DEVICE addresses as in ``spgemm_csc_csr_device``.  ``result.nnz`` = P;
        ``result.partials_ptrs()`` borrows the arrays."""
        cfg = self._config(False, 0, k_range)
        return _call(self, "osp_spgemm_partials", self._h, _DT[np.dtype(dtype)], M, K, N, *_dptrs(ptrs), _lib.OSP_DEVICE, C.byref(cfg))

    def merge_record_parts_device(self, dtype, M, N, part_ptrs, *, partial_capacity=0, validate=False):
        """Sum parts given as (rowptr, records) DEVICE addresses (``osp_merge_record_parts``) into one CSR.
        validate=True checks the offsets and the columns on the device first."""
        n = len(part_ptrs)
        rp, rc = (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, (r, c) in enumerate(part_ptrs):
            rp[i], rc[i] = int(r), int(c)
        cfg = self._config(validate, partial_capacity, None)
        return _call(self, "osp_merge_record_parts", self._h, _DT[np.dtype(dtype)], M, N, n, rp, rc, _lib.OSP_DEVICE, C.byref(cfg))

    def spgemm_csc_csr_panels(self, dtype, M, K, N, ptrs, on_panel, *, device=True, validate=False, partial_capacity=0,
                              k_range=None, row_shard=None):
        """Streamed product (``osp_spgemm_csc_csr_panels``): C is never resident as a whole.  ``ptrs`` = the six operand
        addresses (ints; device memory unless device=False).  ``on_panel(p)`` is called once per finished row panel, in
        row order, with a dict: row_begin, row_end, nnz, index, count and the DEVICE addresses rowptr / colidx / vals
        (valid only during the call; wrap them zero-copy, e.g. ``distributed._as_tensor``).  An exception raised by
        the callback aborts the product and is re-raised.  Returns the info dict (counters, phase times)."""
        cfg = self._config(validate, partial_capacity, k_range, row_shard)
        err = []

        def tramp(pp, _user):
            p = pp.contents
            try:
                on_panel({"row_begin": p.row_begin, "row_end": p.row_end, "nnz": p.nnz, "index": p.index, "count": p.count,
                          "rowptr": p.rowptr or 0, "colidx": p.colidx or 0, "vals": p.vals or 0})
                return 0
            except BaseException as e:  # never let an exception cross the C frames
                err.append(e)
                return 1

        fn = _lib.PANEL_FN(tramp)
        info = _lib.ResultInfo()
        st = _lib.lib().osp_spgemm_csc_csr_panels(self._h, _DT[np.dtype(dtype)], M, K, N, *_dptrs(ptrs),
                                                  _lib.OSP_DEVICE if device else _lib.OSP_HOST, C.byref(cfg), fn, None, C.byref(info))
        if err:
            raise err[0]
        _lib.check(st)
        return info.as_dict()

    def merge_csr_parts(self, M, N, parts, *, partial_capacity=0):
        """Sum CSR matrices of equal shape.  parts: list of (rowptr, colidx, vals) numpy triples."""
        dt = np.dtype(parts[0][2].dtype)
        keep, n = [], len(parts)
        rp, ci, va = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, (r, c, v) in enumerate(parts):
            r = np.ascontiguousarray(r, np.int64); c = np.ascontiguousarray(c, np.uint32); v = np.ascontiguousarray(v, dt)
            keep += [r, c, v]
            rp[i], ci[i], va[i] = r.ctypes.data, (c.ctypes.data if c.size else 0), (v.ctypes.data if v.size else 0)
        cfg = self._config(False, partial_capacity, None)
        return _call(self, "osp_merge_csr_parts", self._h, _DT[dt], M, N, n, rp, ci, va, _lib.OSP_HOST, C.byref(cfg), keep=keep)

    def merge_csr_parts_device(self, dtype, M, N, part_ptrs, *, partial_capacity=0):
        """Device-resident parts: list of (rowptr, colidx, vals) device addresses."""
        n = len(part_ptrs)
        rp, ci, va = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, (r, c, v) in enumerate(part_ptrs):
            rp[i], ci[i], va[i] = int(r), int(c), int(v)
        cfg = self._config(False, partial_capacity, None)
        return _call(self, "osp_merge_csr_parts", self._h, _DT[np.dtype(dtype)], M, N, n, rp, ci, va, _lib.OSP_DEVICE, C.byref(cfg))

    def build(self, M, N, rows, cols, vals=None, *, dup="plus", dtype=np.float64, space="host"):
        """An M x N CSR result from the COO list (rows[t], cols[t], vals[t]) (``osp_csr_build``): any order, a coordinate may
        repeat, and the repeats are combined in LIST order by ``dup``: ``"plus"`` (acc + v), ``"min"``, ``"max"`` (``ewise``'s
        expressions), ``"first"``, ``"last"``, ``"count"`` (how many, as a value; reads no value) or ``"error"`` (a repeat is
        ``OspError(ERR_DUPLICATE)``).  A coordinate given once keeps its value's bits.  ``vals=None``: every value is 1.
        Lists are array-likes (``space="host"``; ``vals`` is converted to ``dtype``) or torch tensors of 4-byte integers /
        ``(device address, count)`` pairs, with ``vals`` a tensor of ``dtype`` or a device address (``space="device"``: the
        caller has synchronised).  An index beyond its dimension is ``OspError(ERR_RANGE)`` on either path.  Returns
        (result, stats dict): nnz_in, nnz_out, long_runs, ms_total, launches, readbacks."""
        b = _lib.Build()
        b.space, b.dup = _space(space), _enum(_lib.DUP_OPS, dup, "dup")
        dt = np.dtype(dtype)
        if dt not in _DT:
            raise TypeError("dtype must be float32 or float64")
        rp, nr, keep_r = _u32_list(rows, space, "rows")   # (an empty list: address 0, passed as NULL)
        cp, nc, keep_c = _u32_list(cols, space, "cols")
        if nr != nc:
            raise OspError(_lib.ERR_ARG, f"rows and cols must have the same length (got {nr} and {nc})")
        vp, keep_v = None, None
        if vals is not None:
            if space == "host":
                keep_v = np.ascontiguousarray(vals, dt)
                if keep_v.shape != (nr,):
                    raise OspError(_lib.ERR_ARG, f"vals must have {nr} entries (got shape {keep_v.shape})")
                vp = keep_v.ctypes.data if nr else None
            elif hasattr(vals, "data_ptr"):
                if vals.numel() != nr or vals.element_size() != dt.itemsize or not vals.is_floating_point() or not vals.is_contiguous():
                    raise OspError(_lib.ERR_ARG, f"vals must be a contiguous tensor of {nr} values of {dt}")
                keep_v, vp = vals, (vals.data_ptr() if nr else None)
            else:
                vp = int(vals)
        b.M, b.N, b.nnz, b.dtype = int(M), int(N), nr, _DT[dt]
        b.rows, b.cols, b.vals = rp or None, cp or None, vp
        return _call(self, "osp_csr_build", self._h, C.byref(b), stats=_lib.BuildStats(), keep=(keep_r, keep_c, keep_v))

    def spgemm_mtx(self, path_a, path_b, transpose_b=True, dtype=np.float32, *, validate=True, partial_capacity=0):
        """The reference CLI's data flow: two .mtx files in, A * B^T (default) out."""
        cfg = self._config(validate, partial_capacity, None)
        return _call(self, "osp_spgemm_mtx", self._h, _DT[np.dtype(dtype)], os.fsencode(path_a), os.fsencode(path_b), int(bool(transpose_b)),
                     C.byref(cfg))


class MultiGpu:
    """Several GPUs of one node behind ONE call (``osp_multi_*``): the k-sharded product of SURVEY.md 8e inside the library --
    slabs of the shared dimension on their ranks, partial products copied GPU to GPU to the rank that owns their row while
    the next panel multiplies, one merge per row range as the pieces arrive.  ``devices`` may name an ordinal more than
    once (logical ranks sharing a GPU)."""

    def __init__(self, devices):
        self._h = None
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        _lib.check(_lib.lib().osp_multi_context_create(arr, len(devices), C.byref(h)))
        self._h = h
        self.devices = list(devices)
        self._ops = None

    def load(self, M, K, N, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals):
        """Cut k into slabs and put every rank's slab on its GPU (host numpy operands).  Replaces what was loaded before."""
        dt, arrs = _csc_csr_arrays(K, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals)
        self.unload()
        h = C.c_void_p()
        _lib.check(_lib.lib().osp_multi_operands_create(self._h, _DT[dt], M, K, N, *[_ptr(a) for a in arrs], C.byref(h)))
        self._ops, self._shape, self._dtype = h, (M, N), dt

    def unload(self):
        if self._ops is not None:
            _lib.lib().osp_multi_operands_destroy(self._ops)
            self._ops = None

    def multiply(self, *, validate=False, partial_capacity=0, fetch=True, checksum=False):
        """One product of the loaded operands.  Returns (info dict, (rowptr, colidx, vals) host arrays or None).
        checksum=True adds info["val_sum"] = the sum of all values of C, formed shard by shard on the GPUs (torch)."""
        cfg = _config(validate, partial_capacity)
        h = C.c_void_p()
        _lib.check(_lib.lib().osp_spgemm_multi(self._h, self._ops, C.byref(cfg), C.byref(h)))
        try:
            info = _lib.MultiInfo()
            _lib.check(_lib.lib().osp_multi_result_info(h, C.byref(info)))
            out = None
            extra = {}
            if checksum:
                import torch
                from .distributed import _as_tensor
                total = 0.0
                for g in range(info.nranks):
                    sh, va = C.c_void_p(), C.c_void_p()
                    _lib.check(_lib.lib().osp_multi_result_shard(h, g, None, None, C.byref(sh)))
                    _lib.check(_lib.lib().osp_result_device_ptrs(sh, None, None, C.byref(va)))
                    n = info.rank[g].nnz_c
                    if n:
                        dev = torch.device("cuda", info.rank[g].device)
                        f64 = self._dtype == np.float64
                        total += float(_as_tensor(va.value, n, "<f8" if f64 else "<f4", dev, torch.float64 if f64 else torch.float32)
                                       .sum(dtype=torch.float64))
                extra["val_sum"] = total
            if fetch:
                rowptr = np.zeros(self._shape[0] + 1, np.int64)
                colidx = np.empty(info.nnz_c, np.uint32)
                vals = np.empty(info.nnz_c, self._dtype)
                _lib.check(_lib.lib().osp_multi_result_copy_csr(h, _ptr(rowptr), _ptr(colidx), _ptr(vals)))
                out = (rowptr, colidx, vals)
            d = info.as_dict()
            d.update(extra)
            return d, out
        finally:
            _lib.lib().osp_multi_result_destroy(h)

    def spgemm_csc_csr(self, M, K, N, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals, **kw):
        self.load(M, K, N, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals)
        return self.multiply(**kw)

    def close(self):
        if self._h is not None:
            self.unload()
            _lib.lib().osp_multi_context_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- ingest helpers (host, no GPU) ---------------------------------------------------------------
def read_mtx(path, symmetric=False):
    """``readcoo`` (SimSpGEMM.cpp:55-100): returns (nrow, ncol, rows u32, cols u32, vals f64)."""
    L = _lib.lib()
    nrow, ncol, nnz = C.c_uint64(), C.c_uint64(), C.c_uint64()
    r, c, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _lib.check(L.osp_mtx_read(os.fsencode(path), int(symmetric), C.byref(nrow), C.byref(ncol), C.byref(nnz),
                              C.byref(r), C.byref(c), C.byref(v)))
    n = nnz.value
    try:
        rows = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_uint32)), (max(n, 1),))[:n].copy()
        cols = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_uint32)), (max(n, 1),))[:n].copy()
        vals = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), (max(n, 1),))[:n].copy()
    finally:
        for p in (r, c, v):
            L.osp_host_free(p)
    return nrow.value, ncol.value, rows, cols, vals


def _compress(by_col, nseg, rows, cols, vals):
    dt = np.dtype(vals.dtype)
    if dt not in _DT:
        raise TypeError("values must be float32 or float64")
    rows = np.ascontiguousarray(rows, np.uint32); cols = np.ascontiguousarray(cols, np.uint32)
    vals = np.ascontiguousarray(vals)
    nnz = len(rows)
    ptr = np.zeros(nseg + 1, np.int64); idx = np.zeros(nnz, np.uint32); out = np.zeros(nnz, dt)
    fn = getattr(_lib.lib(), "osp_coo_to_compressed_f32" if dt == np.float32 else "osp_coo_to_compressed_f64")
    _lib.check(fn(int(by_col), nseg, nnz, _ptr(rows), _ptr(cols), _ptr(vals), _ptr(ptr), _ptr(idx), _ptr(out)))
    return ptr, idx, out


def coo_to_csr(nrow, rows, cols, vals):
    """``coo2csr<false>`` (SimSpGEMM.cpp:102-152); duplicate coordinates raise OspError(233)."""
    return _compress(0, nrow, rows, cols, vals)


def coo_to_csc(ncol, rows, cols, vals):
    """``coo2csr<true>`` (SimSpGEMM.cpp:102-152)."""
    return _compress(1, ncol, rows, cols, vals)


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def _as_coo(x):
    """dense ndarray / torch tensor / scipy sparse -> (nrow, ncol, rows, cols, vals)."""
    import scipy.sparse as sp
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    if not sp.issparse(x):
        x = sp.csr_matrix(np.asarray(x))  # what util.py:61-62 does before mmwrite
    x = x.tocoo()
    return x.shape[0], x.shape[1], x.row.astype(np.uint32), x.col.astype(np.uint32), x.data


def _product_operands(A, B, transpose_b, dtype, mask=None):
    """What ``spgemm`` and ``spgemm_masked`` share: the operands checked and compressed on the host.  Returns (M, K, N, the six
    arrays of A in CSC and B in CSR -- followed by the mask's row pointers and columns when a mask is given)."""
    M, K, ar, ac, av = _as_coo(A)
    br_n, bc_n, br, bc, bv = _as_coo(B)
    if transpose_b:
        br_n, bc_n, br, bc = bc_n, br_n, bc, br
    if br_n != K:
        raise OspError(_lib.ERR_DIM, f"inner dimensions differ: A is {M}x{K}, B is {br_n}x{bc_n}")
    if mask is not None:
        mm, mn, mr, mc, _ = _as_coo(mask)
        if (mm, mn) != (M, bc_n):
            raise OspError(_lib.ERR_ARG, f"the mask is {mm}x{mn}, the product {M}x{bc_n}")
    dt = np.dtype(dtype or np.result_type(av.dtype, bv.dtype))
    if dt not in _DT:
        dt = np.dtype(np.float64)
    arrs = coo_to_csc(K, ar, ac, av.astype(dt)) + coo_to_csr(K, br, bc, bv.astype(dt))
    if mask is not None:
        arrs += coo_to_csr(M, mr, mc, np.zeros(len(mr), np.float32))[:2]
    return M, K, bc_n, arrs


def spgemm(A, B, transpose_b=True, ctx=None, dtype=None):
    """``A @ B.T`` (default, as the reference CLI) or ``A @ B`` as scipy CSR, computed on the GPU."""
    ctx = ctx or default_context()
    M, K, N, arrs = _product_operands(A, B, transpose_b, dtype)
    res = ctx.spgemm_csc_csr(M, K, N, *arrs)
    out = res.to_scipy()
    res.close()
    return out


def spgemm_masked(A, B, mask, transpose_b=True, ctx=None, dtype=None):
    """``(A @ B.T)`` (default, as ``spgemm``) or ``A @ B``, computed only at the pattern of ``mask`` (its values are not
    read), as scipy CSR.  An entry of the mask where no product exists is absent from the result; an entry whose products
    cancel is kept as an explicit 0."""
    ctx = ctx or default_context()
    M, K, N, arrs = _product_operands(A, B, transpose_b, dtype, mask)
    res = ctx.spgemm_masked(M, K, N, *arrs)
    out = res.to_scipy()
    res.close()
    return out


def block_grid(blocks):
    """The checks of ``block_matrix``, which touch no handle: ``blocks`` as a rectangular grid of ``CsrResult`` or None, every
    block row and block column with at least one block (``scipy.sparse.bmat`` refuses an all-None one too) and consistent
    heights and widths, one context and dtype.  Returns (grid, row offsets, column offsets, the first block)."""
    grid = [list(row) for row in blocks]
    if not grid or not grid[0] or any(len(row) != len(grid[0]) for row in grid):
        raise ValueError("blocks must be a non-empty rectangular grid")
    heights, widths, first = [None] * len(grid), [None] * len(grid[0]), None
    for i, row in enumerate(grid):
        for k, b in enumerate(row):
            if b is None:
                continue
            if not isinstance(b, CsrResult):
                raise TypeError("a block must be a CsrResult or None")
            first = b if first is None else first
            if b._ctx is not first._ctx:
                raise OspError(_lib.ERR_ARG, "the blocks belong to different contexts")
            if b.dtype != first.dtype:
                raise OspError(_lib.ERR_ARG, "the blocks' dtypes differ")
            for sizes, at, got, what in ((heights, i, b.shape[0], "row"), (widths, k, b.shape[1], "column")):
                if sizes[at] is None:
                    sizes[at] = got
                elif sizes[at] != got:
                    raise ValueError(f"blocks[{i}][{k}] has {got} {what}s, its block {what} {sizes[at]}")
    for sizes, what in ((heights, "row"), (widths, "column")):
        if None in sizes:
            raise ValueError(f"block {what} {sizes.index(None)} is all None: its size is unknown")
    return grid, np.concatenate([[0], np.cumsum(heights)]).astype(np.int64), np.concatenate([[0], np.cumsum(widths)]).astype(np.int64), first


def block_matrix(blocks):
    """The matrix assembled from a grid of blocks, ``scipy.sparse.bmat``'s semantics for a grid (a list of rows) of
    ``CsrResult`` or None: block (i, k) stands at the row offset of block row i and the column offset of block column k, None
    is an empty block, sizes come from the blocks and must agree along every block row and column.  It starts from an
    empty result (``Context.build`` with empty lists) and makes ONE ``assign`` per non-None block, with contiguous row and
    column lists from the offsets (None where a block spans every row or column); intermediate results are closed.  The
    cost is one pass over the growing result per block, so this is meant for small grids: [[0, B], [B^T, 0]], a few
    diagonal blocks.  The blocks stay valid.  Returns (result, stats dict): blocks (assigned), nnz_out, ms_total, launches,
    readbacks (sums over the calls)."""
    grid, r0, c0, first = block_grid(blocks)
    M, N = int(r0[-1]), int(c0[-1])
    out, _ = first._ctx.build(M, N, [], [], dtype=first.dtype, space="host")
    stats = {"blocks": 0, "nnz_out": 0, "ms_total": 0.0, "launches": 0, "readbacks": 0}
    try:
        for i, row in enumerate(grid):
            for k, b in enumerate(row):
                if b is None or b.shape[0] == 0 or b.shape[1] == 0:
                    continue
                rows = None if b.shape[0] == M else np.arange(r0[i], r0[i + 1])
                cols = None if b.shape[1] == N else np.arange(c0[k], c0[k + 1])
                nxt, st = out.assign(b, rows, cols, None, "host")
                out.close()
                out = nxt
                stats["blocks"] += 1
                for key in ("ms_total", "launches", "readbacks"):
                    stats[key] += st[key]
    except BaseException:
        out.close()
        raise
    stats["nnz_out"] = out.nnz
    return out, stats
