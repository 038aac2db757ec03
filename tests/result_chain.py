"""A seeded chain driver for the operations that take a CSR result and return a result or a vector (not a test file: the
CPU and GPU tests import it, and ``python -m tests.result_chain`` runs it on the GPU in a process of its own).

A chain starts from three uploaded CSR operands and applies 6 to 10 operations drawn at random from the whole surface --
apply_mask, select, ewise, inflate_prune, select_vertices, apply_vectors, transpose, mxm, matmul, reduce, mxv, extract (and
permute), build, mxd, sddmm, mxv_arg -- each to a randomly chosen live result or a pair of them (build to a live result's
entries as a shuffled COO list), closing results at random points so that pool buffers recycle from one
operation into another.  Every step follows one protocol, so that NaN payloads and summation orders never accumulate:

  1. the operation's device inputs are read back to the host (fresh copies, never a cache);
  2. the numpy models of tests/*_model.py compute the answer from those arrays;
  3. the backend's output is compared with it: row pointers and columns equal, values equal as BITS, and a value that came
     out of arithmetic and is a NaN in the model only has to be a NaN (each operation's own test file's rule);
  4. the stats fields the per-operation tests check are compared with what the model predicts;
  5. the output joins the live set -- a result of zero rows or zero columns, which extract makes from an empty list, like any
     other: every kind is drawn on it.

A device output that the CALLER owns (the ``out`` of reduce, mxv, mxv_arg and mxd, mxv_arg's ``out_arg``) is a slice in the
middle of a larger buffer filled with a sentinel no result can be (Frame): a margin that changed is a mismatch, and so is an
element of the output that still holds the sentinel.

The generator only draws legal calls: an illegal draw (no conforming partner, values an operation does not take, a product
beyond PRODUCT_CAP, a dense operand beyond DENSE_CAP) is REDRAWN, and no drawn step is ever skipped.  The driver talks to a
backend object: GpuBackend wraps CsrResult, ModelBackend the models themselves, so the generator and the coverage counters run
without a GPU (tests/test_result_chain_cpu.py), and a ModelBackend with one planted defect shows that the comparison bites.

Only a mismatch, or a call the library refused, becomes a ChainMismatch (exit status 1 of main(); 2: the default seeds miss
a coverage condition).  Any other error -- OspError(ERR_HIP), an error of torch -- may be a GPU fault: it leaves the driver
as itself, nothing is closed behind it, and main() exits with DEVICE_ERROR_STATUS so that a caller starts nothing more on
the GPU."""
import argparse
import collections
import os
import re
import sys
import time

import numpy as np

from tests import (bfs_model, build_model, ewise_model, extract_model, mcl_model, mxd_model, mxv_arg_model, mxv_model, sddmm_model,
                   semiring_model, transpose_model, truss_model, vector_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMPACT = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_compact.h")).read()
# the unit of work of the bit compaction behind every CSR-to-CSR filter
CHUNK = int(re.search(r"kCompactThreads\s*=\s*(\d+)", _COMPACT).group(1)) * int(re.search(r"kCompactRounds\s*=\s*(\d+)", _COMPACT).group(1))
BLOCK = vector_model.BLOCK           # the longest segment one wave reduces
SHORT_CAP = semiring_model.SHORT_CAP  # the most products of a short row of mxm
# transpose: a result of at most this many rows takes the row-mask path
ROWMASK_MAX = int(re.search(r"kTrMaskRows\s*=\s*(\d+)", open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_transpose.h")).read()).group(1))
FRONTIER_NCOL = 1 << 16
# mxm and matmul are redrawn when the operands' row pointers predict more partial products than this.  Chosen on the CPU so
# that the numpy models keep the default seeds well under a minute (MEASUREMENTS.md section 0m); one row of the starting
# operands alone gives more than 3 * SHORT_CAP products, so the long-row class of mxm stays reachable.
PRODUCT_CAP = 400_000
MCL_MAX_ROWS = 4096                  # the model of inflate_prune loops over rows in Python
MAX_LIVE = 6
# mxd and sddmm redraw k while the entries times k, or a dense operand's rows times k, exceed this many elements.  Chosen on
# the CPU like PRODUCT_CAP (the models of mxd and sddmm are k passes over the entries); the largest k stays reachable on the
# three starting operands: at most 60 000 entries (starting_operands asserts it) and the frontier's 2^16 columns.
DENSE_CAP = 9_000_000
KINDS = ["apply_mask", "select", "ewise", "inflate_prune", "select_vertices", "apply_vectors", "transpose", "mxm", "matmul", "reduce",
         "mxv", "extract", "build", "mxd", "sddmm", "mxv_arg"]
DTYPES = [np.float32, np.float64]
# chosen on the model backend (greedily, among the seeds below 800) so that every condition of Coverage.REQUIRED is met
# twice in both dtypes (the results of zero rows or columns are rare, and the seeds that reach every kind with one hold many)
DEFAULT_SEEDS = [92, 109, 133, 181, 256, 267, 311, 323, 340, 426, 485, 553, 566, 619, 632, 657, 728]
assert PRODUCT_CAP > 3 * SHORT_CAP
assert DENSE_CAP >= max(60_000, FRONTIER_NCOL) * max(mxd_model.KS + sddmm_model.KS)


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _special(dt):
    from tests import test_gpu_apply_mask as am   # (imports torch: only when operands are built)
    return am._special(dt)


def _mask_for(*a, **kw):
    from tests import test_gpu_apply_mask as am
    return am._mask_for(*a, **kw)


# the library's status for a HIP runtime error, from its C header (outerspace_amd._lib, which loads the library, has the same)
ERR_HIP = int(re.search(r"OSP_ERR_HIP\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read()).group(1))
DEVICE_ERROR_STATUS = 3    # main()'s exit status for an error that is no mismatch: what follows must leave the GPU alone


def is_refusal(e):
    """Whether an exception out of a backend's call says that the library REFUSED the call (a finding like any mismatch:
    every draw is legal) and not that the device or the runtime failed: the Python layer's ValueError / TypeError, and an
    OspError of any status but ERR_HIP.  Everything else -- OspError(ERR_HIP), any error of torch -- may be a GPU fault."""
    if isinstance(e, (ValueError, TypeError)):
        return True
    status = getattr(e, "status", None)
    return isinstance(e, RuntimeError) and status is not None and status != ERR_HIP


class ChainMismatch(AssertionError):
    def __init__(self, seed, dtype, step, kind, params, what):
        self.seed, self.dtype, self.step, self.kind, self.params, self.what = seed, np.dtype(dtype).name, step, kind, params, what
        super().__init__(f"CHAIN_MISMATCH seed={seed} dtype={self.dtype} step={step} op={kind} params={params}: {what}\n"
                         f"replay: python -m tests.result_chain --seeds {seed}")


# ---- a caller's output with margins ---------------------------------------------------------------------------------------------
# Bit patterns no result can be: NaNs with a payload of the driver's own (no input holds it, a copied NaN keeps its input's
# payload and a computed one has the hardware's), and a position no row has.
SENTINEL = {np.dtype(np.float32): np.uint32(0x7fc5eed5), np.dtype(np.float64): np.uint64(0x7ff85eed5eed5eed),
            np.dtype(np.int64): np.int64(np.iinfo(np.int64).min + 1),
            np.dtype(np.uint32): np.uint32(0xfeed5eed)}        # (an index list: tests/test_gpu_conv.py; no row of its cases)
MARGIN = 64                          # the fewest elements on either side of a caller's output


class MarginDamaged(Exception):
    """A backend's call changed an element outside the output it was given (the Chain makes a ChainMismatch of it)."""


class Frame:
    """A caller-owned dense output of ``shape`` as a slice in the middle of a buffer of SENTINELs, at least ``pad`` elements
    on either side.  The buffer is handled as BITS (uint32 / uint64, int64 for positions): ``new()`` makes it on the host,
    ``check(name, bits)`` raises MarginDamaged when a margin of the buffer after the call differs from the sentinel, and
    ``interior(bits)`` is the output in its dtype and shape."""

    def __init__(self, shape, dtype, pad=MARGIN):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n, self.pad = int(np.prod(self.shape, dtype=np.int64)), max(int(pad), MARGIN)
        self.sentinel = SENTINEL[self.dtype]

    def new(self):
        return np.full(self.n + 2 * self.pad, self.sentinel, self.sentinel.dtype)

    def check(self, name, bits):
        assert bits.dtype == self.sentinel.dtype and bits.shape == (self.n + 2 * self.pad,)
        for side, part in (("before", bits[:self.pad][::-1]), ("past", bits[self.pad + self.n:])):
            bad = np.flatnonzero(part != self.sentinel)
            if len(bad):       # (offset 1: the element next to the output)
                raise MarginDamaged(f"{name}: the margin {side} the caller's output of {self.n} elements changed at offset {bad[0] + 1} "
                                    f"{'before its first' if side == 'before' else 'past its last'} element: bits {int(part[bad[0]]):#x}, "
                                    f"the sentinel is {int(self.sentinel):#x} ({len(bad)} changed)")

    def interior(self, bits):
        return bits[self.pad:self.pad + self.n].view(self.dtype).reshape(self.shape)


def caller_outputs(kind, p, shape, k=None):
    """The caller-owned device outputs of a call as {name: (shape, dtype or None for the values' dtype, pad)}: what a backend
    frames.  ``shape`` is the input's."""
    M, N = shape
    out = {}
    if kind == "reduce" and p["out"] == "device":
        out["vector"] = ((M if p["axis"] == "rows" else N,), None, MARGIN)
    if kind in ("mxv", "mxv_arg") and p.get("out") == "caller":
        out["vector"] = ((M,), None, MARGIN)
    if kind == "mxv_arg" and p.get("out_arg") == "caller":
        out["arg"] = ((M,), np.int64, MARGIN)
    if kind == "mxd" and p.get("out") in ("caller", "x"):
        out["vector"] = ((M, p["k"]), None, max(MARGIN, p["k"]))
    return out


# ---- what the models say --------------------------------------------------------------------------------------------------------
_MEMO = [None, None, None, None]


def expected(kind, p, ins, aux):
    """The model's answer for one call.  ins: the (shape, (rowptr, col, val)) of the CSR inputs as read back; aux: the host
    arrays of the call (mask, vectors, lists, dense operands).  Returns a dict: ``csr`` (rowptr, col, val) and ``shape``, or
    ``vec`` -- a dense array of one or two dimensions, or the pair (vector or None, int64 vector) of mxv_arg --; ``nan_ok``
    (a mask, or one bool for all: where a NaN of the model only has to be a NaN); ``stats``.  The last answer is kept: the
    model backend and the driver ask for the same one."""
    key = (kind, repr(p), tuple(id(a) for _, csr in ins for a in csr), tuple(id(aux[k]) for k in sorted(aux)))
    if _MEMO[0] == key:
        return _MEMO[1]
    (M, N), x = ins[0]
    nnz = len(x[1])
    if kind == "apply_mask":
        mask = ins[1][1][:2] if p["mask"] in ("result", "self") else (aux["m_rowptr"], aux["m_col"])
        csr = bfs_model.apply_mask(*x, *mask, N, p["complement"])
        out = dict(csr=csr, shape=(M, N), nan_ok=False, stats=dict(nnz_in=nnz, nnz_mask=len(mask[1]), nnz_out=len(csr[1])))
    elif kind == "select":
        csr = truss_model.select(*x, p["op"], p["threshold"], p["diag"], p["fill"])
        out = dict(csr=csr, shape=(M, N), nan_ok=False, stats=dict(nnz_in=nnz, nnz_out=len(csr[1])))
    elif kind == "ewise":
        y = ins[1][1]
        plan = ewise_model.Plan(x, y, N)
        rowptr, col, val, computed = plan.result(p["mode"], p["op"])
        out = dict(csr=(rowptr, col, val), shape=(M, N), nan_ok=False if p["op"] in ewise_model.COPY_OPS else computed,
                   stats=dict(nnz_a=nnz, nnz_b=len(y[1]), nnz_both=plan.nnz_both, nnz_out=len(col)))
    elif kind == "inflate_prune":
        rowptr, col, val, st = mcl_model.inflate_prune(*x, p["power"], p["threshold"], p["max_per_row"])
        out = dict(csr=(rowptr, col, val), shape=(M, N), nan_ok=True,
                   stats={k: st[k] for k in ("nnz_in", "nnz_out", "rows_capped", "rows_rescued")})
    elif kind == "select_vertices":
        csr = vector_model.select_vertices(*x, aux.get("keep_rows"), aux.get("keep_cols"))
        out = dict(csr=csr, shape=(M, N), nan_ok=False, stats=dict(nnz_in=nnz, nnz_out=len(csr[1]), long_segments=0))
    elif kind == "apply_vectors":
        val, computed = vector_model.apply_vectors(*x, aux.get("rows"), p["row_op"], aux.get("cols"), p["col_op"])
        out = dict(csr=(x[0], x[1], val), shape=(M, N), nan_ok=bool(computed), stats=dict(nnz_in=nnz, nnz_out=nnz, long_segments=0))
    elif kind == "transpose":
        path = 0 if nnz == 0 else 1 if M <= ROWMASK_MAX else 2
        out = dict(csr=transpose_model.transpose(*x, N), shape=(N, M), nan_ok=False,
                   stats=dict(nnz=nnz, path=path, passes=transpose_model.passes(N) if path == 2 else 0))
    elif kind == "mxm":
        (_, Nb), y = ins[1]
        csr, st = semiring_model.mxm(x, y, Nb, p["add"], p["mul"])
        out = dict(csr=csr, shape=(M, Nb), nan_ok=True, stats=dict(st, nnz_a=nnz, nnz_b=len(y[1])))
    elif kind == "matmul":
        (_, Nb), y = ins[1]
        left = transpose_model.transpose(*x, N) if p["self_transposed"] else x
        csr, st = semiring_model.mxm(left, y, Nb, "plus", "times")
        out = dict(csr=csr, shape=(N if p["self_transposed"] else M, Nb), nan_ok=True, stats=dict(nnz_out=st["nnz_out"]),
                   products=st["products"])
    elif kind == "reduce":
        vec, nlong = vector_model.reduce(*x, N, p["axis"], p["op"])
        out = dict(vec=vec, nan_ok=p["op"] == "plus", stats=dict(nnz_in=nnz, nnz_out=len(vec), long_segments=nlong))
    elif kind == "mxv":
        vec, nlong = mxv_model.mxv(*x, aux.get("x"), p["add"], p["mul"])
        out = dict(vec=vec, nan_ok=p["add"] == "plus", stats=dict(nnz_in=nnz, nnz_out=M, long_segments=nlong))
    elif kind == "extract":
        rows, cols = aux.get("rows"), aux.get("cols")
        if cols is None or extract_model.is_ascending(cols):
            csr, st = extract_model.extract(*x, N, rows, cols)
            stats = dict(nnz_in=nnz, nnz_gathered=st["nnz_gathered"], nnz_out=st["nnz_out"], composed=False)
        else:       # (the composed path ends in a row gather of everything the columns kept)
            csr = extract_model.extract_any(*x, N, rows, cols)
            stats = dict(nnz_in=nnz, nnz_gathered=len(csr[1]), nnz_out=len(csr[1]), composed=True)
        out = dict(csr=csr, shape=(M if rows is None else len(rows), N if cols is None else len(cols)), nan_ok=False, stats=stats)
    elif kind == "build":
        vals = aux.get("b_vals")
        csr, st, layout = build_model.build(M, N, aux["b_rows"], aux["b_cols"], vals, p["dup"], x[2].dtype)
        # (a NaN that dup="plus" computed: the value of a coordinate that repeats)
        out = dict(csr=csr, shape=(M, N), nan_ok=(layout["length"] > 1) if p["dup"] == "plus" and vals is not None else False, stats=st,
                   layout=layout)
    elif kind == "mxd":
        k = p["k"]
        Y, nlong = mxd_model.mxd(*x, aux.get("X"), p["add"], p["mul"], k=k)
        stats = dict(nnz_in=nnz, cols=k, long_segments=nlong, lanes_per_row=mxd_model.lanes_per_row(k))
        if not nlong:       # (with a long row the count needs the scan's own, a device figure)
            stats["launches"] = mxd_model.expected_launches(x[0])
        out = dict(vec=Y, nan_ok=p["add"] == "plus", stats=stats)
    elif kind == "sddmm":
        k = p["k"]
        X = aux.get("X")
        val, computed = sddmm_model.sddmm(*x, X, X if p["y_is_x"] else aux.get("Y"), p["add"], p["mul"], p["accum"], k=k)
        out = dict(csr=(x[0], x[1], val), shape=(M, N), nan_ok=bool(computed),
                   stats=dict(nnz_in=nnz, nnz_out=nnz, cols=k, lanes_per_entry=sddmm_model.lanes_per_entry(k),
                              launches=sddmm_model.expected_launches(nnz)))
    elif kind == "mxv_arg":
        y, arg, nlong, without = mxv_arg_model.mxv_arg(*x, aux.get("x"), p["add"], p["mul"])
        out = dict(vec=(y if p["values"] else None, arg), nan_ok=False, stats=dict(nnz_in=nnz, long_segments=nlong, rows_without=without))
    else:
        raise KeyError(kind)
    _MEMO[:] = [key, out, ins, aux]       # (the inputs are kept alive with it: an id is never reused under the key)
    return out


# ---- backends -------------------------------------------------------------------------------------------------------------------
class _Held:
    """A result of the model backend."""
    def __init__(self, shape, csr):
        self.shape, self.csr = shape, csr


class ModelBackend:
    """The models themselves behind the backend interface: upload / read / close of results, stage / unstage of the dense
    arrays of a call, and run(kind, params, handles, staged) -> (handle or vector, stats)."""
    name = "model"

    def upload(self, ncol, csr):
        return _Held((len(csr[0]) - 1, ncol), csr)

    def read(self, h):
        return h.shape, h.csr

    def close(self, h):
        h.csr = None

    def stage(self, aux, space):
        return dict(aux)

    def unstage(self, staged, space):
        return dict(staged)

    def sync(self):
        pass

    margin_hook = None     # test-only: called as hook(kind, p, {name: (Frame, its buffer's bits)}) before the margins are checked

    def run(self, kind, p, handles, staged):
        want = expected(kind, p, [self.read(h) for h in handles], staged)
        if "vec" not in want:
            return _Held(want["shape"], want["csr"]), dict(want["stats"])
        # a caller's output goes through a Frame as on the GPU, so that the margin check itself runs here too
        parts = dict(zip(("vector", "arg"), want["vec"])) if isinstance(want["vec"], tuple) else {"vector": want["vec"]}
        framed = {}
        for name, (shape, dtype, pad) in caller_outputs(kind, p, handles[0].shape).items():
            fr = Frame(shape, dtype or parts[name].dtype, pad)
            bits = fr.new()
            fr.interior(bits)[...] = parts[name]
            framed[name] = (fr, bits)
        if framed and self.margin_hook is not None:
            self.margin_hook(kind, p, framed)
        for name, (fr, bits) in framed.items():
            fr.check(name, bits)
            parts[name] = fr.interior(bits).copy()
        return ((parts["vector"], parts["arg"]) if isinstance(want["vec"], tuple) else parts["vector"]), dict(want["stats"])


class GpuBackend:
    """CsrResult behind the backend interface (one library context, given or its own)."""
    name = "gpu"

    def __init__(self, ctx=None):
        import torch
        from outerspace_amd import spgemm as S
        from outerspace_amd import _lib
        assert _lib.ERR_HIP == ERR_HIP
        self.torch, self.own = torch, ctx is None
        self.ctx = S.Context(0) if ctx is None else ctx
        self.dev = f"cuda:{self.ctx.device}"

    def finish(self):
        if self.own:
            self.ctx.close()

    def upload(self, ncol, csr):
        return self.ctx.merge_csr_parts(len(csr[0]) - 1, ncol, [csr])

    def read(self, h):
        h._host = None                      # a fresh copy from the device, every time
        rowptr, col, val = h.to_host()
        h._host = None
        return h.shape, (rowptr, col, val)

    def close(self, h):
        h.close()

    def _dev(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        if a.size == 0 and a.ndim == 2:     # (a dense matrix without rows or columns: a tensor of that shape)
            return self.torch.empty(a.shape, dtype=self.torch.from_numpy(a.ravel()[:0].copy()).dtype, device=self.dev)
        if a.size == 0:
            return self.torch.empty(1, dtype=self.torch.from_numpy(a[:0].copy()).dtype, device=self.dev)
        return self.torch.from_numpy(a.copy()).to(self.dev)   # (a copy of the bytes: NaN payloads survive)

    def stage(self, aux, space):
        if space != "device":
            return dict(aux)
        staged = {k: (v.dtype, len(v), self._dev(v)) for k, v in aux.items()}
        self.torch.cuda.synchronize(self.dev)
        return staged

    def unstage(self, staged, space):
        if space != "device":
            return dict(staged)
        out = {}
        for k, (dt, n, t) in staged.items():
            a = t.cpu().numpy()[:n]
            out[k] = a.view(np.uint32) if dt == np.uint32 else a
        return out

    def sync(self):
        self.torch.cuda.synchronize(self.dev)

    def run(self, kind, p, handles, staged):
        x = handles[0]
        space = p.get("space", "host")
        arg = (lambda k: None if k not in staged else staged[k][2]) if space == "device" else (lambda k: staged.get(k))
        if kind == "apply_mask":
            if p["mask"] in ("result", "self"):
                return x.apply_mask(handles[1], complement=p["complement"])
            m = (arg("m_rowptr"), arg("m_col"))
            m = (m[0].data_ptr(), m[1].data_ptr()) if space == "device" else m
            return x.apply_mask(m, complement=p["complement"], space=space)
        if kind == "select":
            return x.select(p["op"], p["threshold"], diag=p["diag"], fill=p["fill"])
        if kind == "ewise":
            return x.ewise(handles[1], p["mode"], p["op"])
        if kind == "inflate_prune":
            return x.inflate_prune(p["power"], p["threshold"], p["max_per_row"])
        if kind == "select_vertices":
            return x.select_vertices(arg("keep_rows"), arg("keep_cols"), space=space)
        if kind == "apply_vectors":
            return x.apply_vectors(arg("rows"), p["row_op"], arg("cols"), p["col_op"], space=space)
        if kind == "transpose":
            return x.transpose()
        if kind == "mxm":
            return x.mxm(handles[1], p["add"], p["mul"])
        if kind == "matmul":
            res = x.matmul(handles[1], self_transposed=p["self_transposed"])
            return res, dict(nnz_out=res.info["nnz_c"])
        # the caller's device outputs, each in the middle of a buffer of sentinels
        framed = {name: self._framed(Frame(shape, dtype or x.dtype, pad)) for name, (shape, dtype, pad) in caller_outputs(kind, p, x.shape).items()}
        out = {name: view for name, (_, _, view) in framed.items()}
        host = lambda t: t if t is None or isinstance(t, np.ndarray) else t.cpu().numpy()
        lst = lambda k: None if k not in staged else staged[k][2][:staged[k][1]] if space == "device" else staged[k]   # (a list: its length counts)
        if kind == "reduce":
            if p["out"] == "host":
                return x.reduce(p["axis"], p["op"])
            _, st = x.reduce(p["axis"], p["op"], out=out["vector"])
            return self._unframe(framed)["vector"], st
        if kind == "mxv":
            y, st = x.mxv(arg("x"), p["add"], p["mul"], out=out.get("vector"), space=space)
            return (self._unframe(framed)["vector"] if framed else host(y)), st
        if kind == "mxv_arg":
            y, a, st = x.mxv_arg(arg("x"), p["add"], p["mul"], out=out.get("vector"), out_arg=out.get("arg"), space=space, values=p["values"])
            back = self._unframe(framed)
            return (back.get("vector", host(y)), back.get("arg", host(a))), st
        if kind == "mxd":
            X = arg("X")
            if p["out"] == "x":                 # out is X: the operand itself lies in the frame
                out["vector"].copy_(X)
                self.torch.cuda.synchronize(self.dev)
                X = out["vector"]
            y, st = x.mxd(X, p["add"], p["mul"], out=out.get("vector"), space=space, k=p["k"] if X is None else None)
            return (self._unframe(framed)["vector"] if framed else host(y)), st
        if kind == "sddmm":
            X = arg("X")
            return x.sddmm(X, X if p["y_is_x"] else arg("Y"), p["add"], p["mul"], p["accum"], space=space, k=p["k"] if X is None and arg("Y") is None else None)
        if kind == "extract":
            if p["permute"]:
                return x.permute(lst("rows"), space=space)
            return x.extract(lst("rows"), lst("cols"), space=space)
        if kind == "build":
            return self.ctx.build(*x.shape, lst("b_rows"), lst("b_cols"), lst("b_vals"), dup=p["dup"], dtype=x.dtype, space=space)
        raise KeyError(kind)

    def _framed(self, fr):
        """(the Frame, its buffer on the device as bits, the output's view in it)."""
        torch = self.torch
        tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int64): torch.int64}[fr.dtype]
        bits = torch.from_numpy(fr.new().view(np.int32 if fr.dtype.itemsize == 4 else np.int64)).to(self.dev)
        view = bits.view(tdt)[fr.pad:fr.pad + fr.n].view(fr.shape)
        torch.cuda.synchronize(self.dev)
        return fr, bits, view

    def _unframe(self, framed):
        """The outputs of the frames as host arrays, their margins checked (MarginDamaged)."""
        back = {}
        for name, (fr, bits, _) in framed.items():
            b = bits.cpu().numpy().view(fr.sentinel.dtype)
            fr.check(name, b)
            back[name] = fr.interior(b).copy()
        return back


# ---- the starting operands ----------------------------------------------------------------------------------------------------------
def _csr_from_lengths(rng, lengths, ncol, val):
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cols = [np.sort(rng.choice(ncol, size=int(k), replace=False)) for k in lengths]
    col = (np.concatenate(cols) if cols else np.zeros(0)).astype(np.uint32)
    return rowptr, col, val(len(col))


def class_lengths(n):
    """The row lengths at which a kernel of the surface takes another path, and one row of about 3000."""
    edge = {0, 1, 63, 64, 65, SHORT_CAP - 1, SHORT_CAP, SHORT_CAP + 1}
    for b in (CHUNK, BLOCK):
        edge |= {b - 1, b, b + 1}
    return sorted(edge) + [min(3000, n - 13)]


def _lengths(rng, nrow, ncol, short_max):
    """Empty rows first and last, the class lengths in a random order among short random rows; nnz no multiple of 64."""
    cls = class_lengths(ncol)
    assert nrow >= len(cls) + 4
    body = np.concatenate([cls, rng.integers(0, short_max + 1, nrow - len(cls) - 4)])
    lengths = np.concatenate([[0, 0], rng.permutation(body), [0, 0]]).astype(np.int64)
    if lengths.sum() % 64 == 0:
        lengths[int(np.flatnonzero((lengths > 1) & (lengths < 60))[0])] += 1     # (one of the short random rows)
    return lengths


def starting_operands(seed, dt):
    """[(name, ncol, csr)]: a FRONTIER (at most 64 rows, 2^16 columns: transpose takes its row-mask path), a square operand A
    of more than 64 rows (the sort path) with am._special's values planted and one all-NaN row, and a square operand P of A's
    shape with small positive values and no special ones (what inflate_prune takes).  Row patterns depend on the seed
    alone, so both dtypes of a seed run on one structure."""
    rng = np.random.default_rng([seed, 1])
    values = lambda k: (rng.standard_normal(k) * 10.0 ** rng.integers(-2, 3, k)).astype(dt)
    n = int(rng.integers(2200, 3101))
    n += n % 64 == 0
    mf = int(rng.integers(len(class_lengths(FRONTIER_NCOL)) + 6, ROWMASK_MAX))      # (below 64: no multiple of it)
    F = _csr_from_lengths(rng, _lengths(rng, mf, FRONTIER_NCOL, 40), FRONTIER_NCOL, values)
    A = _csr_from_lengths(rng, _lengths(rng, n, n, 8), n, values)
    sp_ = _special(dt)
    val = A[2]
    where = rng.choice(len(val), size=3 * len(sp_), replace=False)
    val[where] = np.resize(sp_, len(where))
    lens = np.diff(A[0])
    r = int(np.flatnonzero(lens == 2)[0]) if np.any(lens == 2) else int(np.flatnonzero(lens == 1)[0])
    val[A[0][r]:A[0][r + 1]] = sp_[0]                                                # a row of NaNs only
    plens = rng.integers(0, 25, n)
    plens[[0, 1, n - 1]] = 0
    plens[rng.choice(np.arange(2, n - 1), 3, replace=False)] = [63, 64, 65]
    if plens.sum() % 64 == 0:
        plens[int(np.flatnonzero((plens > 1) & (plens < 24))[0])] += 1                # (one of the short random rows)
    P = _csr_from_lengths(rng, plens, n, lambda k: (rng.random(k) * 0.95 + 0.05).astype(dt))
    for name, ncol, csr in (("F", FRONTIER_NCOL, F), ("A", n, A), ("P", n, P)):
        M, nnz = len(csr[0]) - 1, len(csr[1])
        assert 1 <= M <= 3200 and nnz <= 60000 and csr[0][1] == 0 and csr[0][-2] == nnz, (name, M, nnz)
        assert M % 64 and nnz % 64, (name, M, nnz)
    assert mf <= ROWMASK_MAX < n
    return [("F", FRONTIER_NCOL, F), ("A", n, A), ("P", n, P)]


# ---- one chain ------------------------------------------------------------------------------------------------------------------------
class _Live:
    def __init__(self, h, shape, made_by):
        self.h, self.shape, self.made_by = h, shape, made_by


class Coverage:
    """Counts computed from the inputs and the models (never from device stats), per dtype."""

    def __init__(self):
        self.count = {np.dtype(dt).name: collections.Counter() for dt in DTYPES}
        self.pairs = collections.Counter()
        self.drawn = self.steps = self.redraws = 0

    @property
    def skipped(self):
        """Legal calls that were drawn and did not get through the whole comparison.  The driver has no path that drops a
        drawn call (an illegal draw is a redraw, a mismatch ends the run), so a run that finishes reports 0; the figure is the
        difference of two counters kept at the two ends of a step, so that a path which drops one would show."""
        return self.drawn - self.steps

    REQUIRED = ([f"op:{k}" for k in KINDS] +
                ["transpose:rowmask", "transpose:sort", "mxv:long", "mxv:short", "reduce:long", "reduce:short", "reduce:cols",
                 "mxm:long_row", "mxm:all_short", "in:nnz0", "out:nnz0", "ewise:self", "pair:different",
                 "extract:rows_dup", "extract:cols_ascending", "extract:composed", "extract:permute", "extract:empty_list",
                 "build:no_repeat", "build:long_run", "build:run_over_chunk", "build:novals",
                 "mxd:k1", "mxd:packed", "mxd:tiles", "mxd:long", "mxd:short", "mxd:out_is_x",
                 "sddmm:k0", "sddmm:tiles", "sddmm:accum_reads_value", "sddmm:y_is_x",
                 "mxv_arg:long", "mxv_arg:short", "mxv_arg:tie", "mxv_arg:row_without", "mxv_arg:values_false",
                 "in:dim0", "out:dim0", "out:caller_tensor"] +
                # every kind but extract on an input of zero rows or zero columns
                [f"dim0:{k}" for k in KINDS if k != "extract"] + [
                 # where each planted defect of tests/test_result_chain_cpu.py finds something to damage (the conditions
                 # above serve the defects of extract, mxv_arg and the margins as well)
                 "select:nonempty", "ewise:nonempty", "mxv:zero", "transpose:row_of_two", "reduce:all_nan_row",
                 "build:ordered_run", "mxd:corner_no_nan", "sddmm:accum_ordered", "in:dim0_to_csr"])

    def missing(self):
        """The conditions of the default seed list that this run does not meet."""
        miss = [f"{dt}:{k}" for dt, c in self.count.items() for k in self.REQUIRED if c[k] < 1]
        miss += [f"both:{k}<5" for k in KINDS if sum(c[f"op:{k}"] for c in self.count.values()) < 5]
        if self.skipped:
            miss.append(f"skipped={self.skipped}")
        return miss

    def matrix(self):
        names = ["upload"] + KINDS
        w = max(len(k) for k in names)
        lines = ["input made by (rows) -> operation applied to it (columns: " + " ".join(f"{i}={k}" for i, k in enumerate(KINDS)) + ")"]
        lines.append(" " * w + "".join(f"{i:4d}" for i in range(len(KINDS))))
        for a in names:
            lines.append(f"{a:>{w}}" + "".join(f"{self.pairs[(a, b)]:4d}" for b in KINDS))
        return "\n".join(lines)

    def different_pairs(self):
        return sum(1 for (a, b), c in self.pairs.items() if c and a != "upload" and a != b)

    def summary(self):
        parts = []
        for dt, c in self.count.items():
            parts.append(dt + "[" + " ".join(f"{k.split(':', 1)[1] if k.startswith('op:') else k}={c[k]}" for k in self.REQUIRED) + "]")
        return " ".join(parts)


class Chain:
    def __init__(self, backend, seed, dt, cov):
        self.be, self.seed, self.dt, self.cov = backend, seed, dt, cov
        self.c = cov.count[np.dtype(dt).name]
        self.rng = np.random.default_rng([seed, 2])
        self.live = []
        self.step = -1
        self._host = {}

    # -- reading
    def host(self, L):
        """(shape, csr) of a live result as the device holds it now (one read-back per step and result)."""
        if id(L) not in self._host:
            self._host[id(L)] = self.be.read(L.h)
        return self._host[id(L)]

    def pick(self, ok=lambda L: True):
        cand = [L for L in self.live if ok(L)]
        if not cand:
            return None
        w = np.array([1.0 if L.made_by == "upload" else 3.0 for L in cand])     # (a device-made result three times as often)
        return cand[int(self.rng.choice(len(cand), p=w / w.sum()))]

    def choice(self, seq, p=None):
        return seq[int(self.rng.choice(len(seq), p=p))]

    def vector(self, n, positive=False):
        if positive:
            return (self.rng.random(n) * 0.95 + 0.05).astype(self.dt)
        v = self.rng.standard_normal(n).astype(self.dt)
        if n == 0:
            return v
        sp_ = _special(self.dt)
        where = self.rng.choice(n, size=min(n, max(len(sp_), n // 30)), replace=False)
        v[where] = np.resize(sp_, len(where))
        return v

    # -- the draws: (params, inputs, aux) of a legal call, or None (the caller redraws)
    def draw_apply_mask(self):
        x = self.pick()
        variant = self.choice(["host", "device", "result", "self"], [0.3, 0.3, 0.25, 0.15])
        p = dict(mask=variant, complement=bool(self.rng.integers(2)))
        if variant == "result":
            m = self.pick(lambda L: L is not x and L.shape == x.shape)
            if m is None:
                return None
            return p, [x, m], {}
        if variant == "self":
            return p, [x, x], {}
        (M, N), (rowptr, col, _) = self.host(x)
        share, extra = self.choice([0.0, 0.5, 1.0]), self.choice([0.0, 0.5])
        if M == 0 or N == 0:                    # (no coordinate to name: the only mask of this shape)
            m_rowptr, m_col = np.zeros(M + 1, np.int64), np.zeros(0, np.uint32)
        else:
            m_rowptr, m_col = _mask_for(rowptr, col, N, seed=int(self.rng.integers(1 << 30)), share=share, extra=extra,
                                        edges=bool(self.rng.integers(2)) and N >= 4)
        p["space"] = variant
        return p, [x], dict(m_rowptr=np.ascontiguousarray(m_rowptr, np.int64), m_col=np.ascontiguousarray(m_col, np.uint32))

    def draw_select(self):
        x = self.pick()
        _, (_, _, val) = self.host(x)
        op = self.choice(truss_model.OPS)
        thr, diag = 0.0, 0
        if op in truss_model.VALUE_OPS:
            kind = self.choice(["entry", "zero", "nan", "inf"], [0.6, 0.2, 0.1, 0.1])
            thr = {"zero": 0.0, "nan": float("nan"), "inf": float("inf")}.get(kind, 0.0)
            if kind == "entry" and len(val):
                thr = float(val[int(self.rng.integers(len(val)))])
        else:
            diag = int(self.choice([-2, -1, 0, 1, 3, 1 << 33]))
        fill = self.choice([None, None, 1.0, -0.0, 0.5])
        return dict(op=op, threshold=thr, diag=diag, fill=fill), [x], {}

    def draw_ewise(self):
        x = self.pick()
        y = x if self.rng.random() < 0.25 else self.pick(lambda L: L.shape == x.shape)
        mode = self.choice(ewise_model.MODES)
        op = self.choice(ewise_model.UNION_OPS if mode == "union" else ewise_model.OPS)
        return dict(mode=mode, op=op, same=y is x), [x, y], {}

    def _mcl_ok(self, L):
        if L.shape[0] > MCL_MAX_ROWS:
            return False
        val = self.host(L)[1][2]
        return bool(np.all(np.isfinite(val)) and np.all(val >= 0))

    def draw_inflate_prune(self):
        x = self.pick(self._mcl_ok)
        if x is None:
            return None
        val = self.host(x)[1][2]
        thr = 0.0 if self.rng.random() < 0.4 or not len(val) else float(val[int(self.rng.integers(len(val)))])
        return dict(power=self.choice([1.0, 2.0]), threshold=thr, max_per_row=int(self.choice([0, 0, 1, 7, 64, 1000]))), [x], {}

    def draw_select_vertices(self):
        x = self.pick()
        M, N = x.shape
        aux = {}
        sides = self.choice(["rows", "cols", "both"])
        for key, n, on in (("keep_rows", M, sides != "cols"), ("keep_cols", N, sides != "rows")):
            if on:
                share = self.choice([0.0, 0.5, 0.9, 1.0], [0.1, 0.4, 0.4, 0.1])
                aux[key] = ((self.rng.random(n) < share) * self.rng.choice([1, 2, 255], n)).astype(np.uint8)
        return dict(sides=sides, space=self.choice(["host", "device"])), [x], aux

    def draw_apply_vectors(self):
        x = self.pick()
        M, N = x.shape
        if self.rng.random() < 0.3:     # every value becomes a small positive number: what inflate_prune takes
            return dict(row_op="second", col_op=None, space=self.choice(["host", "device"]), positive=True), [x], dict(rows=self.vector(M, True))
        ops = [None] + vector_model.APPLY_OPS
        row_op, col_op = self.choice(ops), self.choice(ops)
        if row_op is None and col_op is None:
            col_op = self.choice(vector_model.APPLY_OPS)
        aux = {}
        if row_op is not None:
            aux["rows"] = self.vector(M)
        if col_op is not None:
            aux["cols"] = self.vector(N)
        return dict(row_op=row_op, col_op=col_op, space=self.choice(["host", "device"])), [x], aux

    def draw_transpose(self):
        return {}, [self.pick()], {}

    def _products(self, x, y, self_transposed=False):
        (_, (xp, xc, _)), (_, (yp, _, _)) = self.host(x), self.host(y)
        ylen = np.diff(yp)
        return int((np.diff(xp) * ylen).sum()) if self_transposed else int(ylen[xc.astype(np.int64)].sum())

    def draw_mxm(self):
        x = self.pick()
        y = self.pick(lambda L: L.shape[0] == x.shape[1])
        if y is None or self._products(x, y) > PRODUCT_CAP:
            return None
        return dict(add=self.choice(semiring_model.ADD_OPS), mul=self.choice(semiring_model.MUL_OPS), same=y is x), [x, y], {}

    def draw_matmul(self):
        x = self.pick()
        st = bool(self.rng.integers(2))
        y = self.pick(lambda L: L.shape[0] == x.shape[0 if st else 1])
        if y is None or self._products(x, y, st) > PRODUCT_CAP:
            return None
        return dict(self_transposed=st, same=y is x), [x, y], {}

    def draw_reduce(self):
        return dict(axis=self.choice(vector_model.AXES), op=self.choice(vector_model.REDUCE_OPS), out=self.choice(["host", "device"])), [self.pick()], {}

    def draw_mxv(self):
        x = self.pick()
        p = dict(add=self.choice(mxv_model.ADD_OPS), mul=self.choice(mxv_model.MUL_OPS), space=self.choice(["host", "device"]))
        p["out"] = self.caller_out(p["space"])
        if p["mul"] == "first" and self.rng.random() < 0.5:
            return dict(p, x=None), [x], {}
        return p, [x], dict(x=self.vector(x.shape[1]))

    def caller_out(self, space):
        """Whether the call fills a device tensor of the caller's ("caller") or allocates its output (None)."""
        return "caller" if space == "device" and self.rng.random() < 0.5 else None

    def index_list(self, n, variants):
        """(variant, uint32 list or None) over [0, n): one of ``variants`` -- "all" (None), "ascending" (a strictly ascending
        subset), "dup" (any order, repeats), "perm" (a permutation) --, rarely "empty"; a dimension of zero has no other list."""
        variant = "empty" if self.rng.random() < 0.12 else self.choice(variants)
        if n == 0 and variant != "all":
            variant = "empty"
        if variant == "all":
            return variant, None
        if variant == "empty":
            idx = np.zeros(0, np.int64)
        elif variant == "ascending":
            idx = np.flatnonzero(self.rng.random(n) < self.choice([0.1, 0.5, 0.9]))
            idx = idx if len(idx) else np.array([int(self.rng.integers(n))])
        elif variant == "perm":
            idx = self.rng.permutation(n)
        else:
            idx = self.rng.integers(0, n, int(self.rng.integers(2, max(3, n + n // 4))))
            idx[int(self.rng.integers(1, len(idx)))] = idx[0]        # (at least one index twice)
        return variant, idx.astype(np.uint32)

    def draw_extract(self):
        x = self.pick()
        M, N = x.shape
        space = self.choice(["host", "device"])
        if M == N and self.rng.random() < 0.2:
            perm = self.rng.permutation(M).astype(np.uint32)
            return dict(permute=True, rows="perm", cols="perm", space=space), [x], dict(rows=perm, cols=perm)
        rv, rows = self.index_list(M, ["all", "ascending", "dup"])
        cv, cols = self.index_list(N, ["all", "ascending", "ascending", "perm", "dup"])
        aux = {k: v for k, v in (("rows", rows), ("cols", cols)) if v is not None}
        return dict(permute=False, rows=rv, cols=cv, space=space), [x], aux

    def draw_build(self):
        x = self.pick()
        (M, N), (rowptr, col, val) = self.host(x)
        nnz = len(col)
        r = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr))
        c = col.astype(np.int64)
        order = self.rng.permutation(nnz)
        r, c, v = r[order], c[order], val[order]
        repeats = self.choice(["none", "few", "long_run", "over_chunk"]) if nnz else "none"
        if repeats != "none":
            # (coordinate of the list, copies of it in all): the extra copies get fresh values, and the list is shuffled again
            copies = {"few": [int(self.rng.integers(2, 4)) for _ in range(min(5, nnz))],
                      "long_run": [build_model.LONG_RUN - 1, build_model.LONG_RUN, build_model.LONG_RUN + 1][:min(3, nnz)],
                      "over_chunk": [CHUNK + 1]}[repeats]
            which = self.rng.choice(nnz, size=len(copies), replace=False)
            extra = np.repeat(which, np.array(copies) - 1)
            r, c, v = np.concatenate([r, r[extra]]), np.concatenate([c, c[extra]]), np.concatenate([v, self.vector(len(extra))])
            order = self.rng.permutation(len(r))
            r, c, v = r[order], c[order], v[order]
        dup = self.choice([d for d in build_model.DUP_OPS if d != "error" or repeats == "none"])
        p = dict(dup=dup, repeats=repeats, vals=bool(self.rng.random() >= 0.2), space=self.choice(["host", "device"]))
        aux = dict(b_rows=r.astype(np.uint32), b_cols=c.astype(np.uint32))
        if p["vals"]:
            aux["b_vals"] = np.ascontiguousarray(v)
        return p, [x], aux

    def dense_k(self, ks, *counts):
        """k from ``ks``, redrawn while a dense operand or the products of the call would exceed DENSE_CAP elements."""
        while True:
            k = int(self.choice(ks))
            if max(counts) * k <= DENSE_CAP:
                return k
            self.cov.redraws += 1

    def draw_mxd(self):
        x = self.pick()
        (M, N), (_, col, _) = self.host(x)
        k = self.dense_k(mxd_model.KS, len(col), M, N)
        p = dict(add=self.choice(mxd_model.ADD_OPS), mul=self.choice(mxd_model.MUL_OPS), k=k, space=self.choice(["host", "device"]))
        p["out"] = self.caller_out(p["space"])
        if p["mul"] == "first" and self.rng.random() < 0.5:
            return dict(p, X=None), [x], {}
        if M == N and p["space"] == "device" and self.rng.random() < 0.4:
            p["out"] = "x"
        return p, [x], dict(X=self.vector(N * k).reshape(N, k))

    def draw_sddmm(self):
        x = self.pick()
        (M, N), (_, col, _) = self.host(x)
        k = self.dense_k(sddmm_model.KS, len(col), M, N)
        p = dict(add=self.choice(sddmm_model.ADD_OPS), mul=self.choice(sddmm_model.MUL_OPS), accum=self.choice(sddmm_model.ACCUM_OPS + [None]),
                 k=k, y_is_x=False, space=self.choice(["host", "device"]))
        aux = dict(X=self.vector(M * k).reshape(M, k))
        if M == N and self.rng.random() < 0.3:
            return dict(p, y_is_x=True), [x], aux
        aux["Y"] = self.vector(N * k).reshape(N, k)
        if p["mul"] in ("first", "second") and self.rng.random() < 0.5:       # (the operand mul does not read)
            del aux["Y" if p["mul"] == "first" else "X"]
            p["none"] = "Y" if p["mul"] == "first" else "X"
        return p, [x], aux

    def draw_mxv_arg(self):
        x = self.pick()
        N = x.shape[1]
        p = dict(add=self.choice(mxv_arg_model.ADD_OPS), mul=self.choice(mxv_arg_model.MUL_OPS), space=self.choice(["host", "device"]),
                 values=bool(self.rng.random() < 0.7))
        p["out"] = self.caller_out(p["space"]) if p["values"] else None
        p["out_arg"] = self.caller_out(p["space"])
        if p["mul"] == "first" and self.rng.random() < 0.5:
            return dict(p, x=None), [x], {}
        v = self.vector(N)
        if self.rng.random() < 1 / 3:       # at most four distinct values, both zeros and a NaN among them: tied best products
            pool = np.array([0.0, -0.0, np.nan, self.rng.standard_normal()], self.dt)
            v = pool[self.rng.choice(4, size=N, p=[0.2, 0.2, 0.1, 0.5])]
            p["few_values"] = True
        return p, [x], dict(x=v)

    # -- comparing
    def fail(self, kind, p, what):
        raise ChainMismatch(self.seed, self.dt, self.step, kind, p, what)

    def same_ints(self, kind, p, name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            self.fail(kind, p, f"{name}: {got.shape[0] if got.ndim else got} entries, the model has {want.shape[0]}")
        bad = np.flatnonzero(got != want)
        if len(bad):
            self.fail(kind, p, f"{name}[{bad[0]}] = {got[bad[0]]}, the model has {want[bad[0]]} ({len(bad)} differ)")

    def same_values(self, kind, p, name, got, want, nan_ok):
        got, want = np.asarray(got), np.asarray(want)
        if got.dtype != want.dtype or got.shape != want.shape:
            self.fail(kind, p, f"{name}: {got.dtype}{got.shape}, the model has {want.dtype}{want.shape}")
        got, want = got.ravel(), want.ravel()                   # (a dense matrix: the position reported is row * k + column)
        nan_ok = nan_ok.ravel() if isinstance(nan_ok, np.ndarray) else nan_ok
        loose = np.isnan(want) & nan_ok
        # (a NaN that only has to be a NaN may still not be the sentinel a caller's output was filled with: nothing wrote there)
        bad = np.flatnonzero(np.where(loose, ~np.isnan(got) | (_bits(got) == SENTINEL[got.dtype]), _bits(got) != _bits(want)))
        if len(bad):
            i = bad[0]
            self.fail(kind, p, f"{name}[{i}] = {got[i]!r} (bits {int(_bits(got)[i]):#x}), the model has {want[i]!r} "
                               f"(bits {int(_bits(want)[i]):#x}) ({len(bad)} differ)")

    def same_dense(self, kind, p, got, want, nan_ok):
        """A dense output: an array of one or two dimensions, or mxv_arg's pair (vector or None, positions)."""
        if not isinstance(want, tuple):
            return self.same_values(kind, p, "vector", got, want, nan_ok)
        if not isinstance(got, tuple) or len(got) != 2:
            self.fail(kind, p, f"the call returned {type(got).__name__}, the model has a pair")
        if want[0] is None or got[0] is None:
            if want[0] is not None or got[0] is not None:
                self.fail(kind, p, f"vector: {'None' if got[0] is None else 'an array'}, the model has {'None' if want[0] is None else 'an array'}")
        else:
            self.same_values(kind, p, "vector", got[0], want[0], nan_ok)
        if np.asarray(got[1]).dtype != np.int64:
            self.fail(kind, p, f"arg: {np.asarray(got[1]).dtype}, the model has int64")
        self.same_ints(kind, p, "arg", got[1], want[1])

    # -- counting
    def note(self, kind, p, inputs, ins, aux, want):
        c = self.c
        c[f"op:{kind}"] += 1
        for L in {id(L): L for L in inputs}.values():
            self.cov.pairs[(L.made_by, kind)] += 1
            if L.made_by not in ("upload", kind):
                c["pair:different"] += 1
        (M, N), x = ins[0]
        lens = np.diff(x[0])
        if any(len(csr[1]) == 0 for _, csr in ins):
            c["in:nnz0"] += 1
        if "csr" in want and len(want["csr"][1]) == 0:
            c["out:nnz0"] += 1
        if kind == "transpose" and len(x[1]):
            c["transpose:rowmask" if M <= ROWMASK_MAX else "transpose:sort"] += 1
        if kind in ("mxv", "reduce"):
            c[f"{kind}:long" if want["stats"]["long_segments"] else f"{kind}:short"] += 1
            if kind == "reduce" and p["axis"] == "cols":
                c["reduce:cols"] += 1
        if kind == "mxm" and want["stats"]["products"]:
            c["mxm:long_row" if want["stats"]["long_rows"] else "mxm:all_short"] += 1
        if kind == "ewise" and p["same"]:
            c["ewise:self"] += 1
        # (the targets of the planted defects)
        if kind in ("select", "ewise") and len(want["csr"][1]):
            c[f"{kind}:nonempty"] += 1
        if kind == "mxv" and np.any(want["vec"] == 0):
            c["mxv:zero"] += 1
        if kind == "transpose" and np.any(np.diff(want["csr"][0]) >= 2):
            c["transpose:row_of_two"] += 1
        if kind == "reduce" and p["axis"] == "rows" and p["op"] == "plus" and all_nan_rows(x).any():
            c["reduce:all_nan_row"] += 1
        # shapes and outputs
        dim0 = any(0 in shape for shape, _ in ins)
        if dim0 and kind != "extract":
            c["in:dim0"] += 1
            c[f"dim0:{kind}"] += 1
            if "csr" in want:
                c["in:dim0_to_csr"] += 1
        if "csr" in want and 0 in want["shape"]:
            c["out:dim0"] += 1
        if caller_outputs(kind, p, (M, N)):
            c["out:caller_tensor"] += 1
        if kind == "extract":
            rows = aux.get("rows")
            if p["permute"]:
                c["extract:permute"] += 1
            if rows is not None and len(np.unique(rows)) < len(rows):
                c["extract:rows_dup"] += 1
            if "cols" in aux and len(aux["cols"]) and extract_model.is_ascending(aux["cols"]):
                c["extract:cols_ascending"] += 1
            if want["stats"]["composed"]:
                c["extract:composed"] += 1
            if any(len(aux[k]) == 0 for k in ("rows", "cols") if k in aux):
                c["extract:empty_list"] += 1
        if kind == "build":
            head, length = want["layout"]["head"], want["layout"]["length"]
            if len(head) and np.all(length == 1):
                c["build:no_repeat"] += 1
            if want["stats"]["long_runs"]:
                c["build:long_run"] += 1
            if np.any((length > 1) & (head // CHUNK < (head + length - 1) // CHUNK)):
                c["build:run_over_chunk"] += 1
            if "b_vals" not in aux:
                c["build:novals"] += 1
            elif p["dup"] in ("first", "last") and len(head):
                order, vb = want["layout"]["order"], _bits(aux["b_vals"])
                if np.any(vb[order[head]] != vb[order[head + length - 1]]):     # a run whose ends differ: the fold's direction shows
                    c["build:ordered_run"] += 1
        if kind == "mxd":
            k = p["k"]
            c["mxd:k1" if k == 1 else "mxd:packed" if k < 64 else "mxd:tiles" if k > 64 else "mxd:one_tile"] += 1
            c["mxd:long" if want["stats"]["long_segments"] else "mxd:short"] += 1
            if p["out"] == "x":
                c["mxd:out_is_x"] += 1
            if M and not np.isnan(want["vec"][-1, -1]):
                c["mxd:corner_no_nan"] += 1
        if kind == "sddmm":
            if p["k"] == 0:
                c["sddmm:k0"] += 1
            if p["k"] > 64:
                c["sddmm:tiles"] += 1
            if p["accum"] in sddmm_model.ARITHMETIC and len(x[1]):
                c["sddmm:accum_reads_value"] += 1
                if p["accum"] in ("minus", "div") and sddmm_accum_exchanged(p, x, aux) is not None:
                    c["sddmm:accum_ordered"] += 1
            if p["y_is_x"]:
                c["sddmm:y_is_x"] += 1
        if kind == "mxv_arg":
            c["mxv_arg:long" if want["stats"]["long_segments"] else "mxv_arg:short"] += 1
            if len(arg_ties(p, x, aux)):
                c["mxv_arg:tie"] += 1
            if np.any((want["vec"][1] < 0) & (lens > 0)):
                c["mxv_arg:row_without"] += 1
            if not p["values"]:
                c["mxv_arg:values_false"] += 1

    # -- running
    def run(self):
        be = self.be
        for name, ncol, csr in starting_operands(self.seed, self.dt):
            h = be.upload(ncol, csr)
            L = _Live(h, (len(csr[0]) - 1, ncol), "upload")
            self.step = -1
            shape, back = be.read(h)
            for what, got, want in zip(("rowptr", "col"), back, csr):
                self.same_ints("upload", name, what, got, want)
            # The merge that uploads sums the one part, and some of its paths add it to -0.0 (MEASUREMENTS.md section 0m): a
            # signalling NaN may come back with its quiet bit set.  Nothing else may change -- sign and payload stay -- and
            # the chain starts from what is there.
            quiet = _bits(np.array([np.nan], self.dt))[0] & ~_bits(np.array([np.inf], self.dt))[0]
            asis = back[2].copy()
            quieted = np.isnan(csr[2]) & (_bits(back[2]) == (_bits(csr[2]) | quiet))
            asis[quieted] = csr[2][quieted]
            self.same_values("upload", name, "val", asis, csr[2], False)
            self.live.append(L)
        nsteps = int(self.rng.integers(6, 11))
        try:
            for self.step in range(nsteps):
                self.one_step()
        except ChainMismatch:
            self.close_all()
            raise               # (any other error may be the device's: nothing is closed, closing touches the GPU)
        self.close_all()
        return nsteps

    def close_all(self):
        """Everything is closed in a random order: the buffers of different operations recycle into each other."""
        for i in self.rng.permutation(len(self.live)):
            self.be.close(self.live[i].h)
        self.live = []

    def one_step(self):
        be = self.be
        self._host = {}
        deck = []
        for attempt in range(400):
            if not deck:
                deck = list(self.rng.permutation(KINDS))
            kind = deck.pop()
            drawn = getattr(self, "draw_" + kind)()
            if drawn is not None:
                break
            self.cov.redraws += 1
        else:
            raise RuntimeError(f"seed {self.seed}: no legal call in 400 draws")
        p, inputs, aux = drawn
        self.cov.drawn += 1
        space = p.get("space", "host")
        staged = be.stage(aux, space)
        ins = [self.host(L) for L in inputs]                       # 1. the device inputs, read back
        aux_back = be.unstage(staged, space)
        want = expected(kind, p, ins, aux_back)                    # 2. the model's answer from them
        try:
            got, st = be.run(kind, p, [L.h for L in inputs], staged)
        except ChainMismatch:
            raise
        except MarginDamaged as e:                                 # a write outside a caller's output
            self.fail(kind, p, str(e))
        except Exception as e:
            if not is_refusal(e):                                  # a device or runtime error: never a mismatch, it ends
                raise                                              # the run as itself and nothing more touches the GPU
            self.fail(kind, p, f"the call raised {type(e).__name__}: {e}")    # (a refused call is a finding: every draw is legal)
        if "vec" in want:                                          # 3. the comparison
            self.same_dense(kind, p, got, want["vec"], want["nan_ok"])
        else:
            shape, back = be.read(got)
            if tuple(shape) != tuple(want["shape"]):
                self.fail(kind, p, f"shape {tuple(shape)}, the model has {tuple(want['shape'])}")
            self.same_ints(kind, p, "rowptr", back[0], want["csr"][0])
            self.same_ints(kind, p, "col", back[1], want["csr"][1])
            self.same_values(kind, p, "val", back[2], want["csr"][2], want["nan_ok"])
            if kind == "build" and p["repeats"] == "none":
                # no coordinate repeats: the list is the input's entries shuffled, and the output is the input itself --
                # against the read-back input, not the model's answer
                self.same_ints(kind, p, "rowptr (against the input's)", back[0], ins[0][1][0])
                self.same_ints(kind, p, "col (against the input's)", back[1], ins[0][1][1])
                if "b_vals" in aux_back and p["dup"] != "count":
                    self.same_values(kind, p, "val (against the input's)", back[2], ins[0][1][2], False)
        for k, v in want["stats"].items():                         # 4. the stats
            if st[k] != v:
                self.fail(kind, p, f"stats[{k!r}] = {st[k]}, the model has {v}")
        self.note(kind, p, inputs, ins, aux_back, want)
        self.cov.steps += 1
        if "csr" in want:                                          # 5. the output joins the live set
            self.live.append(_Live(got, tuple(want["shape"]), kind))
        while len(self.live) > MAX_LIVE or (len(self.live) > 2 and self.rng.random() < 0.3):
            L = self.live.pop(int(self.rng.integers(len(self.live))))
            be.close(L.h)


def all_nan_rows(csr):
    """Which rows hold entries that are ALL NaNs."""
    rowptr, _, val = csr
    nan = np.concatenate([[0], np.cumsum(np.isnan(val))])
    lens = np.diff(rowptr)
    return (lens > 0) & (nan[rowptr[1:]] - nan[rowptr[:-1]] == lens)


def arg_ties(p, x, aux):
    """(rows, columns): the rows of an mxv_arg call in which at least two columns hold the best product that is no NaN (under
    the IEEE comparison: -0.0 and +0.0 tie), and for each the LARGEST such column -- the one arg must not name."""
    rowptr, col, val = x
    M = len(rowptr) - 1
    prod = mxv_arg_model.products(rowptr, col, val, aux.get("x"), p["mul"])
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr))
    ok = ~np.isnan(prod)
    best = np.full(M, np.inf if p["add"] == "min" else -np.inf, prod.dtype)
    (np.minimum if p["add"] == "min" else np.maximum).at(best, rows[ok], prod[ok])
    tied = ok & (prod == best[rows])
    last = np.full(M, -1, np.int64)
    np.maximum.at(last, rows[tied], col[tied].astype(np.int64))
    at = np.flatnonzero(np.bincount(rows[tied], minlength=M) >= 2)
    return at, last[at]


def sddmm_accum_exchanged(p, x, aux):
    """The values of an sddmm call whose arithmetic accum got its operands exchanged -- accum(d, c) for accum(c, d) --, or None
    where the comparison could not tell (every value has the same bits, or is a NaN either way)."""
    X = aux.get("X")
    d = sddmm_model.sddmm(*x, X, X if p["y_is_x"] else aux.get("Y"), p["add"], p["mul"], None, k=p["k"])[0]
    right, wrong = ewise_model.apply_op(p["accum"], x[2], d), ewise_model.apply_op(p["accum"], d, x[2])
    tells = (_bits(right) != _bits(wrong)) & ~(np.isnan(right) & np.isnan(wrong))
    return wrong if tells.any() else None


def run_seeds(backend, seeds=None, dtypes=None, cov=None):
    """Every seed in both dtypes.  Returns the Coverage; raises ChainMismatch at the first step that differs."""
    cov = cov or Coverage()
    for seed in (DEFAULT_SEEDS if seeds is None else seeds):
        for dt in (dtypes or DTYPES):
            Chain(backend, int(seed), dt, cov).run()
    return cov


def summary_line(cov, nseeds):
    return f"CHAIN_OK seeds={nseeds} steps={cov.steps} pairs={cov.different_pairs()} redraws={cov.redraws} skipped={cov.skipped} {cov.summary()}"


def main(argv=None):
    ap = argparse.ArgumentParser(description="chains of random result operations against the numpy models")
    ap.add_argument("--seeds", type=int, nargs="*", default=None, help="default: the committed seed list")
    ap.add_argument("--backend", choices=["gpu", "model"], default="gpu")
    ap.add_argument("--dtype", choices=["float32", "float64"], default=None)
    args = ap.parse_args(argv)
    seeds = DEFAULT_SEEDS if args.seeds is None else args.seeds
    t0 = time.perf_counter()
    backend = None
    try:
        backend = GpuBackend() if args.backend == "gpu" else ModelBackend()
        cov = run_seeds(backend, seeds, [np.dtype(args.dtype).type] if args.dtype else None)
    except ChainMismatch as e:
        print(e, flush=True)
        status = 1
    except Exception as e:      # no mismatch: a device or runtime error.  The context is left as it is (closing it runs on
        print(f"CHAIN_DEVICE_ERROR {type(e).__name__}: {e}", flush=True)     # the GPU), and the status tells the caller
        return DEVICE_ERROR_STATUS
    else:
        status = 0
    if hasattr(backend, "finish"):
        backend.finish()
    if status:
        return status
    print(cov.matrix())
    if args.seeds is None and not args.dtype and cov.missing():
        print("CHAIN_COVERAGE_MISSING " + " ".join(cov.missing()), flush=True)
        return 2
    print(f"({args.backend} backend, {time.perf_counter() - t0:.1f} s)")
    print(summary_line(cov, len(seeds)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
