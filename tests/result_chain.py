"""A seeded chain driver for the operations that take a CSR result and return a result or a vector (not a test file: the
CPU and GPU tests import it, and ``python -m tests.result_chain`` runs it on the GPU in a process of its own).

A chain starts from three uploaded CSR operands and applies 6 to 10 operations drawn at random from the whole surface --
apply_mask, select, ewise, inflate_prune, select_vertices, apply_vectors, transpose, mxm, matmul, reduce, mxv -- each to a
randomly chosen live result or a pair of them, closing results at random points so that pool buffers recycle from one
operation into another.  Every step follows one protocol, so that NaN payloads and summation orders never accumulate:

  1. the operation's device inputs are read back to the host (fresh copies, never a cache);
  2. the numpy models of tests/*_model.py compute the answer from those arrays;
  3. the backend's output is compared with it: row pointers and columns equal, values equal as BITS, and a value that came
     out of arithmetic and is a NaN in the model only has to be a NaN (each operation's own test file's rule);
  4. the stats fields the per-operation tests check are compared with what the model predicts;
  5. the output joins the live set.

The generator only draws legal calls: an illegal draw (no conforming partner, values an operation does not take, a product
beyond PRODUCT_CAP) is REDRAWN, and no drawn step is ever skipped.  The driver talks to a backend object: GpuBackend wraps
CsrResult, ModelBackend the models themselves, so the generator and the coverage counters run without a GPU
(tests/test_result_chain_cpu.py), and a ModelBackend with one planted defect shows that the comparison bites.

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

from tests import bfs_model, ewise_model, mcl_model, mxv_model, semiring_model, transpose_model, truss_model, vector_model

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
KINDS = ["apply_mask", "select", "ewise", "inflate_prune", "select_vertices", "apply_vectors", "transpose", "mxm", "matmul", "reduce",
         "mxv"]
DTYPES = [np.float32, np.float64]
# chosen on the model backend so that every condition of Coverage.REQUIRED is met in both dtypes, most of them three times
DEFAULT_SEEDS = [0, 1, 5, 7, 16, 20, 21, 32, 33, 63, 67, 75]
assert PRODUCT_CAP > 3 * SHORT_CAP


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


# ---- what the models say --------------------------------------------------------------------------------------------------------
_MEMO = [None, None, None, None]


def expected(kind, p, ins, aux):
    """The model's answer for one call.  ins: the (shape, (rowptr, col, val)) of the CSR inputs as read back; aux: the host
    arrays of the call (mask, vectors).  Returns a dict: ``csr`` (rowptr, col, val) and ``shape``, or ``vec``; ``nan_ok``
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

    def run(self, kind, p, handles, staged):
        want = expected(kind, p, [self.read(h) for h in handles], staged)
        if "vec" in want:
            return want["vec"], dict(want["stats"])
        return _Held(want["shape"], want["csr"]), dict(want["stats"])


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
        if kind == "reduce":
            if p["out"] == "host":
                return x.reduce(p["axis"], p["op"])
            n = x.shape[0 if p["axis"] == "rows" else 1]
            out = self.torch.full((n,), 7.0, dtype=self.torch.float32 if x.dtype == np.float32 else self.torch.float64, device=self.dev)
            self.torch.cuda.synchronize(self.dev)
            _, st = x.reduce(p["axis"], p["op"], out=out)
            return out.cpu().numpy(), st
        if kind == "mxv":
            y, st = x.mxv(arg("x"), p["add"], p["mul"], space=space)
            return (y.cpu().numpy() if space == "device" else y), st
        raise KeyError(kind)


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
                 # where each planted defect of tests/test_result_chain_cpu.py finds something to damage
                 "select:nonempty", "ewise:nonempty", "mxv:zero", "transpose:row_of_two", "reduce:all_nan_row"])

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
        if p["mul"] == "first" and self.rng.random() < 0.5:
            return dict(p, x=None), [x], {}
        return p, [x], dict(x=self.vector(x.shape[1]))

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
        loose = np.isnan(want) & nan_ok
        bad = np.flatnonzero(np.where(loose, ~np.isnan(got), _bits(got) != _bits(want)))
        if len(bad):
            i = bad[0]
            self.fail(kind, p, f"{name}[{i}] = {got[i]!r} (bits {int(_bits(got)[i]):#x}), the model has {want[i]!r} "
                               f"(bits {int(_bits(want)[i]):#x}) ({len(bad)} differ)")

    # -- counting
    def note(self, kind, p, inputs, ins, want):
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
        except Exception as e:
            if not is_refusal(e):                                  # a device or runtime error: never a mismatch, it ends
                raise                                              # the run as itself and nothing more touches the GPU
            self.fail(kind, p, f"the call raised {type(e).__name__}: {e}")    # (a refused call is a finding: every draw is legal)
        if "vec" in want:                                          # 3. the comparison
            self.same_values(kind, p, "vector", got, want["vec"], want["nan_ok"])
        else:
            shape, back = be.read(got)
            if tuple(shape) != tuple(want["shape"]):
                self.fail(kind, p, f"shape {tuple(shape)}, the model has {tuple(want['shape'])}")
            self.same_ints(kind, p, "rowptr", back[0], want["csr"][0])
            self.same_ints(kind, p, "col", back[1], want["csr"][1])
            self.same_values(kind, p, "val", back[2], want["csr"][2], want["nan_ok"])
        for k, v in want["stats"].items():                         # 4. the stats
            if st[k] != v:
                self.fail(kind, p, f"stats[{k!r}] = {st[k]}, the model has {v}")
        self.note(kind, p, inputs, ins, want)
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
