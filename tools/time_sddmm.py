#!/usr/bin/env python3
"""Times osp_csr_sddmm under (plus, times) against the torch composition (X[r] * Y[c]).sum(1) on the same device
(MEASUREMENTS.md section 0s).  One process; run it under one `timeout`.

Shapes (--shapes), each in f64 and f32 (--dtypes), X and Y random on the device, at every k of --ks (default 1,4,16,64,256):
  adjacency  the symmetric 0/1 adjacency of generators.rmat_coo at --scale (default 20; edge factor 16): hub rows
  uniform    2^--uniform-scale (default 20) rows of --uniform-degree (default 16) random columns each
On each, after one warm-up of both, --reps times (default 20), smallest - largest reported:
  (a) A.sddmm(X, Y)                     device time from the call's own hipEvents (stats ms_total: the kernel AND the copies
                                        of the pattern into the new result)
  (b) (X[r] * Y[c]).sum(1)              torch events; the COO rows r are computed before and not timed.  It materialises two
                                        nnz x k tensors: where that does not fit, the line says so instead of a time
The tool refuses to go on when (a) and (b) differ by more than (k + 4) eps of sum |x y| somewhere.  Beside (a): its share of
Context.stream_copy_gbps() on the GATHERED bytes 2 nnz k sizeof(T) (what the lanes load, mostly from cache), and on the
COMPULSORY bytes (M + N) k sizeof(T) plus the pattern read and the result written.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import spgemm as S  # noqa: E402
from tools.time_mxv import symmetric_adjacency  # noqa: E402


def spread(times, key="ms"):
    return {f"{key}_min": min(times), f"{key}_max": max(times)}


def gathered_bytes(nnz, k, V):
    """What the lanes load: one row segment of X and one of Y per entry."""
    return 2 * nnz * k * V


def compulsory_bytes(M, N, nnz, k, V):
    """What has to move if every row of X and Y were read once: X and Y, the pattern read (row pointers, columns) and copied
    into the result, and the result's values."""
    return (M + N) * k * V + 2 * (8 * (M + 1) + 4 * nnz) + nnz * V


def uniform_pattern(ctx, scale, degree, dt, dev):
    n = 1 << scale
    g = torch.Generator(device=dev).manual_seed(3)
    r = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(degree)
    c = torch.randint(0, n, (n * degree,), dtype=torch.int32, device=dev, generator=g)
    torch.cuda.synchronize()
    return ctx.build(n, n, r, c, None, dup="first", dtype=dt, space="device")[0]


def torch_composition(X, Y, r, c, reps):
    """((times, values), None) or (None, why not)."""
    try:
        out = (X[r] * Y[c]).sum(1)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = (X[r] * Y[c]).sum(1)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return (times, out), None
    except Exception as e:   # noqa: BLE001  (whatever this build says, out of memory above all: it is reported, not hidden)
        torch.cuda.empty_cache()
        return None, f"{type(e).__name__}: {str(e)[:160]}"


def time_shape(head, name, A, ks, reps, copy_gbps):
    from outerspace_amd.distributed import _as_tensor
    M, N = A.shape
    V = np.dtype(A.dtype).itemsize
    f32 = A.dtype == np.float32
    tdt = torch.float32 if f32 else torch.float64
    dev = f"cuda:{A._ctx.device}"
    rowptr = torch.from_numpy(A.rowptr.copy()).to(dev)
    r = torch.repeat_interleave(torch.arange(M, device=dev), rowptr[1:] - rowptr[:-1])
    c = torch.from_numpy(A.colidx.astype(np.int64)).to(dev)
    row = np.diff(A.rowptr)
    head = {**head, "shape": name, "M": M, "N": N, "nnz": A.nnz, "row_mean": float(row.mean()), "row_max": int(row.max()), "copy_gbps": copy_gbps}
    for k in ks:
        X = torch.rand((M, k), dtype=tdt, device=dev) - 0.5
        Y = torch.rand((N, k), dtype=tdt, device=dev) - 0.5
        torch.cuda.synchronize()
        ta, st = [], None
        for rep in range(reps + 1):
            E, st = A.sddmm(X, Y)
            if rep:
                ta.append(st["ms_total"])
            if rep < reps:
                E.close()
        got = _as_tensor(E.device_ptrs()[2], E.nnz, "<f4" if f32 else "<f8", dev, tdt).clone()
        torch.cuda.synchronize()   # (the copy is torch's: it is done before E's arrays go back to the pool)
        E.close()
        gb, cb = gathered_bytes(A.nnz, k, V), compulsory_bytes(M, N, A.nnz, k, V)
        line = {**head, "k": k, "lanes_per_entry": st["lanes_per_entry"], "launches": st["launches"], "sddmm": spread(ta),
                "gathered_bytes": gb, "gathered_gbps_at_min": gb / min(ta) / 1e6, "gathered_share_of_copy": gb / min(ta) / 1e6 / copy_gbps,
                "compulsory_bytes": cb, "compulsory_gbps_at_min": cb / min(ta) / 1e6, "compulsory_share_of_copy": cb / min(ta) / 1e6 / copy_gbps}
        res, why = torch_composition(X, Y, r, c, reps)
        if res is None:
            line["torch"] = why
        else:
            tt, want = res
            scale = (X.abs()[r] * Y.abs()[c]).sum(1)
            if not bool(((got - want).abs() <= (k + 4) * torch.finfo(tdt).eps * scale).all()):
                sys.exit(f"{name} k={k}: sddmm and the torch composition differ: not timing a wrong result")
            line.update({"torch": spread(tt), "torch_over_sddmm": min(tt) / min(ta), "torch_over_sddmm_worst": min(tt) / max(ta), "agree": True})
            del want, scale
        print(json.dumps(line), flush=True)
        del X, Y, got, res
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--uniform-scale", type=int, default=20)
    ap.add_argument("--uniform-degree", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="1,4,16,64,256")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--shapes", default="adjacency,uniform")
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    ctx = S.Context(0)
    copy_gbps = ctx.stream_copy_gbps()
    adj = None   # (the adjacency is generated once: its values are ones in either dtype)
    for name in args.dtypes.split(","):
        dt = np.float32 if name == "f32" else np.float64
        head = {"dtype": name, "reps": args.reps}
        shapes = args.shapes.split(",")
        if "adjacency" in shapes:
            adj = adj or symmetric_adjacency(args.scale, args.edge_factor, np.float64)
            n, (rowptr, col, val) = adj
            A = ctx.merge_csr_parts(n, n, [(rowptr, col, val.astype(dt))])
            time_shape({**head, "scale": args.scale}, "adjacency", A, ks, args.reps, copy_gbps)
            A.close()
            ctx.trim()
        if "uniform" in shapes:
            A = uniform_pattern(ctx, args.uniform_scale, args.uniform_degree, dt, f"cuda:{ctx.device}")
            time_shape({**head, "scale": args.uniform_scale}, "uniform", A, ks, args.reps, copy_gbps)
            A.close()
            ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
