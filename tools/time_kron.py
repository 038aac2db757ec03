#!/usr/bin/env python3
"""Times osp_csr_kron (MEASUREMENTS.md section 0aa).  One process; run it under one `timeout`.

Two operand pairs, in f32 and f64 (--dtypes):
  (a) the directed adjacency of generators.rmat_coo at --scale (default 11, edge factor 16, seed 1) (x) itself: the
      Kronecker square of an R-MAT pattern, about 10^9 entries, millions of short rows
  (b) a hub-heavy pair: one row of --hub entries (default 15000) followed by --hub rows of one entry, (x) itself: one row of
      out holds hub^2 entries, 2 hub rows hold hub, the rest one
Each runs beside the bytes of out (row pointers, columns, values) at the measured stream-copy rate (osp_stream_copy_probe,
which counts read + written bytes: a kernel that only stores is set against that rate as it is, and against the 6.0-6.2
TB/s that plain stores reach on this device), and -- where out has at most --baseline-max entries -- beside the route that
existed before: the three COO lists of the product expanded in torch and passed to Context.build(dup="error",
space="device"), whose arrays are compared with the product's.  Device times: the calls' own hipEvents (stats ms_total), the
torch expansion by torch events; one warm-up, smallest - largest of --reps.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import graph  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402
from outerspace_amd.distributed import _as_tensor  # noqa: E402


def spread(times):
    return {"ms_min": min(times), "ms_max": max(times)}


def coo_of(x, dev, dt):
    """(rows, cols, vals) of a result as device tensors (int64, int64, dt)."""
    rp, ci, va = x.device_ptrs()
    td = torch.float32 if dt == np.float32 else torch.float64
    ptr = _as_tensor(rp, x.shape[0] + 1, "<i8", dev, torch.int64)
    col = _as_tensor(ci, x.nnz, "<i4", dev, torch.int32).long() & 0xffffffff
    val = _as_tensor(va, x.nnz, "<f4" if dt == np.float32 else "<f8", dev, td)
    return torch.repeat_interleave(torch.arange(x.shape[0], device=dev), ptr[1:] - ptr[:-1]), col, val


def torch_route(ctx, dev, dt, a, b):
    """a (x) b by the expansion of its COO lists in torch and one build.  Returns (result, device ms)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    ra, ca, va = coo_of(a, dev, dt)
    rb, cb, vb = coo_of(b, dev, dt)
    rows = (ra[:, None] * b.shape[0] + rb[None, :]).reshape(-1).to(torch.int32)
    cols = (ca[:, None] * b.shape[1] + cb[None, :]).reshape(-1).to(torch.int32)
    vals = (va[:, None] * vb[None, :]).reshape(-1).contiguous()
    t1.record()
    torch.cuda.synchronize(dev)
    out, st = ctx.build(a.shape[0] * b.shape[0], a.shape[1] * b.shape[1], rows, cols, vals, dup="error", dtype=dt, space="device")
    return out, t0.elapsed_time(t1) + st["ms_total"], t0.elapsed_time(t1)


def same(x, y):
    """Equal arrays, compared on the device (the results hold up to 10^9 entries)."""
    if x.shape != y.shape or x.nnz != y.nnz:
        return False
    dev = torch.device("cuda", x._ctx.device)
    bits = ("<i4", torch.int32) if x.dtype == np.float32 else ("<i8", torch.int64)   # (values as integers of their width)
    kinds = ((x.shape[0] + 1, "<i8", torch.int64), (x.nnz, "<i4", torch.int32), (x.nnz,) + bits)
    return all(torch.equal(_as_tensor(px, n, code, dev, td), _as_tensor(py, n, code, dev, td))
               for px, py, (n, code, td) in zip(x.device_ptrs(), y.device_ptrs(), kinds))


def hub_pair(ctx, dt, hub):
    rows = np.concatenate([np.zeros(hub, np.uint32), np.arange(1, hub + 1, dtype=np.uint32)])
    cols = np.concatenate([np.arange(hub, dtype=np.uint32), np.arange(hub, dtype=np.uint32)])
    vals = np.random.default_rng(2).standard_normal(2 * hub).astype(dt)
    return ctx.build(hub + 1, hub, rows, cols, vals, dup="error", dtype=dt, space="host")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=11)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--hub", type=int, default=15000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", choices=["f32", "f64"], default=["f32", "f64"])
    ap.add_argument("--ops", nargs="*", default=["times", "first"])
    ap.add_argument("--baseline-max", type=int, default=1 << 30, help="the torch route runs where out has at most this many entries")
    args = ap.parse_args()
    ctx = S.Context(0)
    dev = torch.device("cuda", ctx.device)
    gbps = ctx.stream_copy_gbps()
    for name in args.dtypes:
        dt = np.float32 if name == "f32" else np.float64
        V = np.dtype(dt).itemsize
        head = {"dtype": name, "reps": args.reps, "copy_gbps": gbps}
        n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
        w = np.random.default_rng(1).standard_normal(len(r))
        rmat = graph.adjacency_matrix(r.astype(np.int64), c.astype(np.int64), n, w, directed=True, loops=True, dup="first", dtype=dt, ctx=ctx)
        hub = hub_pair(ctx, dt, args.hub)
        for case, a in ((f"(a) R-MAT scale {args.scale} (x) itself", rmat), (f"(b) hub {args.hub} (x) itself", hub)):
            for op in args.ops:
                times, first, nbytes = [], None, 0
                for rep in range(args.reps + 1):
                    out, st = a.kron(a, op)
                    if rep == 0:
                        first = {k: st[k] for k in ("nnz_a", "nnz_b", "nnz_out", "launches", "readbacks")}
                        first.update(M=out.shape[0], N=out.shape[1])
                        nbytes = 8 * (out.shape[0] + 1) + out.nnz * (4 + V)
                    else:
                        times.append(st["ms_total"])
                    if rep < args.reps:
                        out.close()
                line = {**head, "case": case, "op": op, **first, "kron": spread(times), "bytes_out": nbytes,
                        "write_gbps": nbytes / min(times) / 1e6, "write_over_copy_rate": nbytes / min(times) / 1e6 / gbps}
                if op == "times" and out.nnz <= args.baseline_max:
                    t_route, t_expand, ok = [], [], None
                    for rep in range(min(args.reps, 2) + 1):
                        comp, ms, ms_expand = torch_route(ctx, dev, dt, a, a)
                        if rep == 0:
                            ok = same(out, comp)
                        else:
                            t_route.append(ms)
                            t_expand.append(ms_expand)
                        comp.close()
                        torch.cuda.empty_cache()
                    line.update(torch_route=spread(t_route), torch_expansion_ms_min=min(t_expand), equals_torch_route=ok,
                                torch_route_over_kron=min(t_route) / min(times))
                out.close()
                print(json.dumps(line), flush=True)
        rmat.close()
        hub.close()
        ctx.trim()
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
