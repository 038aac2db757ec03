#!/usr/bin/env python3
"""Times osp_csr_assign (MEASUREMENTS.md section 0z).  One process; run it under one `timeout`.

c is the symmetric adjacency of generators.rmat_coo at --scale (default 20, edge factor 16, seed 1) as a result, --dtype f64;
the a of (a) is cut out of a second R-MAT (seed 2) of the same size:
  (a) a random ascending I x I block of --block vertices (default 2^16) assigned from other.extract(I, I), without accum and
      with "plus"
  (b) a row batch: --block random distinct rows with cols None, a = other.extract(R, None)
  (c) the same a as (a) embedded into an empty result
Each case runs beside the COMPOSITION of calls that existed before osp_csr_assign -- select_vertices of the region,
apply_mask(complement) of it, torch index gathers of a's coordinates plus a build, a union (no accum), or the gathers, the
build and the union alone (accum; an embedding is the gathers and the build) -- whose arrays are compared with the fused
call's, and beside the bytes of one read of c and a plus one write of out at the measured stream-copy rate
(osp_stream_copy_probe).  Device times: the calls' own hipEvents (stats ms_total), the torch gathers by torch events; one
warm-up, smallest - largest of --reps.  Prints one JSON line per case."""
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


def adjacency(ctx, dev, dt, scale, edge_factor, seed):
    n, r, c, _ = gen.rmat_coo(scale, edge_factor, "g500", seed=seed)
    n, rowptr, colidx, vals = graph.symmetric_adjacency(r.astype(np.int64), c.astype(np.int64), n, dev)
    vals = vals.to(torch.float32 if dt == np.float32 else torch.float64)
    cols32 = colidx.to(torch.int32)
    torch.cuda.synchronize(dev)
    return ctx.merge_csr_parts_device(dt, n, n, [(rowptr.data_ptr(), cols32.data_ptr(), vals.data_ptr())])


def same(x, y):
    bits = np.uint64 if x.vals.dtype == np.float64 else np.uint32
    return bool(np.array_equal(x.rowptr, y.rowptr) and np.array_equal(x.colidx, y.colidx) and np.array_equal(x.vals.view(bits), y.vals.view(bits)))


def composition(ctx, dev, dt, c, a, rows_t, cols_t, keep_r, keep_c, accum):
    """out and its device time by the calls that existed before assign.  rows_t / cols_t: int64 device tensors (None: identity);
    keep_r / keep_c: uint8 device vectors of the region (None: every row / column); c None: an embedding."""
    ms, made = 0.0, []
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rp, ci, va = a.device_ptrs()
    td = torch.float32 if dt == np.float32 else torch.float64
    t0.record()
    a_ptr = _as_tensor(rp, a.shape[0] + 1, "<i8", dev, torch.int64)
    a_col = _as_tensor(ci, a.nnz, "<i4", dev, torch.int32).long() & 0xffffffff
    a_val = _as_tensor(va, a.nnz, "<f4" if dt == np.float32 else "<f8", dev, td)
    a_row = torch.repeat_interleave(torch.arange(a.shape[0], device=dev), a_ptr[1:] - a_ptr[:-1])
    big_r = (a_row if rows_t is None else rows_t[a_row]).to(torch.int32).contiguous()
    big_c = (a_col if cols_t is None else cols_t[a_col]).to(torch.int32).contiguous()
    t1.record()
    torch.cuda.synchronize(dev)
    ms += t0.elapsed_time(t1)
    M, N = (c.shape if c is not None else (int(keep_r.numel()), int(keep_c.numel())))
    E, st = ctx.build(M, N, big_r, big_c, a_val, dup="error", dtype=dt, space="device")
    ms += st["ms_total"]
    if c is None:
        return E, ms
    made.append(E)
    base = c
    if accum is None:
        region, st = c.select_vertices(keep_r, keep_c)
        ms += st["ms_total"]
        made.append(region)
        base, st = c.apply_mask(region, complement=True)
        ms += st["ms_total"]
        made.append(base)
    out, st = base.union(E, accum or "plus")
    ms += st["ms_total"]
    for x in made:
        x.close()
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--block", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dt = np.float32 if args.dtype == "f32" else np.float64
    V = np.dtype(dt).itemsize
    ctx = S.Context(0)
    dev = torch.device("cuda", ctx.device)
    gbps = ctx.stream_copy_gbps()
    head = {"scale": args.scale, "dtype": args.dtype, "reps": args.reps, "copy_gbps": gbps}
    C_ = adjacency(ctx, dev, dt, args.scale, args.edge_factor, 1)
    other = adjacency(ctx, dev, dt, args.scale, args.edge_factor, 2)
    n = C_.shape[0]
    print(json.dumps({**head, "case": "c and the matrix a is cut from", "n": n, "nnz_c": C_.nnz, "nnz_other": other.nnz}), flush=True)
    rng = np.random.default_rng(3)
    I = np.sort(rng.choice(n, args.block, replace=False))
    R = rng.permutation(n)[:args.block]
    ti32, tr32 = (torch.from_numpy(x.astype(np.int32)).to(dev) for x in (I, R))
    ti, tr = ti32.long(), tr32.long()
    keep_i = torch.zeros(n, dtype=torch.uint8, device=dev)
    keep_i[ti] = 1
    keep_rows = torch.zeros(n, dtype=torch.uint8, device=dev)
    keep_rows[tr] = 1
    torch.cuda.synchronize(dev)
    block, _ = other.extract(ti32, ti32)
    batch, _ = other.extract(tr32, None)
    empty, _ = ctx.build(n, n, [], [], dtype=dt, space="host")

    def bytes_model(c, a, out):
        """one read of c and of a, one write of out: row pointers, columns and values"""
        return sum(8 * (x.shape[0] + 1) + x.nnz * (4 + V) for x in (c, a, out))

    cases = [("(a) block I x I, no accum", C_, block, ti32, ti32, ti, ti, keep_i, keep_i, None),
             ("(a) block I x I, plus", C_, block, ti32, ti32, ti, ti, keep_i, keep_i, "plus"),
             ("(b) row batch, cols None, no accum", C_, batch, tr32, None, tr, None, keep_rows, None, None),
             ("(b) row batch, cols None, plus", C_, batch, tr32, None, tr, None, keep_rows, None, "plus"),
             ("(c) embedding of the block into an empty result", empty, block, ti32, ti32, ti, ti, keep_i, keep_i, None)]
    for name, c, a, rows32, cols32, rows64, cols64, kr, kc, accum in cases:
        first, st, t_fused, t_comp, ok = None, None, [], [], None
        for rep in range(args.reps + 1):
            out, st = c.assign(a, rows32, cols32, accum)
            comp, ms = composition(ctx, dev, dt, None if c is empty else c, a, rows64, cols64, kr, kc, accum)
            if rep == 0:
                ok = same(out, comp)
                first = {k: st[k] for k in ("nnz_c", "nnz_a", "nnz_region", "nnz_both", "nnz_out", "launches", "readbacks")}
                nbytes = bytes_model(c, a, out)
            else:
                t_fused.append(st["ms_total"])
                t_comp.append(ms)
            out.close()
            comp.close()
        print(json.dumps({**head, "case": name, **first, "fused": spread(t_fused), "composition": spread(t_comp),
                          "equals_composition": ok, "composition_over_fused": min(t_comp) / min(t_fused), "bytes_model": nbytes,
                          "ms_at_copy_rate": nbytes / gbps / 1e6, "copy_rate_share": nbytes / min(t_fused) / 1e6 / gbps}), flush=True)
    for x in (block, batch, empty, other, C_):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
