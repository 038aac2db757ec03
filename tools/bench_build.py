#!/usr/bin/env python3
"""Times osp_csr_build (MEASUREMENTS.md section 0p).  One process; run it under one `timeout`.

On the edge list of generators.rmat_coo at --scale (default 20, edge factor 16, seed 1), self loops dropped, followed by
its mirrored copy -- the symmetric list of section 0o --, as int32 device tensors with random weights, --dtype f64:
  (a) Context.build(dup="min") against the way without build: graph.weighted_adjacency(keep="min") (torch.unique on 64-bit
      keys, scatter_reduce_, bincount) plus the one-part import merge_csr_parts_device, on the same device tensors
  (b) Context.build(dup="plus") on the list doubled (every coordinate at least twice) against graph._directed_pattern_result
      (torch.unique, bincount, the import) on the same tensors: the nearest thing without build, which only deduplicates
  (c) one coordinate repeated --run times (default 2^20) under "plus" -- a chain of dependent additions by definition,
      folded by one wave -- and under "first"
  (d) graph.adjacency_matrix end to end (checks, mirroring, conversion, build) on the one-directional list
Wall times are host clocks around work that ends in a device synchronise; device times are the calls' own hipEvents (stats
ms_total).  One warm-up call, smallest - largest of --reps.  (a)'s arrays are compared with the other way's.  --only CASE runs
one case (for a kernel trace).  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import graph  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402


def spread(times, key="ms"):
    return {key + "_min": min(times), key + "_max": max(times)}


def timed(dev, reps, call):
    """call() -> (result, stats or None); one warm-up call, whose result is returned open.  Returns (first result, last
    stats, wall ms of every repetition, device ms of every repetition or None)."""
    first, wall, device, st = None, [], [], None
    for rep in range(reps + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res, st = call()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if rep == 0:
            first = res
        else:
            wall.append((t1 - t0) * 1e3)
            if st is not None:
                device.append(st["ms_total"])
            res.close()
    return first, st, wall, device or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--run", type=int, default=1 << 20, help="length of the one run of (c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    ap.add_argument("--only", choices=["a", "b", "c", "d"], default=None)
    args = ap.parse_args()
    dt = np.float32 if args.dtype == "f32" else np.float64
    tdt = torch.float32 if dt == np.float32 else torch.float64
    ctx = S.Context(0)
    dev = torch.device("cuda", ctx.device)
    head = {"scale": args.scale, "dtype": args.dtype, "reps": args.reps}
    n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
    r, c = r.astype(np.int64), c.astype(np.int64)
    keep = r != c
    r, c = r[keep], c[keep]
    rng = np.random.default_rng(3)
    w = rng.random(len(r)) + 0.5
    tr, tc, tw = torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(w).to(dev).to(tdt)
    sr, sc, sw = torch.cat([tr, tc]), torch.cat([tc, tr]), torch.cat([tw, tw])          # the symmetric list
    sr32, sc32 = sr.to(torch.int32), sc.to(torch.int32)
    torch.cuda.synchronize(dev)
    print(json.dumps({**head, "case": "the symmetric list", "n": n, "entries": int(sr.numel())}), flush=True)
    want = lambda case: args.only in (None, case)   # noqa: E731

    if want("a"):
        def other_way():
            _, rowptr, colidx, vals = graph.weighted_adjacency(tr, tc, n, tw, keep="min", device=dev)
            return graph._csr_result(ctx, dt, n, n, rowptr, colidx.to(torch.int32), vals.to(tdt), dev), None
        O, _, wall_o, _ = timed(dev, args.reps, other_way)
        B, st, wall_b, dev_b = timed(dev, args.reps, lambda: ctx.build(n, n, sr32, sc32, sw, dup="min", dtype=dt, space="device"))
        bits = np.uint32 if dt == np.float32 else np.uint64
        same = bool(np.array_equal(O.rowptr, B.rowptr) and np.array_equal(O.colidx, B.colidx) and np.array_equal(O.vals.view(bits), B.vals.view(bits)))
        print(json.dumps({**head, "case": "(a) weighted_adjacency(keep=min) + import", "nnz_out": O.nnz, **spread(wall_o, "wall_ms")}), flush=True)
        print(json.dumps({**head, "case": "(a) build(dup=min)", "nnz_in": st["nnz_in"], "nnz_out": st["nnz_out"], "launches": st["launches"],
                          "readbacks": st["readbacks"], "long_runs": st["long_runs"], **spread(wall_b, "wall_ms"), **spread(dev_b, "device_ms"),
                          "arrays_equal": same, "other_way_over_build_wall": min(wall_o) / min(wall_b)}), flush=True)
        O.close()
        B.close()

    if want("b"):
        dr, dc, dw = torch.cat([sr, sr]), torch.cat([sc, sc]), torch.cat([sw, sw])      # the list doubled
        dr32, dc32 = dr.to(torch.int32), dc.to(torch.int32)
        torch.cuda.synchronize(dev)
        O, _, wall_o, _ = timed(dev, args.reps, lambda: (graph._directed_pattern_result(dr, dc, n, dt, ctx)[1], None))
        B, st, wall_b, dev_b = timed(dev, args.reps, lambda: ctx.build(n, n, dr32, dc32, dw, dup="plus", dtype=dt, space="device"))
        same = bool(np.array_equal(O.rowptr, B.rowptr) and np.array_equal(O.colidx, B.colidx))
        print(json.dumps({**head, "case": "(b) _directed_pattern_result (deduplicates only) on the list doubled", "nnz_out": O.nnz,
                          **spread(wall_o, "wall_ms")}), flush=True)
        print(json.dumps({**head, "case": "(b) build(dup=plus) on the list doubled", "nnz_in": st["nnz_in"], "nnz_out": st["nnz_out"],
                          "launches": st["launches"], "readbacks": st["readbacks"], "long_runs": st["long_runs"], **spread(wall_b, "wall_ms"),
                          **spread(dev_b, "device_ms"), "pattern_equal": same, "other_way_over_build_wall": min(wall_o) / min(wall_b)}), flush=True)
        O.close()
        B.close()
        del dr, dc, dw, dr32, dc32

    if want("c"):
        m = args.run
        one = torch.full((m,), 7, dtype=torch.int32, device=dev)
        ones = torch.from_numpy(rng.random(m)).to(dev).to(tdt)
        torch.cuda.synchronize(dev)
        for op in ("plus", "first"):
            B, st, wall_b, dev_b = timed(dev, args.reps, lambda: ctx.build(16, 16, one, one, ones, dup=op, dtype=dt, space="device"))
            print(json.dumps({**head, "case": f"(c) one coordinate {m} times, dup={op}", "nnz_out": st["nnz_out"], "launches": st["launches"],
                              "readbacks": st["readbacks"], "long_runs": st["long_runs"], **spread(wall_b, "wall_ms"), **spread(dev_b, "device_ms"),
                              "ns_per_entry_device": min(dev_b) * 1e6 / m}), flush=True)
            B.close()

    if want("d"):
        A, _, wall_a, _ = timed(dev, args.reps, lambda: (graph.adjacency_matrix(tr, tc, n, tw, dup="min", dtype=dt, ctx=ctx), None))
        print(json.dumps({**head, "case": "(d) graph.adjacency_matrix end to end", "nnz_out": A.nnz, **spread(wall_a, "wall_ms")}), flush=True)
        A.close()
    ctx.close()


if __name__ == "__main__":
    main()
