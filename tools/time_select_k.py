#!/usr/bin/env python3
"""Times osp_csr_select_k (MEASUREMENTS.md section 0ab).  One process; run it under one `timeout`.

Operands, in f32 and f64 (--dtypes):
  (a) the directed adjacency of generators.rmat_coo at --scale (default 20, edge factor 16, seed 1) with non-negative random
      values: every order (--orders) at every k (--ks, default 1 16 256)
  (b) one row of --hub entries (default 9 * 10^6) alone, values with thousands of copies each, so the value orders run every
      radix pass: every order at k = 20000
Each case: ms (the call's own hipEvents, stats ms_total) as median and smallest - largest of --reps after one warm-up,
launches, read-backs, capped and long rows; beside the time of a device copy of `in`'s three arrays (torch clones under
torch events: read once, write once -- the floor of any select that keeps most of `in`), and, for LARGEST, beside
``inflate_prune(power=1, threshold=0, max_per_row=k)`` on the same operand, whose pattern is compared with the select's.
Last, one ``graph.sample_neighbors`` batch on the scale's undirected graph: --seeds seeds (default 1024), fanouts 15 10 5,
wall time of the whole call and the k-selects' share.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import graph  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402
from outerspace_amd.distributed import _as_tensor  # noqa: E402


def spread(times):
    return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}


def copy_ms(x, dev, reps):
    """Device time of copying x's three arrays, smallest and largest of reps."""
    rp, ci, va = x.device_ptrs()
    code, td = ("<f4", torch.float32) if x.dtype == np.float32 else ("<f8", torch.float64)
    parts = [_as_tensor(rp, x.shape[0] + 1, "<i8", dev, torch.int64), _as_tensor(ci, max(x.nnz, 1), "<i4", dev, torch.int32),
             _as_tensor(va, max(x.nnz, 1), code, dev, td)]
    times = []
    for rep in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        copies = [p.clone() for p in parts]
        t1.record()
        torch.cuda.synchronize(dev)
        del copies
        if rep:
            times.append(t0.elapsed_time(t1))
    return spread(times)


def timed(call, reps, keys):
    """call() -> (result, stats) reps + 1 times; the last result is returned open."""
    times, first, out = [], None, None
    for rep in range(reps + 1):
        if out is not None:
            out.close()
        out, st = call()
        if rep == 0:
            first = {k: st[k] for k in keys}
        else:
            times.append(st["ms_total"])
    return out, first, spread(times)


def same_pattern(x, y, dev):
    if x.shape != y.shape or x.nnz != y.nnz:
        return False
    kinds = ((x.shape[0] + 1, "<i8", torch.int64), (max(x.nnz, 1), "<i4", torch.int32))
    return all(torch.equal(_as_tensor(px, n, code, dev, td), _as_tensor(py, n, code, dev, td))
               for px, py, (n, code, td) in zip(x.device_ptrs()[:2], y.device_ptrs()[:2], kinds))


def cases(ctx, dev, a, head, case, orders, ks, reps):
    floor = copy_ms(a, dev, reps)
    keys = ("nnz_in", "nnz_out", "rows_capped", "rows_long", "launches", "readbacks")
    for order in orders:
        for k in ks:
            out, first, t = timed(lambda: a.select_k(k, order, seed=1), reps, keys)
            line = {**head, "case": case, "order": order, "k": k, **first, "select_k": t, "copy_of_in": floor,
                    "select_k_over_copy": t["ms_median"] / floor["ms_median"]}
            if order == "largest":
                ref, rfirst, rt = timed(lambda: a.inflate_prune(power=1.0, threshold=0.0, max_per_row=k), reps, ("launches", "rows_long"))
                line.update(inflate_prune=rt, inflate_prune_launches=rfirst["launches"], same_pattern=same_pattern(out, ref, dev),
                            select_k_over_inflate_prune=t["ms_median"] / rt["ms_median"])
                ref.close()
            out.close()
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--hub", type=int, default=9_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", choices=["f32", "f64"], default=["f32", "f64"])
    ap.add_argument("--orders", nargs="*", default=["largest", "smallest", "random"])
    ap.add_argument("--ks", nargs="*", type=int, default=[1, 16, 256])
    ap.add_argument("--seeds", type=int, default=1024)
    args = ap.parse_args()
    ctx = S.Context(0)
    dev = torch.device("cuda", ctx.device)
    n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
    r, c = r.astype(np.int64), c.astype(np.int64)
    for name in args.dtypes:
        dt = np.float32 if name == "f32" else np.float64
        head = {"dtype": name, "reps": args.reps}
        w = np.abs(np.random.default_rng(1).standard_normal(len(r)))
        rmat = graph.adjacency_matrix(r, c, n, w, directed=True, loops=True, dup="first", dtype=dt, ctx=ctx)
        cases(ctx, dev, rmat, head, f"(a) R-MAT scale {args.scale}", args.orders, args.ks, args.reps)
        rmat.close()
        vals = np.random.default_rng(2).integers(0, 1000, args.hub).astype(dt)
        hub = ctx.build(1, args.hub, np.zeros(args.hub, np.uint32), np.arange(args.hub, dtype=np.uint32), vals, dup="error", dtype=dt, space="host")[0]
        cases(ctx, dev, hub, head, f"(b) one row of {args.hub}", args.orders, [20000], args.reps)
        hub.close()
        ctx.trim()
        torch.cuda.empty_cache()
    seeds = np.random.default_rng(3).choice(n, min(args.seeds, n), replace=False)
    times, info = [], None
    for rep in range(args.reps + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        blocks, frontiers, info = graph.sample_neighbors(r, c, n, seeds, (15, 10, 5), seed=rep, ctx=ctx)
        torch.cuda.synchronize(dev)
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
        for b in blocks:
            b.close()
    print(json.dumps({"case": f"(c) sample_neighbors on R-MAT scale {args.scale}, the graph's build included", "seeds": len(seeds),
                      "fanouts": [15, 10, 5], "frontiers": [len(f) for f in frontiers], "nnz": info["nnz"], "select_k_launches": info["launches"],
                      "select_k_ms": info["ms_total"], "wall": spread(times)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
