#!/usr/bin/env python3
"""Times osp_csr_scan and osp_csr_draw (MEASUREMENTS.md section 0ac).  One process; run it under one `timeout`.

Operands, in f32 and f64 (--dtypes):
  (a) the directed adjacency of generators.rmat_coo at --scale (default 20, edge factor 16, seed 1) with non-negative random
      values: ``scan`` under every op, beside ``apply_vectors`` with one row vector on the same operand (the same traffic:
      values read once, values and pattern written) and beside the stream copy probe's rate; then ``draw`` at --draws
      (default 1 16 256) beside ``select_k(s, "random")``
  (b) one row of --hub entries (default 9 * 10^6) alone: ``scan`` under every op -- the chain is 2.8 * 10^5 sequential steps
Each case: ms (the call's own hipEvents, stats ms_total) as median and smallest - largest of --reps after one warm-up, launches,
read-backs, and the bytes the call moves at the least (values read, the three arrays written) over its time.  Last, one step of
``graph.weighted_random_walks`` beside one of ``graph.random_walks`` on the scale's undirected graph, --walkers walkers
(default 65536): wall time of the whole call (the graph's build included) for 0 steps and for --steps steps; the difference
over --steps is one step.  Prints one JSON line per case.  Per-kernel times come from running this tool under a kernel trace
with --only scan (`rocprofv3 --kernel-trace --stats -- python tools/time_scan.py --only scan`)."""
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

OPS = ("plus", "min", "max")


def spread(times):
    return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}


def timed(call, reps, keys):
    """call() -> (result or None, stats) reps + 1 times; results are closed."""
    times, first = [], None
    for rep in range(reps + 1):
        out, st = call()
        if out is not None:
            out.close()
        if rep == 0:
            first = {k: st[k] for k in keys}
        else:
            times.append(st["ms_total"])
    return first, spread(times)


def scan_cases(a, head, case, reps, copy_gbps, with_apply):
    M, nnz, vb = a.shape[0], a.nnz, np.dtype(a.dtype).itemsize
    least = nnz * vb + nnz * (vb + 4) + (M + 1) * 8       # values read; values, columns and row pointers written
    ref = None
    if with_apply:
        x = torch.ones(M, dtype=torch.float32 if vb == 4 else torch.float64, device=f"cuda:{a._ctx.device}")
        torch.cuda.synchronize()
        _, ref = timed(lambda: a.apply_vectors(rows=x, row_op="times"), reps, ("launches",))
    for op in OPS:
        first, t = timed(lambda: a.scan(op), reps, ("nnz_in", "blocks", "launches", "readbacks"))
        line = {**head, "case": case, "op": op, **first, "scan": t, "least_gb_per_s": least / t["ms_median"] / 1e6,
                "stream_copy_gb_per_s": copy_gbps, "fraction_of_copy_rate": least / t["ms_median"] / 1e6 / copy_gbps}
        if ref:
            line.update(apply_vectors=ref, scan_over_apply_vectors=t["ms_median"] / ref["ms_median"])
        print(json.dumps(line), flush=True)


def draw_cases(a, head, case, draws, reps):
    for s in draws:
        first, t = timed(lambda: (None, a.draw(s, seed=1)[-1]), reps, ("nnz_out", "rows_without", "launches", "readbacks"))
        _, ref = timed(lambda: a.select_k(s, "random", seed=1), reps, ("launches",))
        print(json.dumps({**head, "case": case, "draws": s, **first, "draw": t, "select_k_random": ref,
                          "draw_over_select_k": t["ms_median"] / ref["ms_median"]}), flush=True)


def walk_wall(fn, reps, dev):
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(rep)
        torch.cuda.synchronize(dev)
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return spread(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--hub", type=int, default=9_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", choices=["f32", "f64"], default=["f32", "f64"])
    ap.add_argument("--draws", nargs="*", type=int, default=[1, 16, 256])
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--only", choices=["scan"], default=None, help="the scan cases alone (for a kernel trace)")
    args = ap.parse_args()
    ctx = S.Context(0)
    dev = torch.device("cuda", ctx.device)
    copy_gbps = ctx.stream_copy_gbps()
    n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
    r, c = r.astype(np.int64), c.astype(np.int64)
    w = np.abs(np.random.default_rng(1).standard_normal(len(r)))
    for name in args.dtypes:
        dt = np.float32 if name == "f32" else np.float64
        head = {"dtype": name, "reps": args.reps}
        rmat = graph.adjacency_matrix(r, c, n, w, directed=True, loops=True, dup="first", dtype=dt, ctx=ctx)
        head_a = {**head, "M": rmat.shape[0], "nnz": rmat.nnz}
        scan_cases(rmat, head_a, f"(a) R-MAT scale {args.scale}", args.reps, copy_gbps, True)
        if not args.only:
            draw_cases(rmat, head_a, f"(a) R-MAT scale {args.scale}", args.draws, args.reps)
        rmat.close()
        vals = np.random.default_rng(2).random(args.hub).astype(dt)
        hub = ctx.build(1, args.hub, np.zeros(args.hub, np.uint32), np.arange(args.hub, dtype=np.uint32), vals, dup="error", dtype=dt, space="host")[0]
        scan_cases(hub, head, f"(b) one row of {args.hub}", args.reps, copy_gbps, False)
        hub.close()
        ctx.trim()
        torch.cuda.empty_cache()
    if not args.only:
        starts = np.random.default_rng(3).integers(0, n, args.walkers)
        for label, fn in (("weighted_random_walks", lambda steps: lambda rep: graph.weighted_random_walks(r, c, n, w, starts, steps, seed=rep, ctx=ctx)),
                          ("random_walks", lambda steps: lambda rep: graph.random_walks(r, c, n, starts, steps, seed=rep, ctx=ctx))):
            base, full = walk_wall(fn(0), args.reps, dev), walk_wall(fn(args.steps), args.reps, dev)
            print(json.dumps({"case": f"(c) {label} on R-MAT scale {args.scale}, wall time, the graph's build included", "walkers": args.walkers,
                              "steps": args.steps, "wall_0_steps": base, "wall_steps": full,
                              "ms_per_step": (full["ms_median"] - base["ms_median"]) / args.steps}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
