#!/usr/bin/env python3
"""Times Markov clustering (graph.markov_cluster) on the R-MAT generator's graph at --scale (MEASUREMENTS.md section 0c).

Per iteration: the product's and the prune step's device time (the library's events), entries in and out of the step, and
the step's achieved bytes per second -- the bytes the step has to move (12 or 8 per entry read and written, row pointers
in and out) over its device time -- beside what a plain copy reaches in the same run (osp_stream_copy_probe).

--host-prune runs the same loop the way a user had to before osp_csr_inflate_prune existed: every expansion copied to the
host (to_scipy), pruned, inflated and normalised there with numpy, and uploaded again; per iteration the host clock around
that round trip is printed instead of the step's device time.  Prints one JSON line per iteration and a summary line."""
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
from outerspace_amd.sparse_util import _result_as_input  # noqa: E402


def step_bytes(n, nnz_in, nnz_out, vbytes):
    """What one step must read and write: columns and values of the expansion and of the output, both row pointer arrays."""
    return (nnz_in + nnz_out) * (4 + vbytes) + 2 * (n + 1) * 8


def host_step(C, inflation, threshold, max_per_row):
    """prune / inflate / normalise of a scipy CSR with numpy: the step's rules, sums in numpy's own order."""
    C.sort_indices()
    n = C.shape[0]
    ptr, col, val = C.indptr, C.indices, C.data
    row = np.repeat(np.arange(n), np.diff(ptr))
    keep = val >= threshold
    rowmax = np.zeros(n)
    np.maximum.at(rowmax, row, val)
    none = np.bincount(row[keep], minlength=n) == 0
    first_max = np.zeros(len(val), bool)
    if none.any():      # rescue: the first entry that equals the row's maximum
        cand = np.nonzero(none[row] & (val == rowmax[row]))[0]
        _, idx = np.unique(row[cand], return_index=True)
        first_max[cand[idx]] = True
    keep |= first_max
    row, col, val = row[keep], col[keep], val[keep]
    if max_per_row:
        cnt = np.bincount(row, minlength=n)
        if cnt.max(initial=0) > max_per_row:      # only the rows over the cap are sorted
            over = np.nonzero((cnt > max_per_row)[row])[0]
            order = over[np.lexsort((col[over], -val[over], row[over]))]
            ocnt = np.where(cnt > max_per_row, cnt, 0)
            start = (np.cumsum(ocnt) - ocnt)[row[order]]
            drop = order[np.arange(len(order)) - start >= max_per_row]
            stay = np.ones(len(val), bool)
            stay[drop] = False
            row, col, val = row[stay], col[stay], val[stay]
    w = val if inflation == 1 else val * val if inflation == 2 else np.power(val, inflation)
    s = np.bincount(row, weights=w, minlength=n)
    out = w / s[row]
    mx = np.zeros(n)
    np.maximum.at(mx, row, out)
    chaos = float((mx - np.bincount(row, weights=out * out, minlength=n)).max(initial=0.0))
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    return rowptr, col.astype(np.uint32), out, chaos


def host_loop(ctx, dev, n, rows, cols, args, dt):
    _, rowptr, colidx, vals = graph.walk_pattern(rows, cols, n, None, dev)
    ci, va = colidx.to(torch.int32), vals.to(torch.float64 if dt == np.float64 else torch.float32)
    torch.cuda.synchronize(dev)
    pat = ctx.merge_csr_parts_device(dt, n, n, [(rowptr.data_ptr(), ci.data_ptr(), va.data_ptr())])
    T, _ = pat.inflate_prune(1.0, 0.0, 0)
    pat.close()
    log = []
    for it in range(args.max_iter):
        a = _result_as_input(T, dev)
        ptrs = (a.rows.data_ptr(), a.cols.data_ptr(), a.vals.data_ptr())
        exp = ctx.spgemm_coo_device(dt, n, n, n, a.nnz, ptrs, a.nnz, ptrs)
        t0 = time.perf_counter()
        C = exp.to_scipy()
        t1 = time.perf_counter()
        rp, cj, out, chaos = host_step(C, args.inflation, args.threshold, args.max_per_row)
        t2 = time.perf_counter()
        new = ctx.merge_csr_parts(n, n, [(rp, cj, out.astype(dt))])
        t3 = time.perf_counter()
        log.append({"iteration": it + 1, "ms_product": exp.info["ms_total"], "nnz_in": exp.nnz, "nnz_out": int(rp[-1]), "chaos": chaos,
                    "ms_download": (t1 - t0) * 1e3, "ms_host_step": (t2 - t1) * 1e3, "ms_upload": (t3 - t2) * 1e3,
                    "ms_round_trip": (t3 - t0) * 1e3})
        print(json.dumps({"what": "host-prune", **log[-1]}), flush=True)
        exp.close()
        torch.cuda.synchronize(dev)
        del a
        T.close()
        T = new
        if chaos < args.tol:
            break
    T.close()
    return log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--preset", default="g500")
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"])
    ap.add_argument("--inflation", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=1e-4)
    ap.add_argument("--max-per-row", type=int, default=1000)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--host-prune", action="store_true")
    ap.add_argument("--probe-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    dt = np.float64 if args.dtype == "f64" else np.float32
    vbytes = np.dtype(dt).itemsize
    dev = torch.device("cuda", 0)
    ctx = S.Context(0)
    n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, args.preset, seed=1)
    rows = torch.from_numpy(r.astype(np.int64)).to(dev)
    cols = torch.from_numpy(c.astype(np.int64)).to(dev)
    head = {"scale": args.scale, "edge_factor": args.edge_factor, "preset": args.preset, "dtype": args.dtype, "n": n, "edges": len(r)}
    copy_gbps = ctx.stream_copy_gbps(args.probe_bytes, 5)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if args.host_prune:
        log = host_loop(ctx, dev, n, rows, cols, args, dt)
        wall = time.perf_counter() - t0
        print(json.dumps({**head, "what": "host-prune summary", "iterations": len(log), "wall_s": wall, "copy_probe_GBps": copy_gbps,
                          "ms_product_sum": sum(x["ms_product"] for x in log), "ms_round_trip_sum": sum(x["ms_round_trip"] for x in log)}), flush=True)
    else:
        labels, info = graph.markov_cluster(rows, cols, n, inflation=args.inflation, threshold=args.threshold, max_per_row=args.max_per_row,
                                            max_iter=args.max_iter, tol=args.tol, dtype=dt, ctx=ctx)
        wall = time.perf_counter() - t0
        for it in range(info["iterations"]):
            nin, nout, ms = info["nnz_expanded"][it], info["nnz_kept"][it], info["ms_prune"][it]
            gbps = step_bytes(n, nin, nout, vbytes) / (ms * 1e-3) / 1e9
            print(json.dumps({"what": "device", "iteration": it + 1, "ms_product": info["ms_product"][it], "ms_prune": ms,
                              "ms_select": info["ms_select"][it], "nnz_in": nin, "nnz_out": nout, "rows_capped": info["rows_capped"][it],
                              "rows_long": info["rows_long"][it], "prune_GBps": gbps, "prune_over_copy": gbps / copy_gbps}), flush=True)
        print(json.dumps({**head, "what": "device summary", "iterations": info["iterations"], "converged": info["converged"],
                          "chaos": info["chaos"], "clusters": info["n_clusters"], "wall_s": wall, "copy_probe_GBps": copy_gbps,
                          "ms_product_sum": sum(info["ms_product"]), "ms_prune_sum": sum(info["ms_prune"])}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
