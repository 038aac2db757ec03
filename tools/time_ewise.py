#!/usr/bin/env python3
"""Times osp_csr_ewise and graph.personalized_pagerank on the R-MAT generator's graph (MEASUREMENTS.md section 0h).  Two forms:

(default)   no graph: the self-product of the R-MAT matrix at --scale (--preset uniform) against its own every-second-entry
            thinning, union (plus, first) and intersect (times), the best of --reps calls each: device time, the bytes the
            call must move -- columns and values of a, b and out, and the three row pointer arrays -- over that time,
            beside what a plain copy reaches in the same run (osp_stream_copy_probe), and for comparison the same union by
            the sorting merge (merge_csr_parts_device) and the mask filter on the same pair.
--pagerank  graph.personalized_pagerank from --sources vertices (the highest degrees) at --scale (--preset g500), --steps
            steps, with --prune: per step the device times of the product, the select and the union.
Prints one JSON line per case (or per step) and, for --pagerank, a summary line."""
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


def ewise_bytes(nrow, nnz_a, nnz_b, nnz_out, vbytes=8):
    """What one call must read and write: columns and values of a, b and out, three row pointer arrays."""
    return (nnz_a + nnz_b + nnz_out) * (4 + vbytes) + 3 * (nrow + 1) * 8


def run_standalone(ctx, dev, args, n, r, c, v, copy_gbps, head):
    import scipy.sparse as sp
    from outerspace_amd.distributed import _as_tensor
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    prod = ctx.spgemm_csc_csr(n, n, n, A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data,
                              B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data, validate=False)
    rp, ci, va = prod.device_ptrs()
    rowptr = _as_tensor(rp, n + 1, "<i8", dev, torch.int64)
    col = _as_tensor(ci, prod.nnz, "<i4", dev, torch.int32)
    val = _as_tensor(va, prod.nnz, "<f8", dev, torch.float64)
    # every second entry of the product, by position, as a result of its own
    t_col, t_val, t_rowptr = col[::2].contiguous(), val[::2].contiguous(), (rowptr + 1) // 2
    torch.cuda.synchronize(dev)
    thin = ctx.merge_csr_parts_device(np.float64, n, n, [(t_rowptr.data_ptr(), t_col.data_ptr(), t_val.data_ptr())])
    cases = [("union", "plus", prod, thin), ("union", "first", prod, thin), ("union", "plus", thin, prod), ("intersect", "times", prod, thin),
             ("intersect", "times", thin, prod)]
    for mode, op, a, b in cases:
        best = None
        for _ in range(args.reps):
            res, st = a.ewise(b, mode, op)
            res.close()
            best = st if best is None or st["ms_total"] < best["ms_total"] else best
        gbps = ewise_bytes(n, best["nnz_a"], best["nnz_b"], best["nnz_out"]) / (best["ms_total"] * 1e-3) / 1e9
        print(json.dumps({**head, "what": "standalone", "mode": mode, "op": op, "a": "product" if a is prod else "thinned", **best,
                          "GBps": gbps, "over_copy": gbps / copy_gbps, "copy_probe_GBps": copy_gbps}), flush=True)
    best = None
    for _ in range(args.reps):
        res = ctx.merge_csr_parts_device(np.float64, n, n, [prod.device_ptrs(), thin.device_ptrs()])
        ms, nnz = res.info["ms_total"], res.nnz
        res.close()
        best = ms if best is None else min(best, ms)
    print(json.dumps({**head, "what": "standalone", "mode": "sorting merge of the two parts", "nnz_out": nnz, "ms_total": best}), flush=True)
    best = None
    for _ in range(args.reps):
        res, st = prod.apply_mask(thin)
        res.close()
        best = st if best is None or st["ms_total"] < best["ms_total"] else best
    print(json.dumps({**head, "what": "standalone", "mode": "apply_mask of the same pair", **best}), flush=True)
    del rowptr, col, val
    thin.close()
    prod.close()


def run_pagerank(ctx, dev, args, n, r, c, head):
    deg = np.bincount(r, minlength=n) + np.bincount(c, minlength=n)
    src = np.argsort(-deg, kind="stable")[:args.sources].astype(np.int64)
    rows = torch.from_numpy(r.astype(np.int64)).to(dev)
    cols = torch.from_numpy(c.astype(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ppr, info = graph.personalized_pagerank(rows, cols, n, src, max_iter=args.steps, prune=args.prune, ctx=ctx)
    wall = time.perf_counter() - t0
    for k in range(info["iterations"]):
        print(json.dumps({"what": "pagerank", "step": k + 1, **{key: info[key][k] for key in ("frontier_nnz", "nnz_result", "ms_product", "ms_select",
                                                                                               "ms_union")}}), flush=True)
    print(json.dumps({**head, "what": "pagerank summary", "sources": len(src), "steps": info["steps"], "iterations": info["iterations"],
                      "prune": args.prune, "wall_s": wall, "row_sum_min": float(ppr.sum(1).min()), "ms_product_sum": sum(info["ms_product"]),
                      "ms_select_sum": sum(info["ms_select"]), "ms_union_sum": sum(info["ms_union"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--preset", default=None)
    ap.add_argument("--pagerank", action="store_true")
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--prune", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    preset = args.preset or ("g500" if args.pagerank else "uniform")
    dev = torch.device("cuda", 0)
    ctx = S.Context(0)
    n, r, c, v = gen.rmat_coo(args.scale, args.edge_factor, preset, seed=1)
    head = {"scale": args.scale, "edge_factor": args.edge_factor, "preset": preset, "n": n, "edges": len(r)}
    if args.pagerank:
        run_pagerank(ctx, dev, args, n, r, c, head)
    else:
        run_standalone(ctx, dev, args, n, r, c, v.astype(np.float64), ctx.stream_copy_gbps(args.probe_bytes, 5), head)
    ctx.close()


if __name__ == "__main__":
    main()
