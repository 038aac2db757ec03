#!/usr/bin/env python3
"""Times osp_csr_reduce and osp_csr_select_vertices (MEASUREMENTS.md section 0i) on two inputs: the self-product of the R-MAT
matrix at --scale (--preset uniform), millions of short rows, and the `frontier` shape, ONE row of 2^20 entries.

reduce    rows and columns, plus and count: the smallest and the largest device time of --reps calls, the bytes a row reduce
          must read (row pointers and values) over that time beside what a plain copy reaches in the same run
          (osp_stream_copy_probe), and the torch formulation graph.py would otherwise use -- torch.zeros(M).index_add_ over
          osp_result_coo_rows' row array -- timed with torch events around the library call and the index_add_.
select    select_vertices with a 50 % keep vector on rows, on columns and on both, beside osp_csr_select with a position
          predicate ("triu") on the same input: the same three passes plus one gather.
Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402


def spread(times):
    return {"ms_min": min(times), "ms_max": max(times)}


def torch_row_sum(res, dev, reps):
    """torch.zeros(M).index_add_(0, rows, vals) with rows from osp_result_coo_rows: wall time between two torch events."""
    from outerspace_amd.distributed import _as_tensor
    M = res.shape[0]
    vals = _as_tensor(res.device_ptrs()[2], res.nnz, "<f8", dev, torch.float64)
    times = []
    for _ in range(reps):
        rows = torch.empty(max(res.nnz, 1), dtype=torch.int32, device=dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        res.coo_rows_into(rows.data_ptr())          # (synchronous on the library's stream)
        out = torch.zeros(M, dtype=torch.float64, device=dev)
        out.index_add_(0, rows[:res.nnz].to(torch.int64), vals)
        b.record()
        torch.cuda.synchronize(dev)
        times.append(a.elapsed_time(b))
    return out, times


def run(ctx, dev, name, res, reps, copy_gbps, head):
    M, N = res.shape
    for axis in ("rows", "cols"):
        for op in ("plus", "count"):
            sts = [res.reduce(axis, op)[1] for _ in range(reps)]
            times = [s["ms_total"] for s in sts]
            line = {**head, "input": name, "what": "reduce", "axis": axis, "op": op, "M": M, "N": N, "nnz": res.nnz, **spread(times),
                    "long_segments": sts[0]["long_segments"], "launches": sts[0]["launches"]}
            if axis == "rows" and op == "plus":
                nbytes = (M + 1) * 8 + res.nnz * 8 + M * 8
                line["GBps"] = nbytes / (min(times) * 1e-3) / 1e9
                line["copy_probe_GBps"] = copy_gbps
            print(json.dumps(line), flush=True)
    ours = res.reduce("rows", "plus")[0]
    out, times = torch_row_sum(res, dev, reps)
    print(json.dumps({**head, "input": name, "what": "torch index_add_ over coo_rows", **spread(times),
                      "max_abs_diff_to_reduce": float(np.abs(out.cpu().numpy() - ours).max()) if M else 0.0}), flush=True)
    rng = np.random.default_rng(2)
    kr = torch.from_numpy((rng.random(M) < 0.5).astype(np.uint8)).to(dev)
    kc = torch.from_numpy((rng.random(N) < 0.5).astype(np.uint8)).to(dev)
    torch.cuda.synchronize(dev)
    for what, args in (("rows", (kr, None)), ("cols", (None, kc)), ("both", (kr, kc))):
        sts = []
        for _ in range(reps):
            out_, st = res.select_vertices(*args)
            out_.close()
            sts.append(st)
        print(json.dumps({**head, "input": name, "what": "select_vertices", "sides": what, "nnz_in": sts[0]["nnz_in"],
                          "nnz_out": sts[0]["nnz_out"], "launches": sts[0]["launches"], **spread([s["ms_total"] for s in sts])}), flush=True)
    sts = []
    for _ in range(reps):
        out_, st = res.select("triu")
        out_.close()
        sts.append(st)
    print(json.dumps({**head, "input": name, "what": "select triu", "nnz_in": sts[0]["nnz_in"], "nnz_out": sts[0]["nnz_out"],
                      "launches": sts[0]["launches"], **spread([s["ms_total"] for s in sts])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--preset", default="uniform")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import scipy.sparse as sp
    ctx = S.Context(0)
    dev = torch.device("cuda", 0)
    copy_gbps = ctx.stream_copy_gbps(1 << 30, 5)
    head = {"scale": args.scale, "preset": args.preset, "reps": args.reps}
    n, r, c, v = gen.rmat_coo(args.scale, args.edge_factor, args.preset, seed=1)
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    prod = ctx.spgemm_csc_csr(n, n, n, A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data,
                              B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data, validate=False)
    run(ctx, dev, "product", prod, args.reps, copy_gbps, head)
    prod.close()
    m, ncol = 1 << 20, 1 << 21
    rng = np.random.default_rng(5)
    col = np.sort(rng.choice(ncol, size=m, replace=False)).astype(np.uint32)
    front = ctx.merge_csr_parts(1, ncol, [(np.array([0, m], np.int64), col, rng.standard_normal(m))])
    run(ctx, dev, "frontier", front, args.reps, copy_gbps, head)
    front.close()
    ctx.close()


if __name__ == "__main__":
    main()
