#!/usr/bin/env python3
"""Times graph.k_truss and the entry filter osp_csr_select on the R-MAT generator's graph at --scale (MEASUREMENTS.md
section 0e).  Three forms:

(default)        graph.k_truss for --k.  Per round: the device times of the support product and of the filter
                 (select "ge" k - 2 with fill), the entries in and out, and the filter's achieved bytes per second beside what
                 a plain copy reaches in the same run (osp_stream_copy_probe).
--host-select    the same loop the way a user had to write it before the filter existed: every round's supports copied to
                 the host, filtered with numpy, and uploaded again; per round the host clock around that round trip.
--standalone     no graph: on the self-product of the R-MAT matrix (--preset uniform), select of each class -- a value
                 predicate that keeps everything, one that keeps half, the same with fill, a position predicate that keeps
                 everything, one that keeps the upper triangle, the same with fill -- and apply_mask with the product's own
                 pattern on the same result in the same run, ALTERNATING call by call, --reps repetitions after --warmup:
                 medians, spread (max - min), and whether the median stays within apply_mask's median + apply_mask's spread.

The bytes a select call must move (select_bytes):
    flag    value predicate: nnz_in * vbytes;  position predicate: nnz_in * 4 + (M + 1) * 8
    bits    one word per 64 entries, written once and read twice (scan, write): 3 * nnz_in / 8
    scan    one u64 position per word, written and read: 2 * nnz_in / 8
    write   kept entries read (columns; values unless fill) and written (columns and values):
            nnz_out * (4 + (0 if fill else vbytes)) + nnz_out * (4 + vbytes), and the row pointers read and written: 2 * (M + 1) * 8
apply_mask's bytes are tools/time_bfs.py's filter_bytes.
Prints one JSON line per round (or per case) and a summary line."""
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

POSITION_OPS = ("tril", "triu", "diag", "offdiag")


def select_bytes(nrow, nnz_in, nnz_out, op, fill, vbytes=8):
    flag = nnz_in * 4 + (nrow + 1) * 8 if op in POSITION_OPS else nnz_in * vbytes
    return (flag + 5 * nnz_in // 8 + nnz_out * (4 + (0 if fill else vbytes)) + nnz_out * (4 + vbytes) + 2 * (nrow + 1) * 8)


def filter_bytes(nrow, nnz_in, nnz_mask, nnz_out, vbytes=8):
    return (nnz_in + nnz_out) * (4 + vbytes) + nnz_mask * 4 + 3 * (nrow + 1) * 8


def host_select_step(ctx, clock):
    """The step between two support products without osp_csr_select: download, numpy, upload."""
    cmp = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}

    def run(result, op, threshold=0.0, fill=None):
        t0 = time.perf_counter()
        rowptr, col, val = result.to_host()
        t1 = time.perf_counter()
        keep = cmp[op](val, threshold)
        row = np.repeat(np.arange(result.shape[0]), np.diff(rowptr))[keep]
        ptr = np.zeros(result.shape[0] + 1, np.int64)
        ptr[1:] = np.cumsum(np.bincount(row, minlength=result.shape[0]))
        out_val = val[keep] if fill is None else np.full(int(keep.sum()), fill, val.dtype)
        t2 = time.perf_counter()
        out = ctx.merge_csr_parts(result.shape[0], result.shape[1], [(ptr, col[keep], out_val)])
        t3 = time.perf_counter()
        clock.append({"ms_download": (t1 - t0) * 1e3, "ms_host_filter": (t2 - t1) * 1e3, "ms_upload": (t3 - t2) * 1e3,
                      "ms_round_trip": (t3 - t0) * 1e3})
        return out, {"nnz_in": len(col), "nnz_out": int(keep.sum()), "ms_total": (t3 - t0) * 1e3}
    return run


def run_truss(ctx, dev, args, n, rows, cols, copy_gbps, head):
    clock = []
    step = host_select_step(ctx, clock) if args.host_select else None
    what = "host-select" if args.host_select else "device"
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    u, v, info = graph._k_truss(rows, cols, n, args.k, np.float64, ctx, select_step=step)
    wall = time.perf_counter() - t0
    for d in range(info["rounds"]):
        nin, nout, ms = info["nnz_support"][d], info["nnz_kept"][d], info["ms_select"][d]
        line = {"what": what, "round": d + 1, "nnz_graph": info["nnz_graph"][d], "nnz_support": nin, "nnz_kept": nout,
                "ms_product": info["ms_product"][d]}
        if args.host_select:
            line.update(clock[d])
        else:
            gbps = select_bytes(n, nin, nout, "ge", True) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            line.update({"ms_select": ms, "select_GBps": gbps, "select_over_copy": gbps / copy_gbps})
        print(json.dumps(line), flush=True)
    print(json.dumps({**head, "what": what + " summary", "k": args.k, "rounds": info["rounds"], "truss_edges": len(u), "wall_s": wall,
                      "copy_probe_GBps": copy_gbps, "ms_product_sum": sum(info["ms_product"]), "ms_select_sum": sum(info["ms_select"])}),
          flush=True)


def run_standalone(ctx, dev, args, n, r, c, v, copy_gbps, head):
    import scipy.sparse as sp
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    prod = ctx.spgemm_csc_csr(n, n, n, A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data,
                              B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data, validate=False)
    median = float(np.median(prod.vals))
    inf = float("inf")
    cases = {"apply_mask own pattern": None,
             "select ge -inf (keeps all)": ("ge", {"threshold": -inf}, None),
             "select ge median": ("ge", {"threshold": median}, None),
             "select ge median fill": ("ge", {"threshold": median}, 1.0),
             "select tril N (keeps all)": ("tril", {"diag": n}, None),
             "select triu 1": ("triu", {"diag": 1}, None),
             "select triu 1 fill": ("triu", {"diag": 1}, 1.0)}
    times = {name: [] for name in cases}
    last = {}
    for rep in range(args.warmup + args.reps):
        for name, case in cases.items():      # alternating: every case once per repetition
            if case is None:
                res, st = prod.apply_mask(prod)
            else:
                res, st = prod.select(case[0], fill=case[2], **case[1])
            res.close()
            if rep >= args.warmup:
                times[name].append(st["ms_total"])
                last[name] = st
    am = np.array(times["apply_mask own pattern"])
    am_median, am_spread = float(np.median(am)), float(am.max() - am.min())
    for name, case in cases.items():
        t, st = np.array(times[name]), last[name]
        if case is None:
            nbytes = filter_bytes(n, st["nnz_in"], st["nnz_mask"], st["nnz_out"])
        else:
            nbytes = select_bytes(n, st["nnz_in"], st["nnz_out"], case[0], case[2] is not None)
        med = float(np.median(t))
        gbps = nbytes / (med * 1e-3) / 1e9
        line = {**head, "what": "standalone", "case": name, "nnz_in": st["nnz_in"], "nnz_out": st["nnz_out"], "launches": st["launches"],
                "reps": len(t), "ms_median": med, "ms_min": float(t.min()), "ms_max": float(t.max()), "ms_spread": float(t.max() - t.min()),
                "bytes": nbytes, "GBps": gbps, "over_copy": gbps / copy_gbps}
        if case is not None:
            line["within_apply_mask_median_plus_spread"] = bool(med <= am_median + am_spread)
        print(json.dumps(line), flush=True)
    print(json.dumps({**head, "what": "standalone summary", "apply_mask_ms_median": am_median, "apply_mask_ms_spread": am_spread,
                      "copy_probe_GBps": copy_gbps}), flush=True)
    if args.host_select:
        clock = []
        prod._host = None   # (the median above cached the host copy: download again)
        out, _ = host_select_step(ctx, clock)(prod, "ge", median)
        out.close()
        print(json.dumps({**head, "what": "standalone host round trip", **clock[0]}), flush=True)
    prod.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--preset", default="g500")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--host-select", action="store_true")
    ap.add_argument("--standalone", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--probe-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = S.Context(0)
    n, r, c, v = gen.rmat_coo(args.scale, args.edge_factor, args.preset, seed=1)
    head = {"scale": args.scale, "edge_factor": args.edge_factor, "preset": args.preset, "n": n, "edges": len(r)}
    copy_gbps = ctx.stream_copy_gbps(args.probe_bytes, 5)
    if args.standalone:
        run_standalone(ctx, dev, args, n, r, c, v, copy_gbps, head)
    else:
        rows = torch.from_numpy(r.astype(np.int64)).to(dev)
        cols = torch.from_numpy(c.astype(np.int64)).to(dev)
        run_truss(ctx, dev, args, n, rows, cols, copy_gbps, head)
    ctx.close()


if __name__ == "__main__":
    main()
