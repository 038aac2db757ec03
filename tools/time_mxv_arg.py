#!/usr/bin/env python3
"""Times osp_csr_mxv_arg against osp_csr_mxv and against the composition it replaces (MEASUREMENTS.md section 0u).  One
process; run it under one `timeout`.

tools/time_mxv.py's three shapes (adjacency, product, frontier; its builders are imported), each in f64 and f32, x random on
the device, under (min, times) -- a position needs MIN or MAX, so the sum of time_mxv.py has no counterpart here.  On each,
alternating within the process after one warm-up call of each, --reps times, median and smallest - largest reported:
  (a) A.mxv_arg(x, "min", "times")                    y and arg
  (p) A.mxv_arg(x, "min", "times", values=False)      arg only
  (m) A.mxv(x, "min", "times")                        y only: what the extra pair is paid on top of
  (c) the composition a user needed before: y = A.mxv(x, "min", "times"); P = A.apply_vectors(cols=x, col_op="times");
      D = P.apply_vectors(rows=y, row_op="minus"); Z = D.select("eq", 0); arg = Z.mxv(ids, "min", "second")
Device times from the calls' own hipEvents (stats ms_total; (c) is the sum of its five calls).  The tool refuses to go on
when (a) and (m) differ in one bit of y, or (a) and (c) in one position of a row that has entries.  --mxv-only times (m)
alone and touches nothing but ``mxv``: run that way from a checkout of another commit, it is the other side of an A/B of the
unchanged mxv.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402
from time_mxv import bits, frontier, symmetric_adjacency  # noqa: E402

ADD, MUL = "min", "times"


def spread(times):
    return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}


def bytes_model(M, nnz, V, y=True, arg=True):
    """The bytes the call cannot avoid: the row pointers, every column and value once, one gather of x per entry, and per row
    y (V bytes) and arg (8 bytes) as far as they are written."""
    return 8 * (M + 1) + nnz * (4 + V + V) + M * (V * y + 8 * arg)


def composition(A, x, ids, y, col):
    _, s0 = A.mxv(x, ADD, MUL, out=y)
    P, s1 = A.apply_vectors(cols=x, col_op="times")
    D, s2 = P.apply_vectors(rows=y, row_op="minus")
    Z, s3 = D.select("eq", 0)
    _, s4 = Z.mxv(ids, "min", "second", out=col)
    for r in (P, D, Z):
        r.close()
    steps = (s0, s1, s2, s3, s4)
    return sum(s["ms_total"] for s in steps), sum(s["launches"] for s in steps)


def time_shape(head, name, A, reps, mxv_only):
    M, N = A.shape
    V = np.dtype(A.dtype).itemsize
    tdt = torch.float32 if A.dtype == np.float32 else torch.float64
    dev = f"cuda:{A._ctx.device}"
    x = torch.rand(N, dtype=tdt, device=dev) + 0.5
    ids = torch.arange(N, device=dev).to(tdt)
    ya, ym, yc, col = (torch.empty(M, dtype=tdt, device=dev) for _ in range(4))
    arg, argp = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    row = np.diff(A.rowptr)
    head = {**head, "shape": name, "M": M, "N": N, "nnz": A.nnz, "row_mean": float(row.mean()) if M else 0.0, "row_max": int(row.max()) if M else 0,
            "semiring": f"{ADD}.{MUL}"}
    gbs = lambda b, ms: b / ms / 1e6   # noqa: E731
    ta, tp, tm, tc, sa, launches_c = [], [], [], [], None, 0
    for rep in range(reps + 1):
        _, sm = A.mxv(x, ADD, MUL, out=ym)
        if not mxv_only:
            _, _, sa = A.mxv_arg(x, ADD, MUL, out=ya, out_arg=arg)
            _, _, sp = A.mxv_arg(x, ADD, MUL, out_arg=argp, values=False)
            ms_c, launches_c = composition(A, x, ids, yc, col)
        if rep == 0:
            if not mxv_only:
                if not torch.equal(bits(ya), bits(ym)):
                    sys.exit(f"{name}: mxv_arg's y and mxv's differ in {int((bits(ya) != bits(ym)).sum())} values: not timing a wrong result")
                has = arg >= 0
                if not torch.equal(arg[has], col[has].long()) or not torch.equal(arg, argp):
                    sys.exit(f"{name}: mxv_arg and the composition disagree on a position: not timing a wrong result")
            continue
        tm.append(sm["ms_total"])
        if not mxv_only:
            ta.append(sa["ms_total"])
            tp.append(sp["ms_total"])
            tc.append(ms_c)
    b = bytes_model(M, A.nnz, V, arg=False)
    print(json.dumps({**head, "case": "(m) mxv", "group": sm["group"], "launches": sm["launches"], **spread(tm), "bytes_model": b,
                      "gbps_at_median": gbs(b, statistics.median(tm))}), flush=True)
    if mxv_only:
        return
    med = statistics.median
    b = bytes_model(M, A.nnz, V)
    print(json.dumps({**head, "case": "(a) mxv_arg", "group": sa["group"], "launches": sa["launches"], "long_segments": sa["long_segments"],
                      "rows_without": sa["rows_without"], **spread(ta), "bytes_model": b, "gbps_at_median": gbs(b, med(ta)),
                      "a_over_m": med(ta) / med(tm), "equal_bits": True}), flush=True)
    b = bytes_model(M, A.nnz, V, y=False)
    print(json.dumps({**head, "case": "(p) mxv_arg, positions only", **spread(tp), "bytes_model": b, "gbps_at_median": gbs(b, med(tp)),
                      "p_over_m": med(tp) / med(tm)}), flush=True)
    print(json.dumps({**head, "case": "(c) mxv + 2 apply_vectors + select + mxv", "launches": launches_c, **spread(tc),
                      "c_over_a": med(tc) / med(ta), "equal_positions": True}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--mm-scale", type=int, default=14)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--shapes", default="adjacency,product,frontier")
    ap.add_argument("--mxv-only", action="store_true")
    args = ap.parse_args()
    ctx = S.Context(0)
    for name in args.dtypes.split(","):
        dt = np.float32 if name == "f32" else np.float64
        head = {"dtype": name, "reps": args.reps}
        shapes = args.shapes.split(",")
        if "adjacency" in shapes:
            n, (rowptr, col, val) = symmetric_adjacency(args.scale, args.edge_factor, dt)
            val = (np.random.default_rng(3).random(len(col)) + 0.5).astype(dt)   # (weights, not 0/1: a minimum worth looking for)
            A = ctx.merge_csr_parts(n, n, [(rowptr, col, val)])
            time_shape({**head, "scale": args.scale}, "adjacency", A, args.reps, args.mxv_only)
            A.close()
        if "product" in shapes:
            m, r, c, v = gen.rmat_coo(args.mm_scale, args.edge_factor, "g500", seed=1, dtype=dt)
            B = ctx.merge_csr_parts(m, m, [gen.coo_to_csr(m, r, c, v)])
            P, _ = B.mxm(B)
            B.close()
            time_shape({**head, "scale": args.mm_scale}, "product", P, args.reps, args.mxv_only)
            P.close()
        if "frontier" in shapes:
            n, csr = frontier(dt)
            F = ctx.merge_csr_parts(64, n, [csr])
            time_shape(head, "frontier", F, args.reps, args.mxv_only)
            F.close()
        ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
