#!/usr/bin/env python3
"""Times osp_csr_mxv against the composition it fuses (MEASUREMENTS.md section 0l).  One process; run it under one `timeout`.

Three shapes, each in f64 and f32 (--dtypes), x random on the device:
  adjacency  the symmetric 0/1 adjacency of generators.rmat_coo at --scale (default 20, edge factor 16, seed 1): short rows
  product    the self-product of the R-MAT --mm-scale (default 14) matrix: rows of hundreds
  frontier   64 x 2^20 with one row of 2^19 entries and 63 rows of 2^10
On each, alternating within the process after one warm-up call of both, --reps times, smallest - largest reported:
  (a) A.mxv(x)                                                          (plus, times)
  (b) apply_vectors(cols=x, col_op="times") + reduce("rows", "plus") + close(): the only route at the parent commit
Device times from the calls' own hipEvents (stats ms_total; (b) is the sum of its two calls).  The tool refuses to go on
when (a) and (b) differ in one bit.  Beside every time: GB/s on the algorithmic bytes (bytes_model below).  The adjacency is
also run once per OSP_MXV_GROUP value.  Prints one JSON line per case."""
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

GROUPS = [4, 8, 16, 32, 64]


def spread(times):
    return {"ms_min": min(times), "ms_max": max(times)}


def bytes_model(M, nnz, V):
    """The bytes y = A x cannot avoid: the row pointers, every column and value once, one gather of x per entry, y once."""
    return 8 * (M + 1) + nnz * (4 + V + V) + M * V


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def composition(A, x, y):
    prod, s1 = A.apply_vectors(cols=x, col_op="times")
    _, s2 = prod.reduce("rows", "plus", out=y)
    prod.close()
    return s1["ms_total"] + s2["ms_total"], s1["launches"] + s2["launches"]


def time_shape(head, name, A, reps, groups=False):
    M, N = A.shape
    V = np.dtype(A.dtype).itemsize
    tdt = torch.float32 if A.dtype == np.float32 else torch.float64
    dev = f"cuda:{A._ctx.device}"
    x = torch.rand(N, dtype=tdt, device=dev) + 0.5
    ya, yb = torch.empty(M, dtype=tdt, device=dev), torch.empty(M, dtype=tdt, device=dev)
    torch.cuda.synchronize()
    b = bytes_model(M, A.nnz, V)
    row = np.diff(A.rowptr)
    head = {**head, "shape": name, "M": M, "N": N, "nnz": A.nnz, "row_mean": float(row.mean()) if M else 0.0, "row_max": int(row.max()) if M else 0,
            "bytes_model": b}
    ta, tb, st = [], [], None
    for rep in range(reps + 1):
        _, st = A.mxv(x, out=ya)
        ms_b, launches_b = composition(A, x, yb)
        if rep == 0:
            if not torch.equal(bits(ya), bits(yb)):
                sys.exit(f"{name}: mxv and the composition differ in {int((bits(ya) != bits(yb)).sum())} values: not timing a wrong result")
        else:
            ta.append(st["ms_total"])
            tb.append(ms_b)
    gbs = lambda ms: b / ms / 1e6   # noqa: E731
    print(json.dumps({**head, "case": "(a) mxv", "group": st["group"], "launches": st["launches"], "long_segments": st["long_segments"],
                      **spread(ta), "gbps_at_min": gbs(min(ta))}), flush=True)
    print(json.dumps({**head, "case": "(b) apply_vectors + reduce", "launches": launches_b, **spread(tb), "gbps_at_min": gbs(min(tb)),
                      "b_over_a": min(tb) / min(ta), "b_over_a_worst": min(tb) / max(ta), "equal_bits": True}), flush=True)
    if groups:
        for g in GROUPS:
            os.environ["OSP_MXV_GROUP"] = str(g)
            tg = []
            for rep in range(reps + 1):
                _, st = A.mxv(x, out=yb)
                if rep == 0:
                    if not torch.equal(bits(ya), bits(yb)):
                        sys.exit(f"{name}: OSP_MXV_GROUP={g} changes the result")
                else:
                    tg.append(st["ms_total"])
            print(json.dumps({**head, "case": f"mxv, OSP_MXV_GROUP={g}", "group": st["group"], **spread(tg), "gbps_at_min": gbs(min(tg))}), flush=True)
        os.environ.pop("OSP_MXV_GROUP", None)


def symmetric_adjacency(scale, edge_factor, dt):
    n, r, c, _ = gen.rmat_coo(scale, edge_factor, "g500", seed=1)
    r, c = r.astype(np.int64), c.astype(np.int64)
    keep = r != c
    key = np.unique(np.concatenate([r[keep] * n + c[keep], c[keep] * n + r[keep]]))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int64)
    return n, (rowptr, (key % n).astype(np.uint32), np.ones(len(key), dt))


def frontier(dt):
    n = 1 << 20
    rng = np.random.default_rng(2)
    lengths = [1 << 19] + [1 << 10] * 63
    col = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lengths]).astype(np.uint32)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return n, (rowptr, col, (rng.random(len(col)) + 0.5).astype(dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--mm-scale", type=int, default=14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--shapes", default="adjacency,product,frontier")
    args = ap.parse_args()
    ctx = S.Context(0)
    for name in args.dtypes.split(","):
        dt = np.float32 if name == "f32" else np.float64
        head = {"dtype": name, "reps": args.reps}
        shapes = args.shapes.split(",")
        if "adjacency" in shapes:
            n, csr = symmetric_adjacency(args.scale, args.edge_factor, dt)
            A = ctx.merge_csr_parts(n, n, [csr])
            time_shape({**head, "scale": args.scale}, "adjacency", A, args.reps, groups=True)
            A.close()
        if "product" in shapes:
            m, r, c, v = gen.rmat_coo(args.mm_scale, args.edge_factor, "g500", seed=1, dtype=dt)
            B = ctx.merge_csr_parts(m, m, [gen.coo_to_csr(m, r, c, v)])
            P, _ = B.mxm(B)
            B.close()
            time_shape({**head, "scale": args.mm_scale}, "product", P, args.reps)
            P.close()
        if "frontier" in shapes:
            n, csr = frontier(dt)
            F = ctx.merge_csr_parts(64, n, [csr])
            time_shape(head, "frontier", F, args.reps)
            F.close()
        ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
