#!/usr/bin/env python3
"""Times osp_csr_transpose and CsrResult.matmul (MEASUREMENTS.md section 0k).  One process; run it under one `timeout`.

Two shapes from generators.rmat_coo at --scale (default 22, edge factor 16, seed 1):
  adjacency  the n x n adjacency as a result (the sort path; the row-mask path does not apply)
  frontier   64 x n: the first --fold rows of the adjacency folded onto 64 rows (row r goes to r % 64), duplicates merged
On each: the row-mask path where it applies, the sort path with the packed gather (a) and with the bisecting gather (b)
(OSP_TRANSPOSE_PATH / OSP_TRANSPOSE_GATHER, read per call), device times from the call's own hipEvents (stats ms_total), one
warm-up call, smallest - largest of --reps; and the only route of the parent commit, wall clock: to_host + scipy
.T.tocsr() + merge_csr_parts.  Every variant's arrays are compared with the round trip's.  Beside every time: the bytes the
path must move (bytes_model below) and what moving them takes at the measured stream-copy rate (osp_stream_copy_probe).
Then matmul against mxm(plus, times) on the R-MAT --mm-scale (default 16) self-product.  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402


def spread(times):
    return {"ms_min": min(times), "ms_max": max(times)}


def bytes_model(variant, nnz, N, V, passes):
    """HBM bytes a path cannot avoid, every array read or written once per kernel that needs it (bisections and the scans'
    tile sums left out).  V: bytes of a value; a packed record is 8 bytes at V = 4 and 16 at V = 8."""
    if variant == "rowmask":
        # zero N words; pass 1 reads the columns (atomics on N words: counted once); scan reads N words, writes N + 1 pointers;
        # pass 3 reads columns and values and the pointers / words by column, writes columns and values
        return nnz * (4 + 4 + V + 4 + V) + N * (8 + 8 + 8 + 8)
    R = 8 if V == 4 else 16
    # per pass: the histogram reads the keys; the scatter reads keys (and positions after the first pass) and writes both
    # (not in the last pass); the last pass writes column, value and the sorted key; the pointer kernel writes N + 1 pointers
    sort = nnz * (4 * passes + 4 * passes + 4 * (passes - 1) + 8 * (passes - 1) + 4 + V + 4) + 8 * N
    if variant == "pack":
        return sort + nnz * (4 + V + R) + nnz * R      # the pack kernel (columns, values in, records out), one record gathered
    return sort + nnz * V                               # the value gathered by itself


def same(a, b):
    bits = np.uint32 if a[2].dtype == np.float32 else np.uint64
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(bits), b[2].view(bits)))


def time_shape(ctx, head, name, M, N, csr, reps, gbps):
    V = csr[2].dtype.itemsize
    nnz = len(csr[1])
    src = ctx.merge_csr_parts(M, N, [csr])
    # the parent commit's only route
    walls, ref = [], None
    for rep in range(2):
        src._host = None
        t0 = time.perf_counter()
        rp, ci, va = src.to_host()
        T = sp.csr_matrix((va, ci.astype(np.int64), rp), shape=(M, N)).T.tocsr()
        T.sort_indices()
        back = ctx.merge_csr_parts(N, M, [(T.indptr.astype(np.int64), T.indices.astype(np.uint32), T.data)])
        walls.append((time.perf_counter() - t0) * 1e3)
        ref = (T.indptr.astype(np.int64), T.indices.astype(np.uint32), T.data)
        back.close()
    print(json.dumps({**head, "shape": name, "M": M, "N": N, "nnz": nnz, "case": "host round trip (wall)", **spread(walls)}), flush=True)
    variants = [("sort, packed gather (a)", "pack", {"OSP_TRANSPOSE_PATH": "sort"}),
                ("sort, bisecting gather (b)", "bisect", {"OSP_TRANSPOSE_PATH": "sort", "OSP_TRANSPOSE_GATHER": "bisect"})]
    if M <= 64:
        variants.insert(0, ("row mask", "rowmask", {}))
    for label, variant, env in variants:
        for k in ("OSP_TRANSPOSE_PATH", "OSP_TRANSPOSE_GATHER"):
            os.environ.pop(k, None)
        os.environ.update(env)
        times, st, ok = [], None, None
        for rep in range(reps + 1):
            res, st = src.transpose()
            if rep == 0:
                ok = same(res.to_host(), ref)
            else:
                times.append(st["ms_total"])
            res.close()
        b = bytes_model(variant, nnz, N, V, st["passes"])
        print(json.dumps({**head, "shape": name, "case": label, "path": st["path"], "passes": st["passes"], "launches": st["launches"],
                          **spread(times), "equals_round_trip": ok, "bytes_model": b, "ms_at_copy_rate": b / (gbps * 1e9) * 1e3,
                          "copy_rate_share": b / (gbps * 1e9) * 1e3 / min(times), "round_trip_over_this": min(walls) / min(times)}), flush=True)
    for k in ("OSP_TRANSPOSE_PATH", "OSP_TRANSPOSE_GATHER"):
        os.environ.pop(k, None)
    src.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--fold", type=int, default=1 << 18, help="rows of the adjacency folded into the 64-row frontier")
    ap.add_argument("--mm-scale", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dt = np.float32 if args.dtype == "f32" else np.float64
    ctx = S.Context(0)
    gbps = ctx.stream_copy_gbps()
    head = {"scale": args.scale, "dtype": args.dtype, "reps": args.reps, "copy_gbps": gbps}
    n, r, c, v = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1, dtype=dt)
    print(json.dumps({**head, "case": "generated", "n": n, "nnz": len(r)}), flush=True)
    time_shape(ctx, head, "adjacency", n, n, gen.coo_to_csr(n, r, c, v), args.reps, gbps)
    low = r < min(args.fold, n)
    key = np.unique((r[low].astype(np.int64) % 64) * n + c[low].astype(np.int64))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=64))]).astype(np.int64)
    frontier = (rowptr, (key % n).astype(np.uint32), np.random.default_rng(2).random(len(key)).astype(dt) + dt(0.5))
    time_shape(ctx, head, "frontier", 64, n, frontier, args.reps, gbps)
    # matmul (transpose + the outer-product pipeline) against mxm(plus, times)
    m, r, c, v = gen.rmat_coo(args.mm_scale, args.edge_factor, "g500", seed=1, dtype=dt)
    A = ctx.merge_csr_parts(m, m, [gen.coo_to_csr(m, r, c, v)])
    t_mm, t_mxm, t_tr, ok, st = [], [], [], None, None
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        P = A.matmul(A)
        wall = (time.perf_counter() - t0) * 1e3
        At, tst = A.transpose()
        At.close()
        Q, st = A.mxm(A)
        if rep == 0:
            ok = same(P.to_host(), Q.to_host())
        else:
            t_mm.append((wall, P.info["ms_total"]))
            t_tr.append(tst["ms_total"])
            t_mxm.append(st["ms_total"])
        P.close()
        Q.close()
    print(json.dumps({**head, "case": "matmul against mxm(plus, times)", "mm_scale": args.mm_scale, "products": st["products"],
                      "matmul_wall": spread([w for w, _ in t_mm]), "matmul_product_device": spread([d for _, d in t_mm]),
                      "transpose_device": spread(t_tr), "mxm_device": spread(t_mxm), "bit_identical": ok,
                      "mxm_over_transpose_plus_product": min(t_mxm) / (min(t_tr) + min(d for _, d in t_mm))}), flush=True)
    A.close()
    ctx.close()


if __name__ == "__main__":
    main()
