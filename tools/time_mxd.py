#!/usr/bin/env python3
"""Times osp_csr_mxd against k calls of osp_csr_mxv on contiguous columns (MEASUREMENTS.md section 0q).  One process; run it
under one `timeout`.

Shapes (--shapes), each in f64 and f32 (--dtypes), X random on the device, at every k of --ks (default 1,4,16,64,256):
  adjacency  the symmetric 0/1 adjacency of generators.rmat_coo at every scale of --scales (default 18,20; edge factor 16)
  product    the self-product of the R-MAT --mm-scale (default 14) matrix: rows of hundreds
  frontier   16 x 2^21 with rows of 2^20 entries
On each, after one warm-up of both, --reps times (default 20), smallest - largest reported:
  (a) A.mxd(X)                                             (plus, times)
  (b) A.mxv(Xt[c]) for every c, Xt = X^T contiguous        the only route at the parent commit
Device times from the calls' own hipEvents (stats ms_total; (b) is the sum over its k calls) and the wall clock around them.
The tool refuses to go on when (a) and (b) differ in one bit.  Beside (a): GB/s on the algorithmic bytes (bytes_model below)
and how large X is (whether it can sit in the 4 MB L2 or the 256 MB Infinity Cache).  torch.sparse.mm on the same CSR is
timed with torch events for information, when this torch build has it.  --graph times graph.label_spreading and
graph.propagate_features end to end on the R-MAT --graph-scale (default 18) edge list.  Prints one JSON line per case."""
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
from tools.time_mxv import symmetric_adjacency  # noqa: E402


def spread(times, key="ms"):
    return {f"{key}_min": min(times), f"{key}_max": max(times)}


def bytes_model(M, nnz, k, V):
    """The bytes Y = A X needs: the row pointers, every column and value once, one gathered row segment of X per entry, Y
    once."""
    return 8 * (M + 1) + nnz * (4 + V) + nnz * k * V + M * k * V


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def torch_spmm(A, X, reps):
    """torch.sparse.mm of the same CSR, by torch events: (times, None) or (None, why not)."""
    try:
        dev = X.device
        T = torch.sparse_csr_tensor(torch.from_numpy(A.rowptr.copy()).to(dev), torch.from_numpy(A.colidx.astype(np.int64)).to(dev),
                                    torch.from_numpy(A.vals.copy()).to(dev), size=A.shape)
        torch.sparse.mm(T, X)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.sparse.mm(T, X)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return times, None
    except Exception as e:   # noqa: BLE001  (whatever this build says: it is reported, not hidden)
        return None, f"{type(e).__name__}: {str(e)[:200]}"


def time_shape(head, name, A, ks, reps, with_torch):
    M, N = A.shape
    V = np.dtype(A.dtype).itemsize
    tdt = torch.float32 if A.dtype == np.float32 else torch.float64
    dev = f"cuda:{A._ctx.device}"
    row = np.diff(A.rowptr)
    head = {**head, "shape": name, "M": M, "N": N, "nnz": A.nnz, "row_mean": float(row.mean()) if M else 0.0, "row_max": int(row.max()) if M else 0}
    for k in ks:
        X = torch.rand((N, k), dtype=tdt, device=dev) + 0.5
        Xt = X.t().contiguous()
        Ya, yb = torch.empty((M, k), dtype=tdt, device=dev), torch.empty((k, M), dtype=tdt, device=dev)
        torch.cuda.synchronize()
        ta, tb, wa, wb, st = [], [], [], [], None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            _, st = A.mxd(X, out=Ya)
            t1 = time.perf_counter()
            ms_b = 0.0
            for c in range(k):
                ms_b += A.mxv(Xt[c], out=yb[c])[1]["ms_total"]
            t2 = time.perf_counter()
            if rep == 0:
                if not torch.equal(bits(Ya), bits(yb.t().contiguous())):
                    sys.exit(f"{name} k={k}: mxd and the k calls of mxv differ: not timing a wrong result")
            else:
                ta.append(st["ms_total"])
                tb.append(ms_b)
                wa.append((t1 - t0) * 1e3)
                wb.append((t2 - t1) * 1e3)
        b = bytes_model(M, A.nnz, k, V)
        line = {**head, "k": k, "bytes_model": b, "x_bytes": N * k * V, "lanes_per_row": st["lanes_per_row"], "launches": st["launches"],
                "long_segments": st["long_segments"], "mxd": spread(ta), "mxd_wall": spread(wa), "gbps_at_min": b / min(ta) / 1e6,
                "k_mxv": spread(tb), "k_mxv_wall": spread(wb), "mxv_over_mxd": min(tb) / min(ta), "mxv_over_mxd_worst": min(tb) / max(ta),
                "mxv_over_mxd_wall": min(wb) / min(wa), "equal_bits": True}
        if with_torch:
            tt, why = torch_spmm(A, X, reps)
            line["torch_sparse_mm"] = spread(tt) if tt else why
        print(json.dumps(line), flush=True)
        del X, Xt, Ya, yb
        torch.cuda.empty_cache()


def frontier(dt):
    n = 1 << 21
    rng = np.random.default_rng(2)
    lengths = [1 << 20] * 16
    col = np.concatenate([np.sort(rng.choice(n, size=m, replace=False)) for m in lengths]).astype(np.uint32)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return n, (rowptr, col, (rng.random(len(col)) + 0.5).astype(dt))


def time_graph(scale, edge_factor, dt, ctx, reps):
    n, r, c, _ = gen.rmat_coo(scale, edge_factor, "g500", seed=1)
    rng = np.random.default_rng(4)
    labels = {int(v): int(i % 8) for i, v in enumerate(rng.choice(n, size=n // 100, replace=False))}
    X = rng.standard_normal((n, 64)).astype(dt)
    for name, call in (("label_spreading (8 classes, 30 iterations)", lambda: graph.label_spreading(r, c, n, labels, dtype=dt, ctx=ctx)[-1]),
                       ("propagate_features (k = 64, 2 hops)", lambda: graph.propagate_features(r, c, n, X, 2, dtype=dt, ctx=ctx)[-1])):
        call()
        wall, mxd = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            info = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            mxd.append(sum(info["ms_mxd"]))
        print(json.dumps({"dtype": np.dtype(dt).name, "scale": scale, "case": name, "nnz": info["nnz"], "end_to_end": spread(wall),
                          "of_which_mxd_device": spread(mxd), "launches": info["launches"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="18,20")
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--mm-scale", type=int, default=14)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="1,4,16,64,256")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--shapes", default="adjacency,product,frontier")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--graph-scale", type=int, default=18)
    ap.add_argument("--graph-reps", type=int, default=5)
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    ctx = S.Context(0)
    for name in args.dtypes.split(","):
        dt = np.float32 if name == "f32" else np.float64
        head = {"dtype": name, "reps": args.reps}
        shapes = args.shapes.split(",")
        if "adjacency" in shapes:
            for scale in [int(s) for s in args.scales.split(",")]:
                n, csr = symmetric_adjacency(scale, args.edge_factor, dt)
                A = ctx.merge_csr_parts(n, n, [csr])
                time_shape({**head, "scale": scale}, "adjacency", A, ks, args.reps, not args.no_torch)
                A.close()
                ctx.trim()
        if "product" in shapes:
            m, r, c, v = gen.rmat_coo(args.mm_scale, args.edge_factor, "g500", seed=1, dtype=dt)
            B = ctx.merge_csr_parts(m, m, [gen.coo_to_csr(m, r, c, v)])
            P, _ = B.mxm(B)
            B.close()
            time_shape({**head, "scale": args.mm_scale}, "product", P, ks, args.reps, not args.no_torch)
            P.close()
        if "frontier" in shapes:
            n, csr = frontier(dt)
            F = ctx.merge_csr_parts(16, n, [csr])
            time_shape(head, "frontier", F, ks, args.reps, not args.no_torch)
            F.close()
        if args.graph:
            time_graph(args.graph_scale, args.edge_factor, dt, ctx, args.graph_reps)
        ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
