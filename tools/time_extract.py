#!/usr/bin/env python3
"""Times osp_csr_extract (MEASUREMENTS.md section 0o).  One process; run it under one `timeout`.

On the symmetric adjacency of generators.rmat_coo at --scale (default 20, edge factor 16, seed 1) as a result, --dtype f64:
  (a) extract(I, I) for an ascending random half I of the vertices, against select_vertices with the same keep vectors:
      both read the same entries, extract renumbers them as well
  (b) a row gather extract(R, None) of 2^16 random rows with duplicates: GB/s on its algorithmic bytes (bytes_rows below)
      against the measured stream-copy rate (osp_stream_copy_probe)
  (c) the composed path, permute(p) for a random permutation p, against (a)'s direct path
  (d) (a) again with OSP_EXTRACT_DENSE_MAP=1: a 4-byte-per-column map in place of the bitmap and its ranks
Device times from the calls' own hipEvents (stats ms_total), one warm-up call, smallest - largest of --reps.  The arrays of
(a) are compared with select_vertices' renumbered on the host, (d)'s with (a)'s.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from outerspace_amd import generators as gen  # noqa: E402
from outerspace_amd import graph  # noqa: E402
from outerspace_amd import spgemm as S  # noqa: E402


def spread(times):
    return {"ms_min": min(times), "ms_max": max(times)}


def bytes_rows(n_rows, nnz, V):
    """HBM bytes a row gather cannot avoid: per listed row its index, two row pointers of `in`, its length written and read,
    its gathered pointer (written as out's row pointer, read back by the write pass); per entry column and value in and out."""
    return n_rows * (4 + 16 + 4 + 4 + 8 + 8) + nnz * 2 * (4 + V)


def timed(reps, call):
    """call() -> (result, stats); the first call warms up and its result is returned open, the others are closed."""
    first, times, st = None, [], None
    for rep in range(reps + 1):
        res, st = call()
        if rep == 0:
            first = res
        else:
            times.append(st["ms_total"])
            res.close()
    return first, st, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1 << 16, help="rows of the row gather (b)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dt = np.float32 if args.dtype == "f32" else np.float64
    V = np.dtype(dt).itemsize
    ctx = S.Context(0)
    dev = torch.device("cuda", ctx.device)
    gbps = ctx.stream_copy_gbps()
    head = {"scale": args.scale, "dtype": args.dtype, "reps": args.reps, "copy_gbps": gbps}
    n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
    n, rowptr, colidx, vals = graph.symmetric_adjacency(r.astype(np.int64), c.astype(np.int64), n, dev)
    vals = vals.to(torch.float32 if dt == np.float32 else torch.float64)
    cols32 = colidx.to(torch.int32)
    torch.cuda.synchronize(dev)
    A = ctx.merge_csr_parts_device(dt, n, n, [(rowptr.data_ptr(), cols32.data_ptr(), vals.data_ptr())])
    print(json.dumps({**head, "case": "symmetric adjacency", "n": n, "nnz": A.nnz}), flush=True)
    rng = np.random.default_rng(3)

    # (a) an ascending random half on both sides against select_vertices
    keep = rng.random(n) < 0.5
    I = np.flatnonzero(keep)
    ti = torch.from_numpy(I.astype(np.int32)).to(dev)
    k8 = torch.from_numpy(keep.astype(np.uint8)).to(dev)
    torch.cuda.synchronize(dev)
    sel, sst, t_sel = timed(args.reps, lambda: A.select_vertices(k8, k8))
    ext, est, t_ext = timed(args.reps, lambda: A.extract(ti, ti))
    rank = np.cumsum(keep) - 1
    ok = bool(np.array_equal(ext.rowptr, np.concatenate([[0], np.cumsum(np.diff(sel.rowptr)[I])]))
              and np.array_equal(ext.colidx, rank[sel.colidx]) and np.array_equal(ext.vals.view(np.uint64 if V == 8 else np.uint32),
                                                                                    sel.vals.view(np.uint64 if V == 8 else np.uint32)))
    print(json.dumps({**head, "case": "(a) select_vertices, half the vertices on both sides", "nnz_out": sst["nnz_out"],
                      "launches": sst["launches"], **spread(t_sel)}), flush=True)
    print(json.dumps({**head, "case": "(a) extract, the same half, ascending, both sides", "nnz_gathered": est["nnz_gathered"],
                      "nnz_out": est["nnz_out"], "launches": est["launches"], "readbacks": est["readbacks"], **spread(t_ext),
                      "equals_select_vertices_renumbered": ok, "extract_over_select_vertices": min(t_ext) / min(t_sel)}), flush=True)
    sel.close()

    # (d) the dense 4-byte map in place of the bitmap and its ranks
    os.environ["OSP_EXTRACT_DENSE_MAP"] = "1"
    dense, dst, t_dense = timed(args.reps, lambda: A.extract(ti, ti))
    del os.environ["OSP_EXTRACT_DENSE_MAP"]
    same = bool(np.array_equal(dense.rowptr, ext.rowptr) and np.array_equal(dense.colidx, ext.colidx))
    print(json.dumps({**head, "case": "(d) extract with OSP_EXTRACT_DENSE_MAP=1", "launches": dst["launches"], **spread(t_dense),
                      "equals_bitmap_variant": same, "dense_over_bitmap": min(t_dense) / min(t_ext),
                      "map_bytes_bitmap": (n + 63) // 64 * 12, "map_bytes_dense": 4 * n}), flush=True)
    dense.close()
    ext.close()

    # (b) a row gather with duplicates
    R = rng.integers(0, n, args.rows)
    tr = torch.from_numpy(R.astype(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    got, gst, t_rows = timed(args.reps, lambda: A.extract(tr, None))
    b = bytes_rows(len(R), gst["nnz_out"], V)
    print(json.dumps({**head, "case": "(b) row gather with duplicates", "rows": len(R), "nnz_out": gst["nnz_out"], "launches": gst["launches"],
                      "readbacks": gst["readbacks"], **spread(t_rows), "bytes_model": b, "gbps": b / min(t_rows) / 1e6,
                      "copy_rate_share": b / min(t_rows) / 1e6 / gbps}), flush=True)
    got.close()

    # (c) the composed path on a random permutation
    p = rng.permutation(n)
    tp = torch.from_numpy(p.astype(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    perm, pst, t_perm = timed(args.reps, lambda: A.permute(tp))
    assert pst["composed"] and perm.nnz == A.nnz
    print(json.dumps({**head, "case": "(c) composed path, a random permutation (device time of its four calls)", "nnz_out": perm.nnz,
                      "launches": pst["launches"], **spread(t_perm), "composed_over_direct_a": min(t_perm) / min(t_ext),
                      "ms_per_million_entries_composed": min(t_perm) / (perm.nnz / 1e6),
                      "ms_per_million_entries_direct_a": min(t_ext) / (est["nnz_gathered"] / 1e6)}), flush=True)
    perm.close()
    A.close()
    ctx.close()


if __name__ == "__main__":
    main()
