#!/usr/bin/env python3
"""Times osp_csr_mxm (MEASUREMENTS.md section 0j).  The tuned outer-product pipeline is the yardstick: (PLUS, TIMES) by
CsrResult.mxm beside Context.spgemm_coo_device on the same operands, which both already lie in HBM.

--what self      the self-product of the R-MAT matrix at --scale (matrix x matrix)
--what frontier  every level's frontier of a --sources-source BFS on the R-MAT graph at --scale, times the graph
--what paths     graph.shortest_paths end to end (wall time around the call) with --sources sources, split into the
                 products' device time (info["ms_product"]) and the rest
--batch / --cap  set OSP_MXM_BATCH / OSP_MXM_SHORT_CAP for the run (the sweeps that chose the defaults)
Device times are the library's own (ms_total of the call); every case runs --reps times after one warm-up call and reports
the smallest and the largest.  Prints one JSON line per case."""
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


def spread(times):
    return {"ms_min": min(times), "ms_max": max(times)}


def both_products(ctx, dev, ra, rb, reps, semiring=("plus", "times")):
    """(mxm stats of the last call, mxm times, pipeline times, equal bit for bit) on two results."""
    a, b = _result_as_input(ra, dev), _result_as_input(rb, dev)
    torch.cuda.synchronize(dev)
    t_mxm, t_lib, st, same = [], [], None, None
    for rep in range(reps + 1):
        res, st = ra.mxm(rb, *semiring)
        lib = ctx.spgemm_coo_device(ra.dtype, ra.shape[0], ra.shape[1], rb.shape[1], a.nnz, (a.rows.data_ptr(), a.cols.data_ptr(), a.vals.data_ptr()),
                                    b.nnz, (b.rows.data_ptr(), b.cols.data_ptr(), b.vals.data_ptr()))
        if rep == 0 and semiring == ("plus", "times"):
            same = bool(np.array_equal(res.rowptr, lib.rowptr) and np.array_equal(res.colidx, lib.colidx) and
                        np.array_equal(res.vals.view(np.uint64), lib.vals.view(np.uint64)))
        if rep:
            t_mxm.append(st["ms_total"])
            t_lib.append(lib.info["ms_total"])
        res.close()
        lib.close()
    return st, t_mxm, t_lib, same


def line(head, name, st, t_mxm, t_lib, same):
    return json.dumps({**head, "case": name, "products": st["products"], "nnz_out": st["nnz_out"], "short_rows": st["short_rows"],
                       "long_rows": st["long_rows"], "batches": st["batches"], "launches": st["launches"],
                       "mxm": spread(t_mxm), "pipeline": spread(t_lib), "mxm_products_per_s": st["products"] / (min(t_mxm) * 1e-3) if st["products"] else 0.0,
                       "pipeline_products_per_s": st["products"] / (min(t_lib) * 1e-3) if st["products"] else 0.0,
                       "ratio_mxm_over_pipeline": min(t_mxm) / min(t_lib), "bit_identical": same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["self", "frontier", "paths"], default="self")
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--cap", type=int, default=None)
    args = ap.parse_args()
    if args.batch is not None:
        os.environ["OSP_MXM_BATCH"] = str(args.batch)
    if args.cap is not None:
        os.environ["OSP_MXM_SHORT_CAP"] = str(args.cap)
    ctx = S.Context(0)
    dev = torch.device("cuda", 0)
    head = {"what": args.what, "scale": args.scale, "reps": args.reps, "batch": args.batch, "cap": args.cap}
    n, r, c, v = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
    if args.what == "self":
        g = gen.coo_to_csr(n, r, c, v)
        ra = ctx.merge_csr_parts(n, n, [g])
        print(line(head, "rmat self-product", *both_products(ctx, dev, ra, ra, args.reps)), flush=True)
        st, t_mxm, _, _ = both_products(ctx, dev, ra, ra, args.reps, ("min", "plus"))
        print(json.dumps({**head, "case": "rmat self-product (min, plus)", "products": st["products"], "mxm": spread(t_mxm)}), flush=True)
        ra.close()
    elif args.what == "frontier":
        src = np.random.default_rng(3).choice(n, args.sources, replace=False)
        adj = graph._Adjacency(r.astype(np.int64), c.astype(np.int64), n, dev)
        W = graph._adjacency_result(ctx, adj, np.float64, dev)
        _, _, info, levels = graph._bfs_forward(ctx, dev, adj, src, keep_levels=True)
        tot_mxm = tot_lib = 0.0
        for d, (F, _) in enumerate(levels):
            st, t_mxm, t_lib, same = both_products(ctx, dev, F, W, args.reps)
            tot_mxm += min(t_mxm)
            tot_lib += min(t_lib)
            print(line({**head, "level": d, "frontier_nnz": F.nnz}, "bfs frontier x graph", st, t_mxm, t_lib, same), flush=True)
        print(json.dumps({**head, "case": "all levels", "mxm_ms": tot_mxm, "pipeline_ms": tot_lib, "ratio_mxm_over_pipeline": tot_mxm / tot_lib}), flush=True)
        torch.cuda.synchronize(dev)
        for F, _ in levels:
            F.close()
        W.close()
    else:
        src = np.random.default_rng(3).choice(n, args.sources, replace=False)
        w = np.random.default_rng(4).integers(1, 10, len(r)).astype(np.float64)
        rr, cc = torch.as_tensor(r.astype(np.int64), device=dev), torch.as_tensor(c.astype(np.int64), device=dev)
        ww = torch.as_tensor(w, device=dev)
        walls, prods, info = [], [], None
        for rep in range(args.reps + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dist, info = graph.shortest_paths(rr, cc, n, src, weights=ww, ctx=ctx)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                walls.append(wall)
                prods.append(sum(info["ms_product"]))
        print(json.dumps({**head, "case": "shortest_paths", "sources": args.sources, "rounds": info["rounds"], "products": sum(info["products"]),
                          "reached": int(np.isfinite(dist).sum()), "wall": spread(walls), "ms_product": spread(prods),
                          "ms_rest_at_min_wall": min(walls) - prods[walls.index(min(walls))]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
