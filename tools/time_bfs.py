#!/usr/bin/env python3
"""Times the traversals of graph.py on the R-MAT generator's graph at --scale (MEASUREMENTS.md section 0d).  Four forms:

(default)        graph.bfs_levels from --sources vertices (the highest degrees).  Per level: the device times of the product,
                 of the mask filter (osp_csr_apply_mask) and of the union, and the filter's achieved bytes per second -- the
                 bytes it must move, (nnz_in + nnz_out) (4 + value bytes) + 4 nnz_mask + the three row pointer arrays, over
                 its device time -- beside what a plain copy reaches in the same run (osp_stream_copy_probe).
--host-mask      the same search the way a user had to write it before the filter existed: every level's product and the
                 visited set copied to the host, filtered with scipy, and uploaded again; per level the host clock around
                 that round trip is printed beside the filter's device time of the default form.
--ewise-union    the union of every level by osp_csr_ewise (union, first): the default, named so that a run says which it took.
--sort-union     the union of every level by the sorting merge (merge_csr_parts_device) instead, as it was before osp_csr_ewise:
                 the ms_union column is what the two differ in.
--centrality     graph.betweenness_centrality from --sources vertices, --batch at a time: wall time.
--standalone     no graph: apply_mask on the self-product of the R-MAT matrix (--preset uniform) with the product's own
                 pattern thinned to every second entry as the mask, both senses (with --host-mask: the host round trip too).
--runs N repeats the traversal N times (one summary line each).  Prints one JSON line per level (or per case) and a summary line."""
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


def filter_bytes(nrow, nnz_in, nnz_mask, nnz_out, vbytes=8):
    """What one filter call must read and write: columns and values of `in` and `out`, the mask's columns, three row
    pointer arrays."""
    return (nnz_in + nnz_out) * (4 + vbytes) + nnz_mask * 4 + 3 * (nrow + 1) * 8


def host_mask_filter(ctx, clock):
    """The step between product and union without osp_csr_apply_mask: download, scipy, upload."""
    def run(product, visited):
        t0 = time.perf_counter()
        P, V = product.to_scipy(), visited.to_scipy()
        t1 = time.perf_counter()
        V.data[:] = 1.0
        new = (P - P.multiply(V)).tocsr()        # P's values are path counts >= 1: what lies in V's pattern cancels to 0
        new.eliminate_zeros()
        new.sort_indices()
        t2 = time.perf_counter()
        out = ctx.merge_csr_parts(P.shape[0], P.shape[1], [(new.indptr.astype(np.int64), new.indices.astype(np.uint32), new.data)])
        t3 = time.perf_counter()
        clock.append({"ms_download": (t1 - t0) * 1e3, "ms_host_filter": (t2 - t1) * 1e3, "ms_upload": (t3 - t2) * 1e3,
                      "ms_round_trip": (t3 - t0) * 1e3})
        return out, {"ms_total": (t3 - t0) * 1e3}
    return run


def top_degree_sources(n, r, c, k):
    deg = np.bincount(r, minlength=n) + np.bincount(c, minlength=n)
    return np.argsort(-deg, kind="stable")[:k].astype(np.int64)


def run_bfs(ctx, dev, args, n, rows, cols, src, copy_gbps, head):
    adj = graph._Adjacency(rows, cols, n, dev)
    clock = []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    flt = host_mask_filter(ctx, clock) if args.host_mask else graph._device_mask_filter
    union = graph._sort_union if args.sort_union else graph._device_union
    level, sigma, info, _ = graph._bfs_forward(ctx, dev, adj, src, mask_filter=flt, union=union)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    S_ = len(src)
    for d in range(len(info["nnz_product"])):
        nin, nm, nout, ms = info["nnz_product"][d], info["nnz_visited"][d], info["nnz_new"][d], info["ms_mask"][d]
        line = {"what": "host-mask" if args.host_mask else "device", "level": d + 1, "frontier_nnz": info["frontier_nnz"][d], "nnz_product": nin,
                "nnz_visited": nm, "nnz_new": nout, "ms_product": info["ms_product"][d], "ms_union": info["ms_union"][d],
                "union": "sort" if args.sort_union else "ewise"}
        if args.host_mask:
            line.update(clock[d])
        else:
            gbps = filter_bytes(S_, nin, nm, nout) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            line.update({"ms_mask": ms, "mask_GBps": gbps, "mask_over_copy": gbps / copy_gbps})
        print(json.dumps(line), flush=True)
    print(json.dumps({**head, "what": ("host-mask" if args.host_mask else "device") + " summary", "sources": S_, "levels": info["levels"],
                      "reached": int((level >= 0).sum().item()), "wall_s": wall, "union": "sort" if args.sort_union else "ewise", "copy_probe_GBps": copy_gbps,
                      "ms_product_sum": sum(info["ms_product"]), "ms_mask_sum": sum(info["ms_mask"]), "ms_union_sum": sum(info["ms_union"])}),
          flush=True)


def run_standalone(ctx, dev, args, n, r, c, v, copy_gbps, head):
    import scipy.sparse as sp
    A = sp.csc_matrix((v, (r, c)), shape=(n, n)); A.sort_indices()
    B = sp.csr_matrix((v, (c, r)), shape=(n, n)); B.sort_indices()
    prod = ctx.spgemm_csc_csr(n, n, n, A.indptr.astype(np.int64), A.indices.astype(np.uint32), A.data,
                              B.indptr.astype(np.int64), B.indices.astype(np.uint32), B.data, validate=False)
    from outerspace_amd.distributed import _as_tensor
    rp, ci, _ = prod.device_ptrs()
    rowptr = _as_tensor(rp, n + 1, "<i8", dev, torch.int64)
    col = _as_tensor(ci, prod.nnz, "<i4", dev, torch.int32)
    # every second entry of the product's pattern, by position
    m_col = col[::2].contiguous()
    m_rowptr = (rowptr + 1) // 2
    torch.cuda.synchronize(dev)
    mask = (m_rowptr.data_ptr(), m_col.data_ptr())
    for complement in (False, True):
        best = None
        for rep in range(args.reps):
            res, st = prod.apply_mask(mask, complement=complement)
            res.close()
            best = st if best is None or st["ms_total"] < best["ms_total"] else best
        gbps = filter_bytes(n, best["nnz_in"], best["nnz_mask"], best["nnz_out"]) / (best["ms_total"] * 1e-3) / 1e9
        print(json.dumps({**head, "what": "standalone", "complement": complement, **best, "GBps": gbps, "over_copy": gbps / copy_gbps, "copy_probe_GBps": copy_gbps}), flush=True)
    if args.host_mask:
        t0 = time.perf_counter()
        P = prod.to_scipy()
        t1 = time.perf_counter()
        keep = np.zeros(P.nnz, bool)
        keep[::2] = True
        rows_ = np.repeat(np.arange(n), np.diff(P.indptr))[keep]
        ptr = np.zeros(n + 1, np.int64)
        ptr[1:] = np.cumsum(np.bincount(rows_, minlength=n))
        t2 = time.perf_counter()
        out = ctx.merge_csr_parts(n, n, [(ptr, P.indices[keep].astype(np.uint32), P.data[keep])])
        t3 = time.perf_counter()
        out.close()
        print(json.dumps({**head, "what": "standalone host round trip", "ms_download": (t1 - t0) * 1e3, "ms_host_filter": (t2 - t1) * 1e3,
                          "ms_upload": (t3 - t2) * 1e3, "ms_round_trip": (t3 - t0) * 1e3}), flush=True)
    del rowptr, col
    prod.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--preset", default="g500")
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--host-mask", action="store_true")
    ap.add_argument("--sort-union", action="store_true")
    ap.add_argument("--ewise-union", action="store_true")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--centrality", action="store_true")
    ap.add_argument("--standalone", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = S.Context(0)
    n, r, c, v = gen.rmat_coo(args.scale, args.edge_factor, args.preset, seed=1)
    head = {"scale": args.scale, "edge_factor": args.edge_factor, "preset": args.preset, "n": n, "edges": len(r)}
    copy_gbps = ctx.stream_copy_gbps(args.probe_bytes, 5)
    if args.standalone:
        run_standalone(ctx, dev, args, n, r, c, v, copy_gbps, head)
        ctx.close()
        return
    rows = torch.from_numpy(r.astype(np.int64)).to(dev)
    cols = torch.from_numpy(c.astype(np.int64)).to(dev)
    src = top_degree_sources(n, r, c, args.sources)
    if args.centrality:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        bc = graph.betweenness_centrality(rows, cols, n, src, batch=args.batch, ctx=ctx)
        wall = time.perf_counter() - t0
        print(json.dumps({**head, "what": "centrality summary", "sources": len(src), "batch": args.batch, "wall_s": wall,
                          "nonzero": int((bc != 0).sum()), "largest": float(bc.max()), "copy_probe_GBps": copy_gbps}), flush=True)
    else:
        for _ in range(args.runs):
            run_bfs(ctx, dev, args, n, rows, cols, src, copy_gbps, head)
    ctx.close()


if __name__ == "__main__":
    main()
