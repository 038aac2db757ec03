#!/usr/bin/env python3
"""Times osp_csr_mxm_masked against the composition it replaces (MEASUREMENTS.md section 0w).

On the R-MAT graph at --scale it walks the levels of a --sources-source BFS the way graph.bfs_parents does, and on every
level's operands -- the frontier F, the graph A, the parents so far P -- it times

    fused      F.mxm(A, "min", "first", mask=P, complement=True)                       one call
    two calls  F.mxm(A, "min", "first")  then  .apply_mask(P, complement=True)         the two calls the fused one replaces

and, as the one case in the keeping sense, (A A)<A> under (plus, times) both ways, with ``osp_spgemm_masked`` of the same
operands as a third evaluation of that one (A's values are 1: every value is an exact count).  The baseline is ALWAYS the
two existing calls on the same operands in the same process, alternating with the fused call, never an earlier run of the
fused one.
Device times are the library's own (ms_total of each call, summed for the composition); every case runs --reps times after
one warm-up pair and reports the smallest and the largest; the first pair also compares the two results bit for bit.
Prints one JSON line per level, one for all levels and one for (A A)<A>, then the table of MEASUREMENTS.md."""
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


def both(ra, rb, rm, complement, semiring, reps):
    """(fused stats, fused times, two-call times, (product ms, mask ms) of the fastest composition, bit-identical)."""
    t_fused, t_two, parts, st, same = [], [], [], None, None
    for rep in range(reps + 1):
        fused, st = ra.mxm(rb, *semiring, mask=rm, complement=complement)
        full, s1 = ra.mxm(rb, *semiring)
        two, s2 = full.apply_mask(rm, complement=complement)
        if rep == 0:
            bits = np.uint32 if fused.dtype == np.float32 else np.uint64
            same = bool(np.array_equal(fused.rowptr, two.rowptr) and np.array_equal(fused.colidx, two.colidx) and
                        np.array_equal(fused.vals.view(bits), two.vals.view(bits)))
        else:
            t_fused.append(st["ms_total"])
            t_two.append(s1["ms_total"] + s2["ms_total"])
            parts.append((s1["ms_total"], s2["ms_total"]))
        for x in (fused, full, two):
            x.close()
    return st, t_fused, t_two, parts[t_two.index(min(t_two))], same


def record(head, st, t_fused, t_two, parts, same):
    return {**head, "products": st["products"], "products_kept": st["products_kept"], "nnz_out": st["nnz_out"], "nnz_mask": st["nnz_mask"],
            "short_rows": st["short_rows"], "long_rows": st["long_rows"], "launches": st["launches"], "fused": spread(t_fused),
            "two_calls": spread(t_two), "two_calls_product_ms": parts[0], "two_calls_mask_ms": parts[1],
            "ratio_fused_over_two_calls": min(t_fused) / min(t_two), "bit_identical": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ctx = S.Context(0)
    dev = torch.device("cuda", 0)
    head = {"scale": args.scale, "sources": args.sources, "reps": args.reps}
    n, r, c, _ = gen.rmat_coo(args.scale, args.edge_factor, "g500", seed=1)
    src = np.random.default_rng(3).choice(n, args.sources, replace=False)
    _, _, _, _, A = graph._pattern_result(r.astype(np.int64), c.astype(np.int64), n, False, np.float64, ctx)
    S_ = len(src)
    s_dev = torch.as_tensor(src, device=dev)
    rp0 = torch.arange(S_ + 1, dtype=torch.int64, device=dev)
    c0, v0 = s_dev.to(torch.int32), s_dev.to(torch.float64)
    ids = torch.arange(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    F = graph._csr_result(ctx, np.float64, S_, n, rp0, c0, v0, dev, sync=False)
    P = graph._csr_result(ctx, np.float64, S_, n, rp0, c0, v0, dev, sync=False)
    rows, d = [], 0
    while True:
        d += 1
        rec = record({**head, "case": "bfs level", "level": d, "frontier_nnz": F.nnz}, *both(F, A, P, True, ("min", "first"), args.reps))
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        Nx, _ = F.mxm(A, "min", "first", mask=P, complement=True)
        if Nx.nnz == 0:
            Nx.close()
            break
        U, _ = P.ewise(Nx, "union", "first")
        Fn, _ = Nx.apply_vectors(col_op="second", cols=ids)
        for x in (P, F, Nx):
            x.close()
        P, F = U, Fn
    tot_f, tot_t = sum(x["fused"]["ms_min"] for x in rows), sum(x["two_calls"]["ms_min"] for x in rows)
    print(json.dumps({**head, "case": "all levels", "fused_ms": tot_f, "two_calls_ms": tot_t, "ratio_fused_over_two_calls": tot_f / tot_t}),
          flush=True)
    aaa = record({**head, "case": "(A A)<A>"}, *both(A, A, A, False, ("plus", "times"), args.reps))
    # a third evaluation that shares nothing with either side: the outer-product family's masked product (unit values: counts)
    fused, _ = A.mxm(A, mask=A)
    sup = graph._support_product(ctx, A)
    aaa["fused_equals_spgemm_masked"] = bool(np.array_equal(fused.rowptr, sup.rowptr) and np.array_equal(fused.colidx, sup.colidx) and
                                             np.array_equal(fused.vals, sup.vals))
    fused.close()
    sup.close()
    print(json.dumps(aaa), flush=True)
    print("\n| case | products | kept | kept share | fused ms | product ms + mask ms = two calls ms | fused / two calls | same bits |")
    print("|---|---|---|---|---|---|---|---|")
    for x in rows + [aaa]:
        name = f"level {x['level']} (frontier {x['frontier_nnz']})" if "level" in x else x["case"]
        share = x["products_kept"] / x["products"] if x["products"] else 0.0
        print(f"| {name} | {x['products']} | {x['products_kept']} | {share:.3f} | {x['fused']['ms_min']:.3f} | "
              f"{x['two_calls_product_ms']:.3f} + {x['two_calls_mask_ms']:.3f} = {x['two_calls']['ms_min']:.3f} | "
              f"{x['ratio_fused_over_two_calls']:.2f} | {x['bit_identical']} |")
    print(f"| all levels | | | | {tot_f:.3f} | {tot_t:.3f} | {tot_f / tot_t:.2f} | |")
    torch.cuda.synchronize(dev)
    for x in (F, P, A):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
