"""graph.personalized_pagerank on the GPU against the model of tests/ewise_model.py: the non-zero pattern exactly, the values
within a bound derived from the arithmetic (see _ppr_rtol), every row's sum against the series' closed form; with pruning on
inputs whose model values all lie clear of the threshold, so that the patterns stay exact; and the traversal's two unions
(the element-wise one and the sorting merge) against each other."""
import functools
import math

import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import bfs_model
from tests import ewise_model as model

pytestmark = pytest.mark.gpu

ALPHA = 0.85


@pytest.fixture(scope="module", autouse=True)
def _give_memory_back(_ctx_shared):
    yield
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _rmat(scale, nsrc):
    n, r, c, _ = gen.rmat_coo(scale, 16, "g500", seed=1)
    adj = bfs_model.symmetric_adjacency(r, c, n)
    deg = np.diff(adj.indptr)
    by_rank = np.argsort(-deg, kind="stable")
    isolated = np.nonzero(deg == 0)[0]
    assert len(isolated)
    # high, middling and low degrees, one of them twice, and an isolated vertex
    picks = [0, 5, 50, len(by_rank) // 3, 0, 17, 2][:nsrc - 1]
    sources = [int(by_rank[k]) for k in picks] + [int(isolated[0])]
    return n, r, c, adj, np.array(sources)


@functools.lru_cache(maxsize=None)
def _grid(w):
    n, r, c = bfs_model.grid_edges(w, w)
    return n, r, c, bfs_model.symmetric_adjacency(r, c, n), np.array([0, n - 1, (w // 2) * w + w // 2, 0])


@functools.lru_cache(maxsize=None)
def _path(n):
    r, c = np.arange(n - 1), np.arange(1, n)
    return n, r, c, bfs_model.symmetric_adjacency(r, c, n), np.array([0, n // 2])


# (graph, steps K through max_iter): tol = 1e-6 alone would take 85 steps
CASES = {"rmat8": (lambda: _rmat(8, 8), 30), "rmat10": (lambda: _rmat(10, 5), 20), "rmat12": (lambda: _rmat(12, 3), 10),
         "grid16": (lambda: _grid(16), 30), "path50": (lambda: _path(50), 30)}


def _ppr_rtol(adj, K):
    """rtol = 4 K (d_max + 2) 2^-53, K the number of steps, d_max the largest degree.
    Both sides start from the same F_0 and multiply by the same operand values (one correctly rounded alpha / deg each).  An
    entry of a product is a sum of at most d_max non-negative terms, each one rounded multiply of the previous term's entry:
    whatever the order of summation, a step adds at most (1 + d_max - 1) 2^-53 <= (d_max + 1) 2^-53 to the first-order
    relative error, and adding the term to the running sum adds 2^-53 more: K (d_max + 2) 2^-53 after K steps, for either
    side against the exact series.  Nothing is negative, so nothing cancels.  The two sides may err in opposite directions
    (a factor 2), and a second factor 2 covers the terms of second order, which are below 1e-10 of the first here."""
    return 4.0 * K * (int(np.diff(adj.indptr).max(initial=0)) + 2) * 2.0 ** -53


def _compare(ctx, n, r, c, adj, sources, K, prune=0.0):
    got, info = graph.personalized_pagerank(r, c, n, sources, alpha=ALPHA, tol=1e-6, max_iter=K, prune=prune, ctx=ctx)
    want, winfo = model.ppr(adj, sources, alpha=ALPHA, tol=1e-6, max_iter=K, prune=prune)
    assert got.dtype == np.float64 and got.shape == want.shape == (len(sources), n)
    assert info["steps"] == winfo["steps"] == K and info["iterations"] == winfo["iterations"]
    assert info["frontier_nnz"][1:] == [f.nnz for f in winfo["frontiers"]][:-1]
    assert len(info["frontier_nnz"]) == len(info["nnz_result"]) == len(info["ms_product"]) == len(info["ms_union"]) == len(info["ms_select"]) \
        == info["iterations"]
    rtol = _ppr_rtol(adj, K)
    assert np.array_equal(got != 0, want != 0)
    nz = want != 0
    err = float(np.max(np.abs(got[nz] - want[nz]) / want[nz]))
    print(f"K {K} prune {prune:g}: rtol {rtol:.3e}, largest relative difference {err:.3e}, non-zeros {nz.sum()}")
    assert err <= rtol
    return got, info, winfo, rtol


@pytest.mark.parametrize("case", sorted(CASES))
def test_pagerank_equals_model(ctx, case):
    build, K = CASES[case]
    n, r, c, adj, sources = build()
    assert 1 <= len(sources) <= 8 and K <= 30
    got, info, _, rtol = _compare(ctx, n, r, c, adj, sources, K)
    deg = np.diff(adj.indptr)
    for i, s in enumerate(sources):
        total = math.fsum(got[i])
        if deg[s] == 0:     # an isolated source keeps 1 - alpha on itself, and nothing else
            assert got[i, s] == 1 - ALPHA and np.count_nonzero(got[i]) == 1
        else:
            want = 1.0 - ALPHA ** (K + 1)
            assert abs(total - want) <= rtol * want, (case, i, total, want)
    assert info["iterations"] == K and all(x > 0 for x in info["nnz_result"])
    assert info["nnz_result"] == sorted(info["nnz_result"]) and info["nnz_result"][-1] == np.count_nonzero(got)
    assert all(ms == 0.0 for ms in info["ms_select"])
    # duplicate sources are independent rows with the same answer
    dup = [i for i, s in enumerate(sources) if list(sources).count(s) > 1]
    if dup:
        assert np.array_equal(got[dup[0]], got[dup[-1]])


# (graph, K, prune): the thresholds were chosen on the CPU model; the test checks first that they still lie clear
PRUNED = {"rmat8": (lambda: _rmat(8, 8), 30, 1e-4), "rmat10": (lambda: _rmat(10, 5), 20, 1e-5), "grid16": (lambda: _grid(16), 30, 2e-4),
          "path50": (lambda: _path(50), 30, 3e-3)}


@pytest.mark.parametrize("case", sorted(PRUNED))
def test_pagerank_with_pruning(ctx, case):
    build, K, prune = PRUNED[case]
    n, r, c, adj, sources = build()
    _, winfo = model.ppr(adj, sources, alpha=ALPHA, tol=1e-6, max_iter=K, prune=prune)
    # the input condition: no entry of any product of the model lies within 10^3 rtol of the threshold, so the GPU's entries,
    # within rtol of them, fall on the same side of it
    rtol = _ppr_rtol(adj, K)
    vals = np.concatenate([p.data for p in winfo["products"]])
    gap = float(np.min(np.abs(vals - prune) / prune))
    removed = sum(p.nnz - f.nnz for p, f in zip(winfo["products"], winfo["frontiers"]))
    print(f"{case}: prune {prune:g}, nearest product entry {gap:.3e} away (relative), needed {1e3 * rtol:.3e}, removed {removed} of {len(vals)}")
    assert gap > 1e3 * rtol
    assert 0 < removed < len(vals)      # the threshold cuts something, and not everything
    got, info, _, _ = _compare(ctx, n, r, c, adj, sources, K, prune)
    assert any(ms > 0.0 for ms in info["ms_select"])
    full, _ = model.ppr(adj, sources, alpha=ALPHA, tol=1e-6, max_iter=K)
    assert np.all(got <= full * (1 + rtol)) and got.sum() < full.sum()


def test_pagerank_ends_early_when_the_term_is_empty(ctx):
    n, r, c, adj, _ = _path(50)
    got, info, winfo, _ = _compare(ctx, n, r, c, adj, np.array([25]), 30, prune=0.02)
    assert info["iterations"] == winfo["iterations"] < 30 and info["ms_union"][-1] == 0.0 and winfo["frontiers"][-1].nnz == 0


def test_pagerank_without_edges_and_without_sources(ctx):
    e = np.zeros(0, np.int64)
    adj = bfs_model.symmetric_adjacency(e, e, 40)
    got, info, _, _ = _compare(ctx, 40, e, e, adj, np.array([3, 7, 3]), 30)
    assert info["iterations"] == 1 and info["frontier_nnz"] == [3] and np.count_nonzero(got) == 3
    assert got[0, 3] == got[2, 3] == got[1, 7] == 1 - ALPHA
    got, info = graph.personalized_pagerank([0, 1], [1, 2], 3, [], ctx=ctx)
    assert got.shape == (0, 3) and info["iterations"] == 0
    # max_iter = 0: the sources alone
    got, info = graph.personalized_pagerank([0, 1], [1, 2], 3, [1], max_iter=0, ctx=ctx)
    assert got.tolist() == [[0.0, 1 - ALPHA, 0.0]] and info["iterations"] == 0 and info["steps"] == 0


def test_pagerank_rejects_bad_arguments(ctx):
    for sources in ([3], [-1]):
        with pytest.raises(ValueError):
            graph.personalized_pagerank([0, 1], [1, 2], 3, sources, ctx=ctx)
    for kw in ({"alpha": 1.0}, {"alpha": 0.0}, {"tol": 0.0}):
        with pytest.raises(ValueError):
            graph.personalized_pagerank([0, 1], [1, 2], 3, [0], ctx=ctx, **kw)


def test_pagerank_converges_to_networkx(ctx):
    import networkx as nx
    n, r, c = bfs_model.grid_edges(6, 5)
    adj = bfs_model.symmetric_adjacency(r, c, n)
    got, info = graph.personalized_pagerank(r, c, n, [7], alpha=0.5, tol=1e-9, ctx=ctx)     # 29 steps
    assert info["steps"] == info["iterations"] == model.ppr_steps(0.5, 1e-9) <= 30
    ref = nx.pagerank(nx.from_scipy_sparse_array(adj), alpha=0.5, personalization={7: 1.0}, tol=1e-14, max_iter=1000, weight=None)
    want = np.array([ref[v] for v in range(n)])
    assert np.abs(got[0] - want).sum() < 2e-9      # the series' tail, 0.5^30, and nothing else of that size


# ---- the traversal's union --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [10, 12])
def test_bfs_with_either_union_returns_identical_arrays(ctx, scale):
    n, r, c, _ = gen.rmat_coo(scale, 16, "g500", seed=1)
    adjm = bfs_model.symmetric_adjacency(r, c, n)
    by_rank = np.argsort(-np.diff(adjm.indptr), kind="stable")
    sources = np.array([int(by_rank[k]) for k in (0, 5, 50, 500, 0)])
    device = torch.device("cuda", ctx.device)
    adj = graph._Adjacency(r, c, n, device)
    runs = {}
    for name, union in (("ewise", graph._device_union), ("sort", graph._sort_union)):
        level, sigma, info, _ = graph._bfs_forward(ctx, device, adj, sources, union=union)
        runs[name] = (level.cpu().numpy(), sigma.cpu().numpy(), info)
    (l1, s1, i1), (l2, s2, i2) = runs["ewise"], runs["sort"]
    assert np.array_equal(l1, l2) and np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
    for k in ("levels", "frontier_nnz", "nnz_visited", "nnz_product", "nnz_new"):
        assert i1[k] == i2[k], k
    assert i1["levels"] >= 4 and len(i1["ms_union"]) == len(i2["ms_union"]) and all(ms >= 0 for ms in i1["ms_union"])
    want_level, want_sigma, _ = bfs_model.bfs_levels(adjm, sources)
    assert np.array_equal(l1, want_level) and np.array_equal(s1, want_sigma)
    # and the public entry takes whichever is the default
    level, sigma, _ = graph.bfs_levels(r, c, n, sources, ctx=ctx)
    assert np.array_equal(level, l1) and np.array_equal(sigma, s1)
