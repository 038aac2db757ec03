"""graph.bfs_levels and graph.betweenness_centrality on the GPU against the models of tests/bfs_model.py: levels and
shortest-path counts exactly, the centrality within a bound derived from the arithmetic (see _bc_rtol)."""
import functools

import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import bfs_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _give_memory_back(_ctx_shared):
    yield
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    n, r, c, _ = gen.rmat_coo(scale, 16, "g500", seed=1)
    adj = model.symmetric_adjacency(r, c, n)
    deg = np.diff(adj.indptr)
    by_rank = np.argsort(-deg, kind="stable")
    isolated = np.nonzero(deg == 0)[0]
    assert len(isolated)
    sources = [int(by_rank[k]) for k in (0, 5, 50, 500)] + [int(isolated[0])]
    return n, r, c, adj, np.array(sources)


@functools.lru_cache(maxsize=None)
def _grid(w):
    n, r, c = model.grid_edges(w, w)
    sources = np.array([0, n - 1, (w // 2) * w + w // 2, 0])   # two corners, the centre, a corner again
    return n, r, c, model.symmetric_adjacency(r, c, n), sources


def _compare_bfs(ctx, n, r, c, adj, sources, **kw):
    level, sigma, info = graph.bfs_levels(r, c, n, sources, ctx=ctx, **kw)
    want_level, want_sigma, want = model.bfs_levels(adj, sources, **kw)
    assert level.dtype == np.int32 and sigma.dtype == np.float64 and level.shape == sigma.shape == (len(sources), n)
    assert np.array_equal(level, want_level)
    assert want_sigma.max(initial=0) < 2.0 ** 53
    assert np.array_equal(sigma.astype(np.int64), want_sigma.astype(np.int64)) and np.array_equal(sigma, want_sigma)
    assert info["levels"] == want["levels"]
    # one product per level, and one more that finds nothing new (unless max_levels cut the search short)
    k = len(want["nnz_product"])
    assert info["nnz_product"][:k] == want["nnz_product"] and info["nnz_new"][:k] == want["nnz_new"]
    assert len(info["nnz_product"]) == len(info["ms_product"]) == len(info["ms_mask"]) == len(info["ms_union"]) == len(info["frontier_nnz"])
    return level, sigma, info, want


@pytest.mark.parametrize("scale", [10, 12, 14])
def test_bfs_rmat(ctx, scale):
    n, r, c, adj, sources = _rmat(scale)
    level, sigma, info, want = _compare_bfs(ctx, n, r, c, adj, sources)
    # the test cannot pass emptily: a deep enough search, and a filter that removes a good part of every product
    assert info["levels"] >= 4
    removed = 1.0 - sum(info["nnz_new"]) / sum(info["nnz_product"])
    print(f"scale {scale}: levels {info['levels']}, removed by the complement mask {removed:.3f}, largest sigma {sigma.max():.0f}")
    assert 0.2 <= removed <= 0.8
    assert np.all(level[-1] == np.where(np.arange(n) == sources[-1], 0, -1))   # the isolated source reaches nothing
    assert info["nnz_product"][-1] > 0 and info["nnz_new"][-1] == 0


def test_bfs_grid_with_a_duplicate_source(ctx):
    n, r, c, adj, sources = _grid(24)
    level, sigma, info, _ = _compare_bfs(ctx, n, r, c, adj, sources)
    assert info["levels"] == 46 and sigma[0, n - 1] == 8233430727600.0   # C(46, 23) paths from corner to corner
    assert np.array_equal(level[0], level[3]) and np.array_equal(sigma[0], sigma[3])


def test_bfs_path_of_300_vertices(ctx):
    n = 300
    r, c = np.arange(n - 1), np.arange(1, n)
    adj = model.symmetric_adjacency(r, c, n)
    level, sigma, info, _ = _compare_bfs(ctx, n, r, c, adj, np.array([0]))
    assert np.array_equal(level[0], np.arange(n)) and np.all(sigma == 1.0) and info["levels"] == 299
    assert len(info["nnz_product"]) == 300


def test_bfs_without_edges_and_max_levels(ctx):
    n = 50
    e = np.zeros(0, np.int64)
    adj = model.symmetric_adjacency(e, e, n)
    level, sigma, info, _ = _compare_bfs(ctx, n, e, e, adj, np.array([3, 7]))
    assert info["levels"] == 0 and info["nnz_product"] == [0] and (level >= 0).sum() == 2
    n, r, c, adj, sources = _grid(24)
    _, _, info, _ = _compare_bfs(ctx, n, r, c, adj, sources, max_levels=5)
    assert info["levels"] == 5 and len(info["nnz_product"]) == 5


def test_bfs_rejects_bad_sources(ctx):
    with pytest.raises(ValueError):
        graph.bfs_levels([0, 1], [1, 2], 3, [3], ctx=ctx)
    with pytest.raises(ValueError):
        graph.bfs_levels([0, 1], [1, 2], 3, [-1], ctx=ctx)


def _bc_rtol(adj, sources):
    """rtol = 2 (D + 1) (d_max + 4 + s) 2^-53, D the deepest level, d_max the largest degree, s the number of sources.
    sigma is exact.  Every delta is a sum of at most d_max non-negative terms, each a correctly rounded add, divide and
    multiply of values whose relative error is the next level's, so the first-order relative error grows by at most
    (d_max + 3) 2^-53 per level, and the final sum over the sources adds s 2^-53.  No term is negative, so nothing cancels;
    the factor 2 covers the second order."""
    level, _, _ = model.bfs_levels(adj, sources)
    D, d_max, s = int(level.max()), int(np.diff(adj.indptr).max()), len(sources)
    return 2.0 * (D + 1) * (d_max + 4 + s) * 2.0 ** -53


_BC_CASES = {"rmat10": lambda: _rmat(10), "rmat12": lambda: _rmat(12), "grid16": lambda: _grid(16), "grid24": lambda: _grid(24)}


@pytest.mark.parametrize("batch", [2, 64])
@pytest.mark.parametrize("case", sorted(_BC_CASES))
def test_betweenness_equals_brandes(ctx, case, batch):
    n, r, c, adj, sources = _BC_CASES[case]()
    want = model.brandes(adj, sources)
    got = graph.betweenness_centrality(r, c, n, sources, batch=batch, ctx=ctx)
    assert got.dtype == np.float64 and got.shape == (n,)
    rtol = _bc_rtol(adj, sources)
    nz = want != 0
    assert nz.sum() > n // 8
    err = np.max(np.abs(got[nz] - want[nz]) / want[nz])
    print(f"{case} batch {batch}: rtol {rtol:.3e}, largest relative difference {err:.3e}, non-zeros {nz.sum()}")
    assert np.array_equal(got == 0, want == 0)
    assert err <= rtol


def test_betweenness_of_all_sources_is_twice_networkx(ctx):
    import networkx as nx
    n, r, c = model.grid_edges(8, 8)
    adj = model.symmetric_adjacency(r, c, n)
    got = graph.betweenness_centrality(r, c, n, ctx=ctx, batch=24)
    ref = nx.betweenness_centrality(nx.from_scipy_sparse_array(adj), normalized=False)
    want = 2.0 * np.array([ref[v] for v in range(n)])
    assert np.allclose(got, want, rtol=_bc_rtol(adj, np.arange(n)), atol=0)
