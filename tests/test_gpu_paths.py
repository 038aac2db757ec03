"""graph.shortest_paths, graph.widest_paths and graph.min_plus_closure on the GPU: against tests/semiring_model.py round for
round (the ``info`` lists) and against scipy's Dijkstra / a plain widest-path Dijkstra for equality AS FLOATS -- the weights
are integers, so every path sum is exact."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import dijkstra

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import semiring_model as model
from tests.test_mxm_cpu import _scipy_graph, _widest_dijkstra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    n, r, c, _ = gen.rmat_coo(scale, 4, "g500", seed=scale)
    r, c = r.astype(np.int64), c.astype(np.int64)
    w = np.random.default_rng(scale).integers(1, 10, len(r)).astype(np.float64)
    for x in (r, c, w):
        x.setflags(write=False)
    return n, r, c, w


def _sources(n, count):
    return np.random.default_rng(count).choice(n, count, replace=False)


def _same_rounds(info, minfo):
    assert info["rounds"] == minfo["rounds"]
    for key in ("frontier_nnz", "nnz_product", "products"):
        assert info[key] == minfo[key], key
    assert len(info["ms_product"]) == info["rounds"] and all(ms >= 0 for ms in info["ms_product"])


@pytest.mark.parametrize("scale,nsrc", [(8, 1), (8, 4), (10, 64), (12, 4)])
def test_shortest_and_widest_paths_equal_the_model_and_dijkstra(mctx, scale, nsrc):
    n, r, c, w = _rmat(scale)
    src = _sources(n, nsrc)
    Wmin = model.weighted_adjacency(r, c, n, w)
    dist, info = graph.shortest_paths(r, c, n, src, weights=w, ctx=mctx)
    mdist, minfo = model.shortest_paths(Wmin, n, src)
    assert dist.dtype == np.float64 and dist.shape == (nsrc, n)
    assert np.array_equal(dist, mdist)
    _same_rounds(info, minfo)
    assert np.array_equal(dist, dijkstra(_scipy_graph(Wmin, n), directed=True, indices=src))
    Wmax = model.weighted_adjacency(r, c, n, w, keep="max")
    width, winfo = graph.widest_paths(r, c, n, src, weights=w, ctx=mctx)
    mwidth, mwinfo = model.widest_paths(Wmax, n, src)
    assert np.array_equal(width, mwidth)
    _same_rounds(winfo, mwinfo)
    k = min(nsrc, 4)
    assert np.array_equal(width[:k], np.stack([_widest_dijkstra(Wmax, n, int(s)) for s in src[:k]]))


def test_unit_weights_give_the_bfs_levels(mctx):
    n, r, c, _ = _rmat(10)
    src = _sources(n, 4)
    hops, info = graph.shortest_paths(r, c, n, src, ctx=mctx)
    level, _, binfo = graph.bfs_levels(r, c, n, src, ctx=mctx)
    assert np.array_equal(np.where(np.isinf(hops), -1, hops).astype(np.int32), level)
    assert info["rounds"] == binfo["levels"] + 1


def test_float32_distances(mctx):
    n, r, c, w = _rmat(8)
    dist, _ = graph.shortest_paths(r, c, n, [0, 5], weights=w, dtype=np.float32, ctx=mctx)
    assert dist.dtype == np.float32
    W = model.weighted_adjacency(r, c, n, w)
    assert np.array_equal(dist.astype(np.float64), dijkstra(_scipy_graph(W, n), directed=True, indices=[0, 5]))


def test_directed_dag(mctx):
    r, c, w = np.array([0, 0, 1, 2, 3, 1]), np.array([1, 2, 3, 3, 4, 4]), np.array([1.0, 5.0, 1.0, 1.0, 2.0, 9.0])
    dist, info = graph.shortest_paths(r, c, 6, [0, 3], weights=w, directed=True, ctx=mctx)
    assert dist.tolist() == [[0, 1, 5, 2, 4, np.inf], [np.inf, np.inf, np.inf, 0, 2, np.inf]]
    W = model.weighted_adjacency(r, c, 6, w, directed=True)
    mdist, minfo = model.shortest_paths(W, 6, [0, 3])
    assert np.array_equal(dist, mdist)
    _same_rounds(info, minfo)
    width, _ = graph.widest_paths(r, c, 6, [0], weights=w, directed=True, ctx=mctx)
    assert width.tolist() == [[np.inf, 1, 5, 1, 1, 0]]
    und, _ = graph.shortest_paths(r, c, 6, [4], weights=w, ctx=mctx)
    assert und.tolist() == [[4, 3, 3, 2, 0, np.inf]]


def test_unreachable_component_duplicates_and_loops(mctx):
    r = np.array([0, 1, 1, 3, 4, 4, 0])
    c = np.array([1, 0, 2, 4, 3, 4, 1])
    w = np.array([4.0, 2.0, 1.0, 7.0, 6.0, 1.0, 3.0])        # {0, 1} three times: 2 is kept (widest: 4); a loop at 4
    dist, info = graph.shortest_paths(r, c, 6, [0, 3, 5], weights=w, ctx=mctx)
    inf = np.inf
    assert dist.tolist() == [[0, 2, 3, inf, inf, inf], [inf, inf, inf, 0, 6, inf], [inf, inf, inf, inf, inf, 0]]
    width, _ = graph.widest_paths(r, c, 6, [0, 3, 5], weights=w, ctx=mctx)
    assert width.tolist() == [[inf, 4, 1, 0, 0, 0], [0, 0, 0, inf, 7, 0], [0, 0, 0, 0, 0, inf]]
    none, ninfo = graph.shortest_paths(np.zeros(0, np.int64), np.zeros(0, np.int64), 3, [1], ctx=mctx)
    assert none.tolist() == [[inf, 0, inf]] and ninfo["rounds"] == 0
    with pytest.raises(ValueError):
        graph.shortest_paths(r, c, 6, [6], weights=w, ctx=mctx)


def test_max_iter_cuts_the_loop(mctx):
    n = 12
    r, c = np.arange(n - 1), np.arange(1, n)
    dist, info = graph.shortest_paths(r, c, n, [0], max_iter=3, ctx=mctx)
    assert info["rounds"] == 3 and dist[0, :4].tolist() == [0, 1, 2, 3] and np.isinf(dist[0, 4:]).all()
    full, finfo = graph.shortest_paths(r, c, n, [0], ctx=mctx)
    assert full[0].tolist() == list(range(n)) and finfo["rounds"] == n
    mdist, minfo = model.shortest_paths(model.weighted_adjacency(r, c, n), n, [0], max_iter=3)
    assert np.array_equal(dist, mdist) and minfo["rounds"] == 3


def test_min_plus_closure_is_dijkstra_from_every_vertex(mctx):
    n, r, c, _ = gen.rmat_coo(7, 4, "g500", seed=7)
    r, c = r.astype(np.int64), c.astype(np.int64)
    w = np.random.default_rng(7).integers(1, 10, len(r)).astype(np.float64)
    W = model.weighted_adjacency(r, c, n, w)
    D = graph.min_plus_closure(r, c, n, weights=w, ctx=mctx)
    try:
        want = dijkstra(_scipy_graph(W, n), directed=True)
        has, got = model._csr_to_dense((D.rowptr, D.colidx, D.vals), (n, n), np.float64)
        assert np.array_equal(has, np.isfinite(want)) and np.array_equal(got[has], want[has])
        (mp, mc, mv), rounds = model.min_plus_closure(W, n)
        assert np.array_equal(D.rowptr, mp) and np.array_equal(D.colidx, mc) and np.array_equal(D.vals, mv)
        assert D.rounds == rounds <= 7
    finally:
        D.close()
    E = graph.min_plus_closure(np.zeros(0, np.int64), np.zeros(0, np.int64), 4, ctx=mctx)
    try:
        assert E.nnz == 4 and E.colidx.tolist() == [0, 1, 2, 3] and E.vals.tolist() == [0.0] * 4 and E.rounds == 0
    finally:
        E.close()
