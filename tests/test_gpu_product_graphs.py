"""The product graphs and Kronecker powers of outerspace_amd/graph.py (tensor_product, cartesian_product, strong_product,
kronecker_power) on the GPU against the dense models of tests/kron_model.py, on graphs of 5 to 12 vertices; and the
Kronecker square of a loop-free R-MAT seed by its closed forms alone: nnz, degrees, triangles."""
import networkx as nx
import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import kron_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _graph(G):
    G = nx.convert_node_labels_to_integers(G)
    e = np.array(G.edges(), np.int64).reshape(-1, 2)
    return e[:, 0], e[:, 1], G.number_of_nodes()


GRAPHS = {"path": nx.path_graph(5), "cycle": nx.cycle_graph(6), "star": nx.star_graph(6), "petersen": nx.petersen_graph(),
          "wheel": nx.wheel_graph(12), "edgeless": nx.empty_graph(5)}
PAIRS = [("path", "cycle"), ("star", "petersen"), ("wheel", "path"), ("petersen", "petersen"), ("edgeless", "cycle"), ("cycle", "edgeless")]


def _assert_same(res, want):
    assert res.shape == (len(want[0]) - 1,) * 2 and res.nnz == len(want[1])
    assert np.array_equal(res.rowptr, want[0]) and np.array_equal(res.colidx, want[1])
    assert np.array_equal(res.vals, want[2].astype(res.dtype))


@pytest.mark.parametrize("product", ["tensor_product", "cartesian_product", "strong_product"])
@pytest.mark.parametrize("pair", PAIRS)
def test_the_products_equal_their_models(mctx, pair, product):
    g, h = _graph(GRAPHS[pair[0]]), _graph(GRAPHS[pair[1]])
    for dtype in (np.float64, np.float32):
        res, info = getattr(graph, product)(g, h, dtype=dtype, ctx=mctx)
        try:
            _assert_same(res, getattr(model, product)(g, h))
            assert info["n"] == g[2] * h[2] and res.dtype == dtype
        finally:
            res.close()


@pytest.mark.parametrize("product", ["tensor_product", "cartesian_product", "strong_product"])
def test_the_directed_products_with_loops_equal_their_models(mctx, product):
    G, H = nx.gnp_random_graph(7, 0.35, seed=1, directed=True), nx.gnp_random_graph(5, 0.5, seed=2, directed=True)
    G.add_edge(2, 2)
    H.add_edge(0, 0)
    H.add_edge(3, 3)
    g, h = _graph(G), _graph(H)
    res, info = getattr(graph, product)(g, h, directed=True, ctx=mctx)
    try:
        _assert_same(res, getattr(model, product)(g, h, directed=True))   # (a loop of both factors counts twice in the union)
    finally:
        res.close()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_kronecker_power_equals_its_model(mctx, k):
    r, c, n = np.array([0, 0, 1, 2, 2, 3, 4]), np.array([0, 1, 2, 2, 0, 4, 4]), 5
    for directed in (False, True):
        for loops in (False, True):
            res, info = graph.kronecker_power(r, c, n, k, directed=directed, loops=loops, ctx=mctx)
            try:
                want = model.kronecker_power(r, c, n, k, directed, loops)
                _assert_same(res, want)
                seed = model.kronecker_power(r, c, n, 1, directed, loops)
                assert info["n"] == n ** k and info["nnz"] == len(seed[1]) ** k == res.nnz and info["nnz_seed"] == len(seed[1])
                assert len(info["ms_steps"]) == k - 1 and all(ms >= 0 for ms in info["ms_steps"])
            finally:
                res.close()
    with pytest.raises(ValueError):
        graph.kronecker_power(r, c, n, 0, ctx=mctx)


def test_the_kronecker_square_of_an_rmat_seed_by_its_closed_forms(mctx):
    n, r, c, _ = gen.rmat_coo(5, 4, "g500", seed=7)
    t_seed = graph.triangle_count(r, c, n, ctx=mctx)
    assert t_seed > 0
    res, info = graph.kronecker_power(r, c, n, 2, loops=False, ctx=mctx)
    try:
        seed = model.adjacency(r, c, n)
        deg, nnz_seed = seed.sum(1).astype(np.int64), int(seed.sum())
        assert res.shape == (n * n, n * n) and res.nnz == nnz_seed ** 2 == info["nnz"] and info["nnz_seed"] == nnz_seed
        assert np.array_equal(np.diff(res.rowptr), np.outer(deg, deg).reshape(-1))            # degrees are the outer product
        assert np.array_equal(res.reduce("rows", "count")[0].astype(np.int64), np.outer(deg, deg).reshape(-1))
        u = np.repeat(np.arange(n * n, dtype=np.int64), np.diff(res.rowptr))
        assert graph.triangle_count(u, res.colidx.astype(np.int64), n * n, ctx=mctx) == 6 * t_seed ** 2
    finally:
        res.close()
