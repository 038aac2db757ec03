"""graph.core_numbers, k_core, jaccard_similarity and local_clustering on the GPU: the core numbers and cores against networkx,
the similarities and coefficients against tests/vector_model.py bit for bit and against networkx for EQUALITY (each is one
correctly rounded division of two exact integers), and the rounds against the model's, round for round."""
import functools

import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import bfs_model
from tests import vector_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _grid(side):
    i = np.arange(side * side).reshape(side, side)
    return side * side, np.concatenate([i[:, :-1].ravel(), i[:-1, :].ravel()]), np.concatenate([i[:, 1:].ravel(), i[1:, :].ravel()])


def _build(name):
    if name.startswith("rmat"):
        scale = int(name[4:])
        n, r, c, _ = gen.rmat_coo(scale, 16 if scale < 12 else 8, "g500", seed=1)
        return n, r, c
    if name == "grid16":
        return _grid(16)
    if name == "path":
        return 12, np.arange(11), np.arange(1, 12)
    if name == "k6pendant":
        return model.clique_with_pendant(6)
    if name == "edgeless":
        return 5, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if name == "isolated":   # a triangle with a tail among vertices that have no edge; duplicates and a self loop
        return 40, np.array([3, 7, 11, 11, 20, 7, 5]), np.array([7, 11, 3, 20, 21, 3, 5])
    raise KeyError(name)


GRAPHS = ["rmat8", "rmat10", "rmat12", "grid16", "path", "k6pendant", "edgeless", "isolated"]


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(n, rows, cols, adj, G): the edge list, the model's adjacency and networkx's graph, built once."""
    import networkx as nx
    n, r, c = _build(name)
    adj = bfs_model.symmetric_adjacency(r, c, n)
    return n, r, c, adj, nx.from_scipy_sparse_array(adj)


def _edges(u, v):
    return list(zip(u.tolist(), v.tolist()))


@pytest.mark.parametrize("name", GRAPHS)
def test_core_numbers_equal_networkx(mctx, name):
    import networkx as nx
    n, r, c, adj, G = _graph(name)
    core, info = graph.core_numbers(r, c, n, ctx=mctx)
    want = nx.core_number(G)
    assert core.dtype == np.int64 and core.tolist() == [want[i] for i in range(n)]
    mcore, minfo = model.core_numbers(adj)
    assert (info["rounds"], info["nnz_graph"], info["k_max"]) == (minfo["rounds"], minfo["nnz_graph"], minfo["k_max"])
    assert len(info["ms_reduce"]) == len(info["ms_select"]) == info["rounds"]
    if name == "isolated":
        assert core[[3, 7, 11]].tolist() == [2, 2, 2] and core[[20, 21]].tolist() == [1, 1] and core.sum() == 8
    if name == "grid16":
        assert core.tolist() == [2] * 256


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_core_numbers_in_both_dtypes(mctx, dtype):
    n, r, c, adj, G = _graph("rmat8")
    core, _ = graph.core_numbers(r, c, n, dtype=dtype, ctx=mctx)
    assert np.array_equal(core, model.core_numbers(adj)[0])


@pytest.mark.parametrize("name", GRAPHS)
def test_k_core_equals_networkx(mctx, name):
    import networkx as nx
    n, r, c, adj, G = _graph(name)
    k_max = model.core_numbers(adj)[1]["k_max"]
    for k in sorted({0, 1, 2, 3, k_max // 2, k_max, k_max + 1}):
        u, v, info = graph.k_core(r, c, n, k=k, ctx=mctx)
        assert _edges(u, v) == sorted(tuple(sorted(e)) for e in nx.k_core(G, k).edges()), k
        mu, mv, minfo = model.k_core(adj, k)
        assert (info["rounds"], info["nnz_graph"]) == (minfo["rounds"], minfo["nnz_graph"])
        if k > k_max:
            assert len(u) == 0
    with pytest.raises(ValueError):
        graph.k_core(r, c, n, k=-1, ctx=mctx)


@pytest.mark.parametrize("name", GRAPHS)
def test_jaccard_and_clustering_equal_model_and_networkx(mctx, name):
    import networkx as nx
    n, r, c, adj, G = _graph(name)
    u, v, jac = graph.jaccard_similarity(r, c, n, ctx=mctx)
    mu, mv, mjac = model.jaccard_similarity(adj)
    assert np.array_equal(u, mu) and np.array_equal(v, mv) and jac.dtype == np.float64
    assert np.array_equal(jac.view(np.uint64), mjac.view(np.uint64))
    want = {(a, b): p for a, b, p in nx.jaccard_coefficient(G, _edges(u, v))}
    assert jac.tolist() == [want[e] for e in _edges(u, v)]
    cc = graph.local_clustering(r, c, n, ctx=mctx)
    assert cc.dtype == np.float64 and np.array_equal(cc.view(np.uint64), model.local_clustering(adj).view(np.uint64))
    wc = nx.clustering(G)
    assert cc.tolist() == [float(wc[i]) for i in range(n)]
    if name == "k6pendant":
        assert cc.tolist() == [20 / 30] + [1.0] * 5 + [0.0] and (u[5], v[5], jac[5]) == (0, 6, 0.0)
    if name in ("grid16", "path"):
        assert not jac.any() and not cc.any()


def test_jaccard_and_clustering_in_float32(mctx):
    n, r, c, adj, G = _graph("rmat8")
    u, v, jac = graph.jaccard_similarity(r, c, n, dtype=np.float32, ctx=mctx)
    assert np.array_equal(jac, model.jaccard_similarity(adj, np.float32)[2])
    assert np.array_equal(graph.local_clustering(r, c, n, dtype=np.float32, ctx=mctx), model.local_clustering(adj))
