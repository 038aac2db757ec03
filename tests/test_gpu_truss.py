"""graph.edge_support, graph.k_truss and graph.truss_decomposition on the GPU against the scipy models of
tests/truss_model.py (themselves checked against networkx in tests/test_select_cpu.py): edge lists, supports, trussness and
the per-round counts, all exact."""
import functools

import numpy as np
import pytest

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import bfs_model
from tests import truss_model as model

pytestmark = pytest.mark.gpu

KS = (2, 3, 4, 8, 16)
# edges, edges of the 16-truss, rounds for k = 4 / 8 / 16, k_max, products of the decomposition
TABLE = {8: (2101, 468, (2, 5, 6), 16, 56), 10: (10502, 4281, (3, 7, 7), 28, 131), 12: (48222, 20864, (4, 7, 9), 49, 273),
         14: (212997, 99759, (4, 9, 11), None, None)}


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    n, r, c, _ = gen.rmat_coo(scale, 16, "g500", seed=1)
    return n, r, c, bfs_model.symmetric_adjacency(r, c, n)


@functools.lru_cache(maxsize=None)
def _model_truss(scale, k):
    return model.k_truss(_rmat(scale)[3], k)


def _same_truss(got, want):
    (u, v, info), (mu, mv, minfo) = got, want
    assert u.dtype == v.dtype == np.int64
    assert np.array_equal(u, mu) and np.array_equal(v, mv)
    for key in ("rounds", "nnz_graph", "nnz_support", "nnz_kept"):
        assert info[key] == minfo[key], key
    assert len(info["ms_product"]) == len(info["ms_select"]) == info["rounds"]
    assert all(t >= 0 for t in info["ms_product"] + info["ms_select"])


@pytest.mark.parametrize("scale", [10, 12, 14])
def test_k_truss_equals_model(ctx, scale):
    n, r, c, adj = _rmat(scale)
    edges, truss16, rounds, _, _ = TABLE[scale]
    assert adj.nnz // 2 == edges
    for k in KS:
        got = graph.k_truss(r, c, n, k, ctx=ctx)
        _same_truss(got, _model_truss(scale, k))
        if k == 2:
            assert len(got[0]) == edges and got[2]["rounds"] == 0
        if k == 3:
            assert got[2]["rounds"] == 1 and got[2]["nnz_kept"] == got[2]["nnz_support"]    # the stop rule: nothing removed
        if k in (4, 8, 16):
            assert got[2]["rounds"] == rounds[(4, 8, 16).index(k)]
    # so that this cannot pass emptily
    u, _, info = got
    assert info["rounds"] >= 5 and len(u) == truss16 and 0.2 * edges <= len(u) <= 0.8 * edges


def test_k_truss_f32_equals_f64(_ctx_shared):
    n, r, c, _ = _rmat(12)
    for k in (2, 4, 16):
        a = graph.k_truss(r, c, n, k, dtype=np.float32, ctx=_ctx_shared)
        _same_truss(a, _model_truss(12, k))
        b = graph.k_truss(r, c, n, k, dtype=np.float64, ctx=_ctx_shared)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["nnz_kept"] == b[2]["nnz_kept"]


@pytest.mark.parametrize("scale", [8, 10])
def test_edge_support_equals_model(ctx, scale):
    n, r, c, adj = _rmat(scale)
    mu, mv, ms = model.edge_support(adj)
    for dt in (np.float64, np.float32):
        u, v, s = graph.edge_support(r, c, n, dtype=dt, ctx=ctx)
        assert u.dtype == v.dtype == s.dtype == np.int64
        assert np.array_equal(u, mu) and np.array_equal(v, mv) and np.array_equal(s, ms)
    assert (s == 0).any() and s.max() > 16
    assert s.sum() // 3 == graph.triangle_count(r, c, n, ctx=ctx) and s.sum() % 3 == 0
    if scale == 10:
        assert s.sum() // 3 == 75692


@pytest.mark.parametrize("scale", [8, 10])
def test_truss_decomposition_equals_model(ctx, scale):
    n, r, c, adj = _rmat(scale)
    mu, mv, mt, minfo = model.truss_decomposition(adj)
    u, v, t, info = graph.truss_decomposition(r, c, n, ctx=ctx)
    assert np.array_equal(u, mu) and np.array_equal(v, mv) and np.array_equal(t, mt) and t.dtype == np.int64
    for key in ("k_max", "products", "rounds", "nnz_graph", "nnz_support", "nnz_kept"):
        assert info[key] == minfo[key], key
    assert (info["k_max"], info["products"]) == TABLE[scale][3:]
    # a level of the decomposition is the k-truss
    for k in (4, 16):
        ku, kv, _ = _model_truss(scale, k) if scale == 10 else model.k_truss(adj, k)
        assert np.array_equal(u[t >= k], ku) and np.array_equal(v[t >= k], kv)


def test_truss_decomposition_f32(_ctx_shared):
    n, r, c, adj = _rmat(8)
    want = model.truss_decomposition(adj)
    got = graph.truss_decomposition(r, c, n, dtype=np.float32, ctx=_ctx_shared)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3]["products"] == want[3]["products"]


def test_grid_has_no_triangle(ctx):
    n, r, c = bfs_model.grid_edges(24, 24)
    u, v, info = graph.k_truss(r, c, n, 3, ctx=ctx)
    assert len(u) == 0 and len(v) == 0
    assert info["rounds"] == 1 and info["nnz_graph"] == [2 * len(r)] and info["nnz_support"] == [0] and info["nnz_kept"] == [0]
    u, v, info = graph.k_truss(r, c, n, 2, ctx=ctx)
    assert len(u) == len(r) and info["rounds"] == 0
    u, v, s = graph.edge_support(r, c, n, ctx=ctx)
    assert len(u) == len(r) and not s.any()
    u, v, t, info = graph.truss_decomposition(r, c, n, ctx=ctx)
    assert len(u) == len(r) and np.all(t == 2) and info["k_max"] == 2 and info["products"] == 1


def test_clique_with_a_path(ctx):
    n, r, c = model.clique_with_path(9, 21)
    adj = bfs_model.symmetric_adjacency(r, c, n)
    cr, cc = np.triu_indices(9, 1)
    for k in (3, 9):
        got = graph.k_truss(r, c, n, k, ctx=ctx)
        _same_truss(got, model.k_truss(adj, k))
        assert np.array_equal(got[0], cr) and np.array_equal(got[1], cc)       # the 36 edges of the clique
    got = graph.k_truss(r, c, n, 10, ctx=ctx)
    _same_truss(got, model.k_truss(adj, 10))
    assert len(got[0]) == 0
    assert len(graph.k_truss(r, c, n, 2, ctx=ctx)[0]) == 36 + 21
    u, v, s = graph.edge_support(r, c, n, ctx=ctx)
    assert np.array_equal(s, np.where(v < 9, 7, 0))
    u, v, t, info = graph.truss_decomposition(r, c, n, ctx=ctx)
    assert np.array_equal(t, np.where(v < 9, 9, 2)) and info["k_max"] == 9
    assert info == dict(model.truss_decomposition(adj)[3], ms_product=info["ms_product"], ms_select=info["ms_select"])


def test_graph_without_edges(_ctx_shared):
    empty = np.zeros(0, np.int64)
    for rows, cols, n in ((empty, empty, 5), (empty, empty, 0), (np.array([1, 3]), np.array([1, 3]), 4)):    # the last: self loops only
        u, v, info = graph.k_truss(rows, cols, n, 3, ctx=_ctx_shared)
        assert len(u) == 0 and len(v) == 0 and info["rounds"] == 0 and info["nnz_graph"] == []
        assert all(len(x) == 0 for x in graph.edge_support(rows, cols, n, ctx=_ctx_shared))
        u, v, t, info = graph.truss_decomposition(rows, cols, n, ctx=_ctx_shared)
        assert len(u) == len(t) == 0 and info["k_max"] == 2 and info["products"] == 0


def test_duplicate_and_reversed_edges_and_self_loops(ctx):
    n, r, c, adj = _rmat(8)
    r, c = r.astype(np.int64), c.astype(np.int64)
    loops = np.arange(0, n, 7)
    rows = np.concatenate([r, c[::2], r[::3], loops])
    cols = np.concatenate([c, r[::2], c[::3], loops])
    perm = np.random.default_rng(3).permutation(len(rows))
    for k in (4, 16):
        _same_truss(graph.k_truss(rows[perm], cols[perm], n, k, ctx=ctx), _model_truss(8, k))
    mu, mv, ms = model.edge_support(adj)
    u, v, s = graph.edge_support(rows[perm], cols[perm], n, ctx=ctx)
    assert np.array_equal(u, mu) and np.array_equal(v, mv) and np.array_equal(s, ms)


def test_arguments(_ctx_shared):
    with pytest.raises(ValueError):
        graph.k_truss([0, 1], [1, 2], 3, k=1, ctx=_ctx_shared)
    with pytest.raises(ValueError):
        graph.k_truss([0, 5], [1, 2], 3, ctx=_ctx_shared)          # a vertex out of range
    with pytest.raises(TypeError):
        graph.k_truss([0, 1], [1, 2], 3, dtype=np.int32, ctx=_ctx_shared)
