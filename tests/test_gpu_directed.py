"""The graph functions that walk edges backwards, on the GPU: graph.strongly_connected against scipy's strong components,
graph.cocitation and graph.bibliographic_coupling against scipy's A^T A and A A^T without their diagonals, exactly."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import connected_components

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import transpose_model as model

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _graphs():
    g = dict(model.graphs())
    n, r, c, _ = gen.rmat_coo(10, 4, "g500", seed=12)
    g["rmat10"] = (n, r.astype(np.int64), c.astype(np.int64))
    return g


GRAPHS = _graphs()


@pytest.fixture(scope="module")
def gctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _labels(n, r, c):
    return connected_components(sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n)), directed=True, connection="strong")[1]


@pytest.mark.parametrize("count", [1, 4, 64])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_strongly_connected_is_scipys_component_of_every_source(gctx, name, count):
    n, r, c = GRAPHS[name]
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    label = _labels(n, r, c)
    # (a small graph has fewer vertices than sources: they repeat)
    sources = np.resize(np.random.default_rng(count).permutation(n), count)
    member, info = graph.strongly_connected(r, c, n, sources, ctx=gctx)
    assert member.dtype == np.bool_ and member.shape == (count, n)
    assert np.array_equal(member, label[sources][:, None] == label[None, :])
    assert member[np.arange(count), sources].all()
    want, winfo = model.strongly_connected(r, c, n, sources)
    assert np.array_equal(member, want)
    assert {k: info[k] for k in winfo} == winfo
    # W has n rows: the row-mask path up to 64 vertices, the sort beyond
    assert info["path"] == (1 if n <= 64 else 2) and info["ms_transpose"] >= 0


def test_max_iter_cuts_the_search_short(gctx):
    n, r, c = GRAPHS["cycle with a tail"]
    full, info = graph.strongly_connected(r, c, n, [0], ctx=gctx)
    assert full[0].tolist() == [True, True, True, True, False, False, False]
    assert info["rounds_forward"] > 2 and info["path"] == 1
    cut, cinfo = graph.strongly_connected(r, c, n, [0], max_iter=2, ctx=gctx)
    want, winfo = model.strongly_connected(r, c, n, [0], max_iter=2)
    assert np.array_equal(cut, want) and cinfo["rounds_forward"] == cinfo["rounds_backward"] == 2
    assert cut[0].tolist() == [True, False, True, False, False, False, False]       # 0 reaches {1, 2} in two steps, {3, 2} reach 0
    none, ninfo = graph.strongly_connected(r, c, n, [0], max_iter=0, ctx=gctx)
    assert none[0].tolist() == [True] + [False] * 6 and ninfo["rounds_forward"] == 0


def test_a_graph_without_edges(gctx):
    member, info = graph.strongly_connected(np.zeros(0, np.int64), np.zeros(0, np.int64), 5, [1, 4], ctx=gctx)
    assert member.tolist() == [[False, True, False, False, False], [False, False, False, False, True]]
    assert info["path"] == 0 and info["rounds_forward"] == 0
    loops, _ = graph.strongly_connected([0, 1], [0, 1], 3, [0, 2], ctx=gctx)          # self loops only: dropped
    assert loops.tolist() == [[True, False, False], [False, False, True]]


def _pattern(n, r, c, dt):
    A = sp.csr_matrix((np.ones(len(r), dt), (r, c)), shape=(n, n))
    A.data[:] = 1                                               # duplicates are one edge
    return A


def _offdiag(P):
    P = P.tocoo()
    keep = P.row != P.col
    out = sp.csr_matrix((P.data[keep], (P.row[keep], P.col[keep])), shape=P.shape)
    out.sort_indices()
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("scale", [8, 10])
def test_cocitation_and_coupling_are_scipys_products_without_the_diagonal(gctx, scale, dt):
    n, r, c, _ = gen.rmat_coo(scale, 8, "g500", seed=13)
    r, c = r.astype(np.int64), c.astype(np.int64)
    r, c = np.concatenate([r, r[:50], [3, 9]]), np.concatenate([c, c[:50], [3, 9]])      # duplicate edges and self loops
    A = _pattern(n, r, c, dt)
    for fn, want in ((graph.cocitation, _offdiag(A.T @ A)), (graph.bibliographic_coupling, _offdiag(A @ A.T))):
        res = fn(r, c, n, dtype=dt, ctx=gctx)
        try:
            assert res.shape == (n, n) and res.dtype == dt and res.nnz == want.nnz > 0
            assert np.array_equal(res.rowptr, want.indptr) and np.array_equal(res.colidx, want.indices)
            assert np.array_equal(res.vals, want.data.astype(dt))
        finally:
            res.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_cocitation_and_coupling_of_an_edgeless_graph(gctx, dt):
    for fn in (graph.cocitation, graph.bibliographic_coupling):
        res = fn(np.zeros(0, np.int64), np.zeros(0, np.int64), 6, dtype=dt, ctx=gctx)
        try:
            assert res.shape == (6, 6) and res.nnz == 0 and np.array_equal(res.rowptr, np.zeros(7, np.int64))
        finally:
            res.close()
