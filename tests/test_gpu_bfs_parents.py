"""graph.bfs_parents on the GPU against the plain-Python trees of tests/mxm_masked_model.py: parents and levels exact, the
levels equal to graph.bfs_levels' on the undirected cases, and the per-level lists of ``info`` consistent."""
import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import mxm_masked_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _check(gctx, r, c, n, sources, directed=False, max_levels=None):
    parent, level, info = graph.bfs_parents(r, c, n, sources, directed=directed, max_levels=max_levels, ctx=gctx)
    wp, wl, deepest = model.bfs_parents(r, c, n, sources, directed, max_levels)
    assert parent.dtype == np.int64 and level.dtype == np.int32 and parent.shape == level.shape == (len(sources), n)
    assert np.array_equal(level, wl) and np.array_equal(parent, wp)
    assert info["levels"] == deepest
    lists = [info[k] for k in ("frontier_nnz", "products", "products_kept", "nnz_new", "ms_mxm")]
    assert len({len(x) for x in lists}) == 1 and deepest <= len(lists[0]) <= deepest + 1
    for d in range(len(lists[0])):
        assert info["products_kept"][d] <= info["products"][d] and info["nnz_new"][d] <= info["products_kept"][d]
        assert info["nnz_new"][d] == int((wl == d + 1).sum())
        assert info["frontier_nnz"][d] == int((wl == d).sum())
    if not directed and max_levels is None:
        lv, _, binfo = graph.bfs_levels(r, c, n, sources, ctx=gctx)
        assert np.array_equal(level, lv) and binfo["levels"] == info["levels"]
    return parent, level, info


@pytest.mark.parametrize("directed", [False, True])
def test_rmat_scale_8_from_four_sources(gctx, directed):
    n, r, c, _ = gen.rmat_coo(8, 16, "g500", seed=2)
    parent, level, info = _check(gctx, r, c, n, [0, 1, 2, 0], directed)
    assert np.array_equal(parent[0], parent[3]) and np.array_equal(level[0], level[3])     # duplicate sources: independent rows
    assert info["levels"] >= 2 and (level >= 0).sum() > 4
    # on the late levels most products land on vertices already reached
    assert sum(info["products_kept"]) < sum(info["products"])


def test_a_path_of_70_vertices_has_69_levels(gctx):
    r, c = np.arange(69), np.arange(1, 70)
    parent, level, info = _check(gctx, r, c, 70, [0])
    assert info["levels"] == 69 and info["frontier_nnz"] == [1] * 70 and level[0].tolist() == list(range(70))
    assert parent[0].tolist() == [0] + list(range(69))
    _check(gctx, r, c, 70, [35, 69])


def test_a_star_has_a_frontier_of_n_minus_one(gctx):
    n = 200
    r, c = np.zeros(n - 1, np.int64), np.arange(1, n)
    parent, level, info = _check(gctx, r, c, n, [0, 7])
    assert info["frontier_nnz"][:2] == [2, n - 1 + 1] and (parent[1, 1:] == 0).sum() == n - 2 and parent[1, 0] == 7


def test_an_isolated_source_and_two_components(gctx):
    r, c = np.array([0, 0, 1, 2, 4, 3]), np.array([1, 2, 3, 3, 5, 3])
    parent, level, info = _check(gctx, r, c, 7, [6, 0, 5])
    assert parent[0].tolist() == [-1] * 6 + [6] and level[0].tolist() == [-1] * 6 + [0]
    assert parent[1].tolist() == [0, 0, 0, 1, -1, -1, -1]
    # a graph without an edge: every source alone
    parent, level, info = graph.bfs_parents(np.zeros(0, np.int64), np.zeros(0, np.int64), 3, [2, 0], ctx=gctx)
    assert parent.tolist() == [[-1, -1, 2], [0, -1, -1]] and level.tolist() == [[-1, -1, 0], [0, -1, -1]] and info["levels"] == 0


def test_max_levels_and_bad_sources(gctx):
    n, r, c, _ = gen.rmat_coo(8, 16, "g500", seed=2)
    parent, level, info = _check(gctx, r, c, n, [0, 3], max_levels=1)
    assert info["levels"] <= 1 and level.max() <= 1 and len(info["products"]) == 1
    for bad in ([n], [-1], [0, n + 5]):
        with pytest.raises(ValueError):
            graph.bfs_parents(r, c, n, bad, ctx=gctx)
