"""graph.pagerank and graph.connected_components on the GPU: the ranks against networkx within the bound the stop criterion
gives (tests/test_mxv_cpu.py derives it), the iteration count against tests/mxv_model.py's, the components against scipy's
exactly and their rounds against the model's exactly."""
import functools

import numpy as np
import pytest
import torch

from outerspace_amd import graph
from tests import mxv_model as model
from tests import test_mxv_cpu as cpu   # the graphs, the bound and the references only

pytestmark = pytest.mark.gpu

ALPHA = cpu.ALPHA


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _networkx_rank(name, tol):
    n, r, c, directed = cpu.RANK_GRAPHS[name]
    return cpu._networkx_rank(n, r, c, directed, tol)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-6)])
@pytest.mark.parametrize("name", list(cpu.RANK_GRAPHS))
def test_pagerank_is_networkx_within_the_stop_criterions_bound(mctx, name, dtype, tol):
    n, r, c, directed = cpu.RANK_GRAPHS[name]
    rank, info = graph.pagerank(r, c, n, alpha=ALPHA, tol=tol, max_iter=1000, directed=directed, dtype=dtype, ctx=mctx)
    want = _networkx_rank(name, tol)
    dist = float(np.abs(rank.astype(np.float64) - want).sum())
    print(f"{name} {np.dtype(dtype)}: iterations={info['iterations']} err={info['err']:.3e} L1 distance={dist:.3e} "
          f"bound={cpu.rank_bound(n, tol):.3e}")
    assert rank.dtype == dtype and rank.shape == (n,) and info["converged"]
    assert dist <= cpu.rank_bound(n, tol)
    if dtype == np.float64:
        _, minfo = model.pagerank(n, r, c, directed, alpha=ALPHA, tol=tol, max_iter=1000)
        assert abs(info["iterations"] - minfo["iterations"]) <= 1 and info["nnz"] == minfo["nnz"]
    assert len(info["ms_mxv"]) == info["iterations"]
    if name == "edgeless":
        assert info["iterations"] == 0 and info["launches"] == 0 and np.array_equal(rank, np.full(n, 1.0 / n, dtype))
    else:
        assert info["launches"] >= info["iterations"] > 0 and info["err"] < n * tol


def test_pagerank_stops_at_max_iter(mctx):
    n, r, c, directed = cpu.RANK_GRAPHS["rmat8 directed"]
    rank, info = graph.pagerank(r, c, n, tol=1e-10, max_iter=3, directed=True, ctx=mctx)
    assert info["iterations"] == 3 and not info["converged"] and info["err"] >= n * 1e-10
    assert abs(rank.sum() - 1.0) < 1e-9


def test_pagerank_of_no_vertices(mctx):
    rank, info = graph.pagerank(np.zeros(0, np.int64), np.zeros(0, np.int64), 0, ctx=mctx)
    assert rank.shape == (0,) and info["converged"] and info["launches"] == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(cpu.COMPONENT_GRAPHS))
def test_connected_components_are_scipys(mctx, name, dtype):
    n, r, c = cpu.COMPONENT_GRAPHS[name]
    labels, info = graph.connected_components(r, c, n, dtype=dtype, ctx=mctx)
    want, ncomp = cpu._scipy_labels(n, r, c)
    _, minfo = model.connected_components(n, r, c, dtype)
    assert labels.dtype == np.int64 and np.array_equal(labels, want)
    assert (info["rounds"], info["components"]) == (minfo["rounds"], minfo["components"]) and info["components"] == ncomp
    assert len(info["ms_mxv"]) == info["rounds"] and info["launches"] >= info["rounds"]


def test_connected_components_without_edges_and_the_float32_guard(mctx):
    none = np.zeros(0, np.int64)
    labels, info = graph.connected_components(none, none, 5, ctx=mctx)
    assert labels.tolist() == [0, 1, 2, 3, 4] and info["rounds"] == 0 and info["components"] == 5 and info["launches"] == 0
    with pytest.raises(ValueError):
        graph.connected_components(none, none, (1 << 24) + 1, dtype=np.float32, ctx=mctx)
