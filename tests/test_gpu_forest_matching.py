"""graph.minimum_spanning_forest and graph.greedy_matching on the GPU against tests/mxv_arg_model.py's sequential algorithms
under the same strict total orders: the forest's edge set and the matching's mates EXACTLY, ties included, in both dtypes
(the model gets the weights rounded to the dtype)."""
import functools
import math

import numpy as np
import pytest
import torch

from outerspace_amd import graph
from tests import mxv_arg_model as model

pytestmark = pytest.mark.gpu

GRAPHS = model.graphs()
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _edges(name, keep, dt):
    n, r, c, w = GRAPHS[name]
    return model.simple_edges(n, r, c, w, keep, dt)


@functools.lru_cache(maxsize=None)
def _kruskal(name, dt):
    return model.kruskal(GRAPHS[name][0], *_edges(name, "min", dt))


@functools.lru_cache(maxsize=None)
def _greedy(name, dt):
    return model.greedy_matching(GRAPHS[name][0], *_edges(name, "max", dt))


def _components(n, u, v):
    lab = list(range(n))

    def find(x):
        while lab[x] != x:
            lab[x] = lab[lab[x]]
            x = lab[x]
        return x

    for a, b in zip(u.tolist(), v.tolist()):
        lab[find(a)] = find(b)
    return sum(find(x) == x for x in range(n))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_forest_is_kruskals_edge_for_edge(mctx, name, dt):
    n, r, c, w = GRAPHS[name]
    u, v, wt, info = graph.minimum_spanning_forest(r, c, n, w, dtype=dt, ctx=mctx)
    ku, kv, kw = _kruskal(name, dt)
    print(f"{name} {np.dtype(dt)}: edges={len(u)} rounds={info['rounds']} components={info['components']} launches={info['launches']}")
    assert u.dtype == v.dtype == np.int64 and wt.dtype == dt
    assert np.array_equal(u, ku) and np.array_equal(v, kv) and np.array_equal(wt, kw)
    eu, ev, _ = _edges(name, "min", dt)
    assert info["components"] == _components(n, eu, ev) and len(u) == n - info["components"]
    assert 0 < info["rounds"] <= math.ceil(math.log2(n)) + 1 and len(info["ms_mxv_arg"]) == info["rounds"]
    assert info["launches"] >= info["rounds"]
    if name == "two components and isolated vertices":
        assert info["components"] == 6
    if name == "star of 2200 leaves plus random edges":
        assert np.diff(np.flatnonzero(np.r_[True, eu[1:] != eu[:-1], True])).max() > 2048     # a row of the long-row path


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_matching_is_the_sequential_greedy_one(mctx, name, dt):
    n, r, c, w = GRAPHS[name]
    mate, info = graph.greedy_matching(r, c, n, w, dtype=dt, ctx=mctx)
    print(f"{name} {np.dtype(dt)}: pairs={info['pairs']} rounds={info['rounds']} launches={info['launches']}")
    assert mate.dtype == np.int64 and mate.shape == (n,)
    assert np.array_equal(mate, _greedy(name, dt))
    m = np.flatnonzero(mate >= 0)
    assert np.array_equal(mate[mate[m]], m) and info["pairs"] == len(m) // 2 > 0
    eu, ev, _ = _edges(name, "max", dt)
    edges = set(zip(eu.tolist(), ev.tolist()))
    assert all((min(a, b), max(a, b)) in edges for a, b in zip(m.tolist(), mate[m].tolist()))     # every pair is an edge
    assert not ((mate[eu] < 0) & (mate[ev] < 0)).any()                                            # no edge has both ends free
    assert 0 < info["rounds"] == len(info["ms_mxv_arg"]) <= info["launches"]


@pytest.mark.parametrize("fn", [graph.minimum_spanning_forest, graph.greedy_matching])
def test_graphs_without_edges_launch_nothing(mctx, fn):
    for n, r, c in ((0, [], []), (5, [], []), (4, [1, 2], [1, 2])):     # no vertices; no edges; self loops only
        out = fn(np.array(r, np.int64), np.array(c, np.int64), n, ctx=mctx)
        info = out[-1]
        assert info["rounds"] == 0 and info["launches"] == 0 and info["ms_mxv_arg"] == []
        if fn is graph.greedy_matching:
            assert out[0].tolist() == [-1] * n and info["pairs"] == 0
        else:
            assert [len(a) for a in out[:3]] == [0, 0, 0] and info["components"] == n


def test_float32_refuses_ids_it_cannot_hold(mctx):
    for fn in (graph.minimum_spanning_forest, graph.greedy_matching):
        with pytest.raises(ValueError):
            fn(np.array([0]), np.array([1 << 24]), dtype=np.float32, ctx=mctx)     # n inferred: 2^24 + 1
