"""graph.induced_subgraph, ego_network and largest_component on the GPU against the models of tests/extract_model.py and
against networkx, on the graphs of tests/test_extract_cpu.py and on the small shapes: a path, an edgeless graph, no vertex at
all, one vertex."""
import networkx as nx
import numpy as np
import pytest
import torch

from outerspace_amd import graph
from tests import extract_model as model
from tests import mxv_model
from tests import test_extract_cpu as cpu          # GRAPHS, _nx_graph, _nx_edges only

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int64)
PATH = (40, np.arange(39), np.arange(39) + 1)
SMALL = {"path": PATH, "edgeless": (5, NONE, NONE), "no vertex": (0, NONE, NONE), "one vertex": (1, NONE, NONE),
         "one vertex with a loop": (1, np.array([0]), np.array([0]))}
STATS = {"nnz_in", "nnz_gathered", "nnz_out", "ms_total", "launches", "readbacks", "composed", "n"}


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _same_edges(got, want, what=""):
    assert got[0].dtype == got[1].dtype == np.int64, what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(cpu.GRAPHS))
def test_induced_subgraph_is_the_model_and_networkx(mctx, name, dt):
    n, r, c = cpu.GRAPHS[name]
    G = cpu._nx_graph(n, r, c)
    rng = np.random.default_rng(31)
    lists = {"ascending half": np.sort(rng.choice(n, n // 2, replace=False)), "a third in any order": rng.permutation(n)[:n // 3],
             "all": np.arange(n), "none": NONE}
    for what, vertices in lists.items():
        u, v, info = graph.induced_subgraph(r, c, n, vertices, dtype=dt, ctx=mctx)
        _same_edges((u, v), model.induced_subgraph(n, r, c, vertices), what)
        _same_edges((u, v), cpu._nx_edges(G.subgraph(vertices.tolist()), vertices), what)
        assert set(info) == STATS and info["n"] == len(vertices), what
        assert info["composed"] == (what == "a third in any order") and (u < v).all()
        assert info["nnz_out"] == 2 * len(u)                          # the symmetric submatrix holds every edge twice
    vertices = rng.permutation(n)
    u, v, info = graph.induced_subgraph(r, c, n, vertices, directed=True, dtype=dt, ctx=mctx)
    _same_edges((u, v), model.induced_subgraph(n, r, c, vertices, directed=True), "directed")
    assert info["nnz_out"] == len(u) and (u == v).any() == bool((r == c).any())


def test_induced_subgraph_refuses_bad_vertex_lists(mctx):
    n, r, c = cpu.GRAPHS["rmat8"]
    for bad in ([1, 2, 1], [0, 0], [n], [-1, 3]):
        with pytest.raises(ValueError):
            graph.induced_subgraph(r, c, n, bad, ctx=mctx)
        with pytest.raises(ValueError):
            graph.induced_subgraph(r, c, n, bad, directed=True, ctx=mctx)
    with pytest.raises(ValueError):
        graph.induced_subgraph(NONE, NONE, 5, [1, 1], ctx=mctx)       # an edgeless graph checks its list as well
    u, v, _ = graph.induced_subgraph(r, c, n, [3, 1, 2], ctx=mctx)    # and the library still works
    _same_edges((u, v), model.induced_subgraph(n, r, c, [3, 1, 2]))


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", list(cpu.GRAPHS))
def test_ego_network_is_the_model_and_networkx(mctx, name, radius):
    n, r, c = cpu.GRAPHS[name]
    G = cpu._nx_graph(n, r, c)
    deg = np.bincount(np.concatenate([r[r != c], c[r != c]]), minlength=n)
    for center in (int(np.argmax(deg)), int(np.flatnonzero(deg == deg[deg > 0].min())[0]), int(np.flatnonzero(deg == 0)[0])):
        vertices, u, v, info = graph.ego_network(r, c, n, center, radius, ctx=mctx)
        wv, wu_, wv_ = model.ego_network(n, r, c, center, radius)
        assert vertices.dtype == np.int64 and np.array_equal(vertices, wv)
        _same_edges((u, v), (wu_, wv_), center)
        E = nx.ego_graph(G, center, radius=radius)
        assert vertices.tolist() == sorted(E.nodes())
        _same_edges((u, v), cpu._nx_edges(E, vertices), center)
        assert info["n"] == len(vertices) and info["levels"] <= radius and not info["composed"]
    vertices, u, v, info = graph.ego_network(r, c, n, 3, 0, ctx=mctx)
    assert vertices.tolist() == [3] and len(u) == 0 and info["levels"] == 0
    with pytest.raises(ValueError):
        graph.ego_network(r, c, n, 3, -1, ctx=mctx)
    with pytest.raises(ValueError):
        graph.ego_network(r, c, n, n, 1, ctx=mctx)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(cpu.GRAPHS) + ["two cliques", "isolated vertices"])
def test_largest_component_is_the_model_and_networkx(mctx, name, dt):
    n, r, c = mxv_model.component_graphs()[name]
    vertices, u, v, info = graph.largest_component(r, c, n, dtype=dt, ctx=mctx)
    wv, wu_, wv_ = model.largest_component(n, r, c)
    assert vertices.dtype == np.int64 and np.array_equal(vertices, wv)
    _same_edges((u, v), (wu_, wv_))
    G = cpu._nx_graph(n, r, c)
    comps = sorted(nx.connected_components(G), key=lambda s: (-len(s), min(s)))
    assert vertices.tolist() == sorted(comps[0])
    _same_edges((u, v), cpu._nx_edges(G.subgraph(comps[0]), vertices))
    assert info["components"] == len(comps) and info["n"] == len(vertices) and info["rounds"] >= 1
    if name == "two cliques":
        assert vertices.tolist() == list(range(6)) and len(u) == 15


@pytest.mark.parametrize("name", list(SMALL))
def test_small_shapes(mctx, name):
    n, r, c = SMALL[name]
    G = cpu._nx_graph(n, r, c)
    everything = np.arange(n)[::-1].copy()
    u, v, info = graph.induced_subgraph(r, c, n, everything, ctx=mctx)
    _same_edges((u, v), model.induced_subgraph(n, r, c, everything), name)
    _same_edges((u, v), cpu._nx_edges(G, everything), name)
    assert info["n"] == n
    u, v, _ = graph.induced_subgraph(r, c, n, NONE, ctx=mctx)
    assert len(u) == len(v) == 0
    vertices, u, v, info = graph.largest_component(r, c, n, ctx=mctx)
    wv, wu_, wv_ = model.largest_component(n, r, c)
    assert np.array_equal(vertices, wv)
    _same_edges((u, v), (wu_, wv_), name)
    if n:
        vertices, u, v, info = graph.ego_network(r, c, n, n - 1, 2, ctx=mctx)
        wv, wu_, wv_ = model.ego_network(n, r, c, n - 1, 2)
        assert np.array_equal(vertices, wv)
        _same_edges((u, v), (wu_, wv_), name)
        assert name != "path" or (vertices.tolist() == [37, 38, 39] and u.tolist() == [0, 1] and v.tolist() == [1, 2])
    if name == "one vertex with a loop":
        u, v, _ = graph.induced_subgraph(r, c, n, [0], directed=True, ctx=mctx)
        assert u.tolist() == [0] and v.tolist() == [0]
