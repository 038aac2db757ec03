"""spgemm.block_matrix and graph.bipartite_adjacency / disjoint_union / replace_subgraph on the GPU, on the inputs of
tests/test_assign_cpu.py, against the models of tests/assign_model.py, scipy.sparse.bmat and networkx; degenerate inputs; the
refusal of duplicate or out-of-range vertices."""
import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from networkx.algorithms import bipartite

from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import assign_model as model
from tests import extract_model
from tests import test_assign_cpu as cpu           # the inputs only
from tests import test_gpu_apply_mask as am        # _bits only

pytestmark = pytest.mark.gpu

_bits = am._bits
GRAPHS = cpu.GRAPHS


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _build(mctx, b):
    (rowptr, col, val), ncol = b
    m = len(rowptr) - 1
    res, _ = mctx.build(m, ncol, np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptr)), col, val, dup="error", dtype=val.dtype, space="host")
    return res


def _blk(m, n, seed):
    rng = np.random.default_rng(seed)
    if n == 0:
        return (np.zeros(m + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0)), 0
    return cpu._csr([int(x) for x in rng.integers(0, n + 1, m)], n, np.float64, seed), n


def _same(res, want, what=""):
    rowptr, col, val = want
    assert res.nnz == len(col), what
    assert np.array_equal(res.rowptr, rowptr) and np.array_equal(res.colidx, col), what
    assert np.array_equal(_bits(res.vals), _bits(np.asarray(val, res.dtype))), what


def test_block_matrix_is_the_model_and_scipys_bmat(mctx):
    grids = {"2x2 with None": [[None, _blk(5, 70, 1)], [_blk(8, 3, 2), None]],
             "full 2x3": [[_blk(4, 9, 3), _blk(4, 1, 4), _blk(4, 130, 5)], [_blk(70, 9, 6), _blk(70, 1, 7), _blk(70, 130, 8)]],
             "a 0-wide block": [[_blk(3, 0, 9), _blk(3, 5, 10)], [None, _blk(2, 5, 11)]],
             "1x1": [[_blk(6, 6, 12)]],
             "a 0-high block": [[_blk(0, 4, 13)], [_blk(3, 4, 14)]],
             "one long row of blocks": [[_blk(3, 2500, 15), _blk(3, 2100, 16)]]}
    for name, grid in grids.items():
        made = [[None if b is None else _build(mctx, b) for b in row] for row in grid]
        out = None
        try:
            out, st = S.block_matrix(made)
            want, shape = model.block_matrix(grid)
            assert out.shape == shape, name
            _same(out, want, name)
            ref = sp.csr_matrix(sp.bmat([[None if b is None else sp.csr_matrix((np.arange(1, len(b[0][1]) + 1, dtype=np.float64),
                                                                                 b[0][1].astype(np.int64), b[0][0]),
                                                                                shape=(len(b[0][0]) - 1, b[1])) for b in row] for row in grid], format="csr"))
            ref.sort_indices()
            assert out.shape == ref.shape and np.array_equal(out.rowptr, ref.indptr) and np.array_equal(out.colidx, ref.indices), name
            nonempty = sum(1 for row in grid for b in row if b is not None and b[1] and len(b[0][0]) > 1)
            assert st["blocks"] == nonempty and st["nnz_out"] == out.nnz and st["ms_total"] >= 0, (name, st)
            for row in made:                                         # the blocks stay valid
                for b in row:
                    assert b is None or b._h is not None
        finally:
            for row in made:
                for b in row:
                    if b is not None:
                        b.close()
            if out is not None:
                out.close()
    one = _build(mctx, _blk(2, 2, 1))
    three = _build(mctx, _blk(3, 3, 2))
    f32 = mctx.build(2, 2, [0], [1], [1.0], dtype=np.float32, space="host")[0]
    try:
        for bad in ([[None]], [[one, None], [None, None]], [[one], [three]], [], [[one, one], [one]]):      # a None row, sizes that disagree
            with pytest.raises(ValueError):
                S.block_matrix(bad)
        with pytest.raises(S.OspError):
            S.block_matrix([[one, f32]])
    finally:
        for x in (one, three, f32):
            x.close()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_bipartite_adjacency_is_networkx(mctx, name):
    n, r, c = GRAPHS[name]
    m, k = n, n // 2
    cc = c % k
    w = np.random.default_rng(13).integers(1, 9, len(r)).astype(np.float64)
    A = graph.bipartite_adjacency(r, cc, (m, k), w, ctx=mctx)
    try:
        assert A.shape == (m + k, m + k)
        _same(A, model.bipartite_adjacency(r, cc, (m, k), w), name)
        G = bipartite.from_biadjacency_matrix(sp.csr_matrix((w, (r, cc)), shape=(m, k)))
        want = {}
        for a, b, d in G.edges(data=True):
            want[(a, b)] = want[(b, a)] = d["weight"]
        u = np.repeat(np.arange(m + k), np.diff(A.rowptr))
        assert set(zip(u.tolist(), A.colidx.tolist())) == set(want)
        assert all(want[(a, b)] == v for a, b, v in zip(u.tolist(), A.colidx.tolist(), A.vals.tolist()))
    finally:
        A.close()
    for shape in ((0, 5), (5, 0), (0, 0), (3, 4)):                     # a side without vertices, a graph without edges
        E = graph.bipartite_adjacency([], [], shape, ctx=mctx)
        assert E.shape == (sum(shape), sum(shape)) and E.nnz == 0 and np.array_equal(E.rowptr, np.zeros(sum(shape) + 1, np.int64))
        E.close()
    for rows, cols in (([m], [0]), ([0], [k]), ([-1], [0])):
        with pytest.raises(ValueError):
            graph.bipartite_adjacency(rows, cols, (m, k), ctx=mctx)


def test_disjoint_union_is_networkx(mctx):
    none = np.zeros(0, np.int64)
    graphs = [GRAPHS["rmat8"], GRAPHS["rmat10"], (0, none, none), (4, none, none), GRAPHS["rmat8"]]
    A, offsets = graph.disjoint_union([(r, c, n) for n, r, c in graphs], ctx=mctx)
    try:
        want, woff = model.disjoint_union([(r, c, n) for n, r, c in graphs])
        assert np.array_equal(offsets, woff) and offsets.tolist() == [0, 256, 1280, 1280, 1284, 1540] and A.shape == (1540, 1540)
        _same(A, want)
        nxg = []
        for n, r, c in graphs:
            G = nx.Graph()
            G.add_nodes_from(range(n))
            G.add_edges_from((int(a), int(b)) for a, b in zip(r, c) if a != b)
            nxg.append(G)
        U = nx.disjoint_union_all(nxg)
        u = np.repeat(np.arange(A.shape[0]), np.diff(A.rowptr))
        assert set(zip(u.tolist(), A.colidx.tolist())) == {(a, b) for a, b in U.edges()} | {(b, a) for a, b in U.edges()}
    finally:
        A.close()
    for gs, shape in (([], (0, 0)), ([(none, none, 0)], (0, 0)), ([(none, none, 3)], (3, 3)), ([(none, none, 0), (none, none, 2)], (2, 2))):
        E, off = graph.disjoint_union(gs, ctx=mctx)
        assert E.shape == shape and E.nnz == 0 and off.tolist() == [0] + list(np.cumsum([g[2] for g in gs]))
        E.close()
    n, r, c = GRAPHS["rmat8"]
    D, off = graph.disjoint_union([(r, c, n), (r, c, n)], directed=True, ctx=mctx)
    try:
        _same(D, model.disjoint_union([(r, c, n), (r, c, n)], directed=True)[0], "directed")
    finally:
        D.close()


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_replace_subgraph_is_the_model_and_networkx(mctx, name, directed):
    n, r, c = GRAPHS[name]
    rng = np.random.default_rng(14)
    G = (nx.DiGraph if directed else nx.Graph)()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(r, c) if directed or a != b)
    edges_of = lambda H: sorted((a, b) if directed else (min(a, b), max(a, b)) for a, b in H.edges())   # noqa: E731
    none = np.zeros(0, np.int64)
    for V in (rng.permutation(n)[:n // 3], np.sort(rng.choice(n, n // 2, replace=False)), np.array([5]), none, np.arange(n)):
        k = len(V)
        sr, sc = (rng.integers(0, k, 3 * k), rng.integers(0, k, 3 * k)) if k else (none, none)
        u, v, info = graph.replace_subgraph(r, c, n, V, sr, sc, directed=directed, ctx=mctx)
        wu, wv = model.replace_subgraph(n, r, c, V, sr, sc, directed)
        assert np.array_equal(u, wu) and np.array_equal(v, wv) and info["n"] == n
        H = G.copy()
        inside = set(V.tolist())
        H.remove_edges_from([(a, b) for a, b in G.edges() if a in inside and b in inside])
        H.add_edges_from((int(V[a]), int(V[b])) for a, b in zip(sr, sc) if directed or a != b)
        assert list(zip(u.tolist(), v.tolist())) == edges_of(H)
        # the inverse of induced_subgraph, both on the device
        iu, iv, _ = graph.induced_subgraph(r, c, n, V, directed=directed, ctx=mctx)
        wiu, wiv = extract_model.induced_subgraph(n, r, c, V, directed)
        assert np.array_equal(iu, wiu) and np.array_equal(iv, wiv)
        u, v, _ = graph.replace_subgraph(r, c, n, V, iu, iv, directed=directed, ctx=mctx)
        assert list(zip(u.tolist(), v.tolist())) == edges_of(G)
    # a graph without edges, and a subgraph put into it
    u, v, info = graph.replace_subgraph(none, none, 6, [4, 1], [0], [1], directed=directed, ctx=mctx)
    assert list(zip(u.tolist(), v.tolist())) == ([(4, 1)] if directed else [(1, 4)])
    u, v, info = graph.replace_subgraph(none, none, 0, none, none, none, directed=directed, ctx=mctx)
    assert len(u) == 0 and info["n"] == 0
    for bad in ([1, 2, 1], [n], [-1]):
        with pytest.raises(ValueError):
            graph.replace_subgraph(r, c, n, bad, [0], [0], directed=directed, ctx=mctx)
