"""The graph functions built on osp_csr_build -- graph.adjacency_matrix, laplacian, incidence_matrix, line_graph -- on the
GPU against tests/build_model.py (row pointers, columns and value bits; tests/test_build_cpu.py checks those models against
scipy and networkx), against networkx directly on the small graphs, on graphs without edges or vertices, and
adjacency_matrix against the arrays the existing helpers make on the device."""
import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import graph
from tests import build_model as model
from tests import test_build_cpu as cpu            # GRAPHS, _weights, _nx_graph only
from tests import test_gpu_apply_mask as am        # _bits, DEV only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
DTYPES = [np.float32, np.float64]
GRAPHS = dict(cpu.GRAPHS)
GRAPHS["one vertex"] = (1, np.zeros(0, np.int64), np.zeros(0, np.int64))
GRAPHS["one vertex and its loop"] = (1, np.zeros(3, np.int64), np.zeros(3, np.int64))


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _assert_same(res, want, shape, dt, what=""):
    rowptr, col, val = want
    assert res.shape == shape and res.dtype == dt and res.nnz == len(col), what
    assert np.array_equal(res.rowptr, rowptr) and np.array_equal(res.colidx, col), what
    assert res.vals.dtype == val.dtype and np.array_equal(_bits(res.vals), _bits(val)), what


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_adjacency_matrix_equals_the_model(mctx, name, dt):
    n, r, c = GRAPHS[name]
    w = cpu._weights(len(r), 41).astype(dt)
    cases = [{}, {"directed": True}, {"loops": True, "dup": "count"}, {"directed": True, "loops": True, "dup": "plus"},
             {"weights": w, "dup": "min"}, {"weights": w, "dup": "max", "directed": True}, {"weights": w, "dup": "plus"},
             {"weights": w, "dup": "last", "loops": True}]
    for kw in cases:
        A = graph.adjacency_matrix(r, c, n, dtype=dt, ctx=mctx, **kw)      # never None: an edgeless graph is an empty result
        try:
            _assert_same(A, model.adjacency_matrix(n, r, c, dtype=dt, **kw), (n, n), dt, (name, kw))
        finally:
            A.close()
    A = graph.adjacency_matrix(torch.as_tensor(r, device=DEV), torch.as_tensor(c, device=DEV), dtype=dt, ctx=mctx)   # tensors, n from the list
    try:
        n_ = int(max(r.max(), c.max())) + 1 if len(r) else 0
        _assert_same(A, model.adjacency_matrix(n_, r, c, dtype=dt), (n_, n_), dt, name)
    finally:
        A.close()
    with pytest.raises(ValueError):
        graph.adjacency_matrix([0, 5], [1, 2], 3, ctx=mctx)
    with pytest.raises(ValueError):
        graph.adjacency_matrix(r, c, n, dup="sum", ctx=mctx)


@pytest.mark.parametrize("name", ["rmat8", "rmat10"])
def test_adjacency_matrix_equals_the_existing_helpers_on_the_device(mctx, name):
    n, r, c = GRAPHS[name]
    tr, tc = torch.as_tensor(r, device=DEV), torch.as_tensor(c, device=DEV)
    _, wp, wc, wv = graph.symmetric_adjacency(tr, tc, n)
    A = graph.adjacency_matrix(tr, tc, n, ctx=mctx)
    try:
        _assert_same(A, (wp.cpu().numpy(), wc.cpu().numpy().astype(np.uint32), wv.cpu().numpy()), (n, n), np.float64, name)
    finally:
        A.close()
    w = cpu._weights(len(r), 42)
    for directed in (False, True):
        for keep in ("min", "max"):
            _, wp, wc, wv = graph.weighted_adjacency(tr, tc, n, torch.as_tensor(w, device=DEV), directed=directed, keep=keep)
            A = graph.adjacency_matrix(tr, tc, n, w, directed=directed, dup=keep, ctx=mctx)
            try:
                _assert_same(A, (wp.cpu().numpy(), wc.cpu().numpy().astype(np.uint32), wv.cpu().numpy()), (n, n), np.float64, (name, directed, keep))
            finally:
                A.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_laplacian_equals_the_model_to_the_bit(mctx, name, dt):
    """One build of the four blocks in their order: the sums' order is fixed by the list, so the bits are the model's."""
    n, r, c = GRAPHS[name]
    for w in (None, cpu._weights(len(r), 43).astype(dt), cpu._weights(len(r), 44, integer=True).astype(dt)):
        Lp = graph.laplacian(r, c, n, w, dtype=dt, ctx=mctx)
        try:
            want = model.laplacian(n, r, c, w, dt)
            _assert_same(Lp, want, (n, n), dt, name)
            if n and w is not None and len(w) and float(w[0]).is_integer():       # integer weights: rows sum to zero exactly
                S_ = sp.csr_matrix((Lp.vals.astype(np.float64), Lp.colidx.astype(np.int64), Lp.rowptr), shape=(n, n))
                assert abs(S_.sum(axis=1)).max() == 0 and abs(S_ - S_.T).sum() == 0
        finally:
            Lp.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_incidence_matrix_and_line_graph_equal_the_models(mctx, name, dt):
    n, r, c = GRAPHS[name]
    B, u, v = graph.incidence_matrix(r, c, n, dtype=dt, ctx=mctx)
    try:
        want, wu, wv = model.incidence_matrix(n, r, c, dt)
        assert u.dtype == np.int64 and np.array_equal(u, wu) and np.array_equal(v, wv)
        _assert_same(B, want, (n, len(wu)), dt, name)
    finally:
        B.close()
    Lg, u, v = graph.line_graph(r, c, n, dtype=dt, ctx=mctx)
    try:
        want, wu, wv = model.line_graph(n, r, c, dt)
        assert np.array_equal(u, wu) and np.array_equal(v, wv)
        _assert_same(Lg, want, (len(wu), len(wu)), dt, name)
        if len(wu) <= 2000:                                               # and networkx itself on the small ones
            G = cpu._nx_graph(n, r, c)
            number = {e: i for i, e in enumerate(zip(u.tolist(), v.tolist()))}
            pairs = {(number[tuple(sorted(a))], number[tuple(sorted(b))]) for a, b in nx.line_graph(G).edges()}
            rr = np.repeat(np.arange(len(wu)), np.diff(Lg.rowptr))
            assert set(zip(rr.tolist(), Lg.colidx.tolist())) == pairs | {(b, a) for a, b in pairs}
    finally:
        Lg.close()
