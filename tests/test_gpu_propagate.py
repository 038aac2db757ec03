"""graph.label_spreading and graph.propagate_features on the GPU, on tests/test_mxd_cpu.py's graphs in both dtypes, against
the float64 scipy evaluation (tests/mxd_model.py's references) within bounds that come from the arithmetic, and against
networkx's predictions wherever the reference's margin exceeds twice that bound.

Measured on an MI355X (the largest ratio distance / bound over all cases): label_spreading 0.0018 (float32) and 0.0016
(float64); propagate_features 0.026 (float32) and 0.022 (float64).  DESIGN.md section 21 has the table."""
import networkx as nx
import numpy as np
import pytest
from networkx.algorithms import node_classification

from outerspace_amd import graph
from tests import mxd_model as model

pytestmark = pytest.mark.gpu

GRAPHS = model.propagate_graphs()
DTYPES = [np.float32, np.float64]
ALPHA, MAX_ITER = 0.99, 30


def _networkx_predictions(n, rows, cols, labels):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(rows, cols) if a != b)
    for v, cls in labels.items():
        G.nodes[v]["label"] = cls
    return node_classification.local_and_global_consistency(G, alpha=ALPHA, max_iter=MAX_ITER)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nclasses", [2, 3, 5])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_label_spreading(_ctx_shared, name, nclasses, dt):
    n, r, c = GRAPHS[name]
    labels = model.labellings(name, n, nclasses)
    F, predicted, info = graph.label_spreading(r, c, n, labels, alpha=ALPHA, max_iter=MAX_ITER, dtype=dt, ctx=_ctx_shared)
    ref, maxdeg = model.reference_label_spreading(n, r, c, labels, ALPHA, MAX_ITER)
    bound = model.label_bound(MAX_ITER, maxdeg, dt)
    assert F.dtype == dt and F.shape == ref.shape and len(predicted) == n
    assert (info["iterations"], info["max_degree"], info["classes"]) == (MAX_ITER, maxdeg, list(range(nclasses)))
    assert len(info["ms_mxd"]) == MAX_ITER and info["launches"] >= MAX_ITER
    # every term is non-negative: an entry that is 0 in exact arithmetic is 0 here, every other one is close RELATIVELY
    assert not (F[ref == 0] != 0).any() and (F >= 0).all()
    rel = np.abs(F.astype(np.float64) - ref)[ref > 0] / ref[ref > 0]
    print(f"{name} classes={nclasses} {np.dtype(dt).name}: max relative distance {rel.max():.3e}, bound {bound:.3e}, ratio {rel.max() / bound:.4f}")
    assert rel.max() <= bound
    decided = model.margins(ref) > 2 * bound
    want = _networkx_predictions(n, r, c, labels)
    assert decided.sum() >= 0.9 * (ref.max(axis=1) > 0).sum()
    assert [p for p, d in zip(predicted, decided) if d] == [w for w, d in zip(want, decided) if d]
    # the model follows the same steps: its predictions on the decided vertices are these too
    assert [p for p, d in zip(model.label_spreading(n, r, c, labels, ALPHA, MAX_ITER, dt)[1], decided) if d] == [p for p, d in zip(predicted, decided) if d]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_propagate_features(_ctx_shared, name, self_loops, dt):
    n, r, c = GRAPHS[name]
    X = np.random.default_rng(3).standard_normal((n, 5)).astype(dt)
    for hops in (1, 2, 3):
        got, info = graph.propagate_features(r, c, n, X, hops, self_loops=self_loops, dtype=dt, ctx=_ctx_shared)
        want, scale, maxdeg = model.reference_propagate(n, r, c, X, hops, self_loops)
        bound = model.propagate_bound(hops, maxdeg, dt)
        assert got.dtype == dt and got.shape == want.shape
        assert (info["hops"], info["max_degree"], len(info["ms_mxd"])) == (hops, maxdeg, hops)
        dist = np.abs(got.astype(np.float64) - want)
        ratio = float((dist[scale > 0] / (bound * scale[scale > 0])).max())
        print(f"{name} self_loops={self_loops} hops={hops} {np.dtype(dt).name}: largest distance / bound {ratio:.4f}")
        assert (dist <= bound * scale).all()
    zero, info = graph.propagate_features(r, c, n, X, 0, self_loops=self_loops, dtype=dt, ctx=_ctx_shared)
    assert np.array_equal(zero, X) and info["launches"] == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_and_edgeless_graphs(_ctx_shared, dt):
    none = np.zeros(0, np.int64)
    F, predicted, info = graph.label_spreading(none, none, 5, {1: 0, 3: 1}, alpha=ALPHA, max_iter=MAX_ITER, dtype=dt, ctx=_ctx_shared)
    wantF, want_pred, _ = model.label_spreading(5, none, none, {1: 0, 3: 1}, ALPHA, MAX_ITER, dt)
    assert F.dtype == dt and np.array_equal(F, wantF) and predicted == want_pred == [0, 0, 0, 1, 0]
    assert info["launches"] == 0 and info["nnz"] == 0 and info["iterations"] == MAX_ITER
    # the per-vertex form of labels: a negative id is "unlabelled"
    F2, predicted2, _ = graph.label_spreading(none, none, 5, [-1, 0, -1, 1, -1], alpha=ALPHA, max_iter=MAX_ITER, dtype=dt, ctx=_ctx_shared)
    assert np.array_equal(F2, F) and predicted2 == predicted
    X = np.arange(10.0).reshape(5, 2).astype(dt)
    got, info = graph.propagate_features(none, none, 5, X, 2, dtype=dt, ctx=_ctx_shared)
    assert got.dtype == dt and np.array_equal(got, X) and info["nnz"] == 5 and info["max_degree"] == 1   # A^ is the identity
    got, info = graph.propagate_features(none, none, 5, X, 2, self_loops=False, dtype=dt, ctx=_ctx_shared)
    assert np.array_equal(got, 0 * X) and info["launches"] == 0
    got, info = graph.propagate_features(none, none, 0, np.zeros((0, 3), dt), 2, dtype=dt, ctx=_ctx_shared)
    assert got.shape == (0, 3) and info["launches"] == 0
    with pytest.raises(ValueError):
        graph.label_spreading(none, none, 0, {}, dtype=dt, ctx=_ctx_shared)
