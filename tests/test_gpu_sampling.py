"""graph.sample_neighbors, graph.knn_graph and graph.random_walks on the GPU against their models in
tests/select_k_model.py, which mirror the device composition with the same seed per hop and step: everything is equal
exactly, and ``info['launches']`` is the model's count of the k-selects' kernels.  R-MAT graphs of scale 10 to 12."""
import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import select_k_model as model
from tests import test_gpu_apply_mask as am   # _bits only

pytestmark = pytest.mark.gpu
_bits = am._bits


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _rmat(scale, seed):
    n, r, c, _ = gen.rmat_coo(scale, 8, "g500", seed=seed)
    return np.asarray(r, np.int64), np.asarray(c, np.int64), int(n)


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("scale", [10, 12])
def test_sample_neighbors_equals_its_model(mctx, scale, directed):
    r, c, n = _rmat(scale, 5)
    deg = np.diff(model.adjacency(r, c, n, directed)[0])
    isolated, hub = int(np.flatnonzero(deg == 0)[0]), int(np.argmax(deg))
    rng = np.random.default_rng(6)
    seeds = rng.choice(n, 62, replace=False)
    seeds = np.concatenate([seeds[seeds != isolated][:61], [hub, isolated, hub]])[-64:]   # one vertex twice, one without neighbours
    assert len(seeds) == 64 and (seeds == hub).sum() >= 2 and deg[hub] > 10
    fanouts = (5, 3)
    blocks, frontiers, info = graph.sample_neighbors(r, c, n, seeds, fanouts, seed=77, directed=directed, ctx=mctx)
    try:
        want_blocks, want_frontiers, want = model.sample_neighbors(r, c, n, seeds, fanouts, seed=77, directed=directed)
        assert len(blocks) == 2 and len(frontiers) == 3
        for f, wf in zip(frontiers, want_frontiers):
            assert f.dtype == np.int64 and np.array_equal(f, wf)
        for h, (B, (bp, bc)) in enumerate(zip(blocks, want_blocks)):
            assert B.shape == (len(frontiers[h]), n) and B.dtype == np.float32
            assert np.array_equal(B.rowptr, bp) and np.array_equal(B.colidx, bc) and (B.vals == 1).all()
        assert info["nnz"] == want["nnz"] and info["rows_capped"] == want["rows_capped"] and info["launches"] == want["launches"]
        # the vertex listed twice drew two samples
        twice = np.flatnonzero(seeds == hub)[:2]
        bp, bc = want_blocks[0]
        assert not np.array_equal(bc[bp[twice[0]]:bp[twice[0] + 1]], bc[bp[twice[1]]:bp[twice[1] + 1]])
    finally:
        for B in blocks:
            B.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("largest", [True, False])
def test_knn_graph_equals_its_model(mctx, largest, dt):
    r, c, n = _rmat(11, 7)
    w = np.random.default_rng(8).integers(1, 50, len(r)).astype(np.float64) / 4   # ties; exact in float32
    for symmetric in ("union", "mutual", None):
        for k in (1, 6):
            out, info = graph.knn_graph(r, c, n, w, k, largest=largest, symmetric=symmetric, dtype=dt, ctx=mctx)
            try:
                (rowptr, col, val), st = model.knn_graph(r, c, n, w, k, largest, symmetric)
                assert out.shape == (n, n) and out.dtype == dt
                assert np.array_equal(out.rowptr, rowptr) and np.array_equal(out.colidx, col)
                assert np.array_equal(_bits(out.vals), _bits(val.astype(dt)))
                assert {name: info[name] for name in st} == st
                assert info["n"] == n and info["nnz"] == len(col)
            finally:
                out.close()


@pytest.mark.parametrize("directed", [False, True])
def test_random_walks_equal_their_model(mctx, directed):
    r, c, n = _rmat(10, 9)
    deg = np.diff(model.adjacency(r, c, n, directed)[0])
    dead_end = int(np.flatnonzero(deg == 0)[0])
    starts = np.random.default_rng(10).integers(0, n, 128)
    starts[[5, 6]] = int(np.argmax(deg))     # two walkers on one vertex
    starts[17] = dead_end
    walks = graph.random_walks(r, c, n, starts, 16, seed=(1 << 64) - 3, directed=directed, ctx=mctx)
    assert walks.shape == (128, 17) and walks.dtype == np.int64
    assert np.array_equal(walks, model.random_walks(r, c, n, starts, 16, seed=(1 << 64) - 3, directed=directed))
    assert (walks[17, 1:] == -1).all() and walks[17, 0] == dead_end
    assert not np.array_equal(walks[5], walks[6])
