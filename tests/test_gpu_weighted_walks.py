"""graph.weighted_random_walks and graph.weighted_sample_neighbors on the GPU against their models in tests/scan_model.py,
which mirror the device composition with the same seed per step and hop: everything is equal exactly.  R-MAT graphs of scale
10 to 12 with small integer weights (a quarter of them zero), so that parallel edges add exactly in either dtype."""
import numpy as np
import pytest
import torch

from outerspace_amd import generators as gen
from outerspace_amd import graph
from tests import scan_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _rmat(scale, seed):
    n, r, c, _ = gen.rmat_coo(scale, 8, "g500", seed=seed)
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    w = np.random.default_rng(seed + 100).integers(0, 4, len(r)).astype(np.float64)
    return r, c, int(n), w


def _stuck(A, n):
    return np.array([not (A[2][A[0][v]:A[0][v + 1]] > 0).any() for v in range(n)])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("directed", [False, True])
def test_weighted_random_walks_equal_their_model(mctx, directed, dt):
    r, c, n, w = _rmat(10, 9)
    A = model.adjacency(r, c, n, w, directed, dt)
    stuck = _stuck(A, n)
    deg = np.diff(A[0])
    zero_only = np.flatnonzero(stuck & (deg > 0))         # neighbours, but no positive weight
    starts = np.random.default_rng(10).integers(0, n, 128)
    starts[[5, 6]] = int(np.argmax(deg))                  # two walkers on one vertex
    starts[17] = int(np.flatnonzero(deg == 0)[0])
    if len(zero_only):
        starts[18] = int(zero_only[0])
    walks = graph.weighted_random_walks(r, c, n, w, starts, 16, seed=(1 << 64) - 3, directed=directed, dtype=dt, ctx=mctx)
    assert walks.shape == (128, 17) and walks.dtype == np.int64
    assert np.array_equal(walks, model.weighted_random_walks(r, c, n, w, starts, 16, seed=(1 << 64) - 3, directed=directed, dt=dt))
    assert (walks[17, 1:] == -1).all() and walks[17, 0] == starts[17]
    assert not np.array_equal(walks[5], walks[6])
    # every step goes along an edge of positive weight
    rows = np.repeat(np.arange(n), deg)
    edge = set(zip(rows[A[2] > 0].tolist(), A[1][A[2] > 0].tolist()))
    for wk in walks:
        for a, b in zip(wk[:-1], wk[1:]):
            assert (b == -1 and (a == -1 or stuck[a])) or (int(a), int(b)) in edge


def test_on_unit_weights_a_walk_s_steps_are_neighbours(mctx):
    r, c, n, _ = _rmat(11, 3)
    rowptr, col, val = model.adjacency(r, c, n, np.ones(len(r)), False, np.float64)
    edge = set(zip(np.repeat(np.arange(n), np.diff(rowptr)).tolist(), col.tolist()))
    starts = np.arange(0, n, 16)
    walks = graph.weighted_random_walks(r, c, n, np.ones(len(r)), starts, 8, seed=4, ctx=mctx)
    assert np.array_equal(walks, model.weighted_random_walks(r, c, n, np.ones(len(r)), starts, 8, seed=4))
    moved = 0
    for wk in walks:
        for a, b in zip(wk[:-1], wk[1:]):
            assert b == -1 or (int(a), int(b)) in edge
            moved += b != -1
    assert moved > 4 * len(starts)
    assert graph.weighted_random_walks(r, c, n, np.ones(len(r)), starts, 0, ctx=mctx).tolist() == starts.reshape(-1, 1).tolist()


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("scale", [10, 12])
def test_weighted_sample_neighbors_equals_its_model(mctx, scale, directed):
    r, c, n, w = _rmat(scale, 5)
    A = model.adjacency(r, c, n, w, directed, np.float64)
    deg = np.diff(A[0])
    stuck = _stuck(A, n)
    isolated, hub = int(np.flatnonzero(deg == 0)[0]), int(np.argmax(deg))
    rng = np.random.default_rng(6)
    seeds = rng.choice(n, 62, replace=False)
    seeds = np.concatenate([seeds[seeds != isolated][:61], [hub, isolated, hub]])[-64:]   # one vertex twice, one without neighbours
    fanouts = (5, 3)
    blocks, frontiers, info = graph.weighted_sample_neighbors(r, c, n, w, seeds, fanouts, seed=77, directed=directed, ctx=mctx)
    try:
        want_blocks, want_frontiers = model.weighted_sample_neighbors(r, c, n, w, seeds, fanouts, seed=77, directed=directed)
        assert len(blocks) == 2 and len(frontiers) == 3
        for f, wf in zip(frontiers, want_frontiers):
            assert f.dtype == np.int64 and np.array_equal(f, wf)
        for h, (B, (bp, bc, bv)) in enumerate(zip(blocks, want_blocks)):
            f = frontiers[h]
            assert B.shape == (len(f), n) and B.dtype == np.float64
            assert np.array_equal(B.rowptr, bp) and np.array_equal(B.colidx, bc) and np.array_equal(B.vals, bv)
            # the multiplicities of a drawable row sum to the fanout
            sums, _ = B.reduce("rows", "plus")
            assert np.array_equal(sums, np.where(stuck[f], 0, fanouts[h]))
            assert info["nnz"][h] == len(bc) and info["rows_without"][h] == int(stuck[f].sum())
        assert info["launches"] > 0 and info["ms_total"] > 0
    finally:
        for B in blocks:
            B.close()
