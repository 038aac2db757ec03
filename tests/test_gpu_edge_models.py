"""graph.edge_scores, graph.landmark_bounds and graph.factorize on the GPU against tests/sddmm_model.py, which follows them
step for step (bits where every step is the library's), and against the float64 references that share nothing with either."""
import functools

import numpy as np
import pytest
import torch

from outerspace_amd import graph
from tests import mxv_model
from tests import sddmm_model as model
from tests import test_gpu_apply_mask as am   # _bits and the device name only

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits = am._bits
DTYPES = [np.float32, np.float64]
K = 8


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _graphs():
    nk, rk, ck = model.karate()
    n8, r8, c8 = mxv_model._rmat(8, 11)
    return {"karate": (nk, rk, ck), "rmat8": (n8, r8, c8)}


@functools.lru_cache(maxsize=None)
def _embeddings(name):
    n = _graphs()[name][0]
    rng = np.random.default_rng(41)
    X, Y = rng.standard_normal((n, K)), rng.standard_normal((n, K))
    X[3] = 0.0   # a zero norm counts as 1: the cosine is 0
    return X, Y


# ---- edge_scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("name", ["karate", "rmat8"])
def test_edge_scores_equal_the_model_and_the_reference(mctx, name, directed, dt):
    n, r, c = _graphs()[name]
    X, Y = (a.astype(dt) for a in _embeddings(name))
    eps = float(np.finfo(dt).eps)
    for Yarg in (None, Y):
        # "dot" is one sddmm on the pattern: the model's bits
        u, v, score, info = graph.edge_scores(r, c, n, X, Yarg, "dot", directed, dtype=dt, ctx=mctx)
        mu, mv, want = model.edge_scores(n, r, c, X, Yarg, "dot", directed, dt)
        assert np.array_equal(u, mu) and np.array_equal(v, mv) and score.dtype == dt
        assert np.array_equal(_bits(score), _bits(want))
        assert info["nnz"] == len(u) > 0 and info["k"] == K and info["launches"] == 1
        ru, rv, ref, scale = model.reference_edge_scores(n, r, c, X, Yarg, "dot", directed)
        assert np.array_equal(u, ru) and np.array_equal(v, rv)
        assert (np.abs(score.astype(np.float64) - ref) <= (K + 4) * eps * scale).all()
        # "cosine": (k + 4) eps relative to ||x|| ||y||, that is absolute on the quotient
        u, v, cos, info = graph.edge_scores(r, c, n, X, Yarg, "cosine", directed, dtype=dt, ctx=mctx)
        _, _, ref, scale = model.reference_edge_scores(n, r, c, X, Yarg, "cosine", directed)
        err = np.abs(cos.astype(np.float64) - ref)
        print(f"{name} directed={directed} {np.dtype(dt).name} Y={'X' if Yarg is None else 'Y'}: cosine max err {err.max() / eps:.2f} eps")
        assert np.array_equal(u, ru) and (err <= (K + 4) * eps).all() and info["launches"] == 3
        assert (cos[u == 3] == 0).all() and (u == 3).any()


def test_edge_scores_without_edges(mctx):
    none = np.zeros(0, np.int64)
    u, v, score, info = graph.edge_scores(none, none, 5, np.ones((5, 2)), ctx=mctx)
    assert len(u) == len(v) == len(score) == 0 and info["launches"] == 0 and info["k"] == 2
    u, v, score, info = graph.edge_scores([1, 1], [1, 1], 3, np.ones((3, 2)), ctx=mctx)   # a self loop alone is no edge
    assert len(score) == 0
    with pytest.raises(ValueError):
        graph.edge_scores([0], [1], 3, np.ones((4, 2)), ctx=mctx)
    with pytest.raises(ValueError):
        graph.edge_scores([0], [1], 3, np.ones((3, 2)), np.ones((3, 3)), ctx=mctx)


# ---- landmark_bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_landmark_bounds_equal_the_model_on_integer_weights(mctx, dt):
    n, r, c = mxv_model._rmat(7, 21)
    w = np.random.default_rng(22).integers(1, 10, len(r)).astype(np.float64)
    deg = np.bincount(np.concatenate([r, c]), minlength=n)
    landmarks = np.argsort(-deg, kind="stable")[:5].astype(np.int64)
    isolated = np.flatnonzero(deg == 0)
    rng = np.random.default_rng(23)
    pairs = np.concatenate([rng.integers(0, n, (60, 2)), [[landmarks[0], 7], [3, 3], [isolated[0], 5], [5, isolated[0]]], [[10, 11], [10, 11]]])
    bound, info = graph.landmark_bounds(r, c, n, landmarks, pairs, w, dtype=dt, ctx=mctx)
    want = model.landmark_bounds(n, r, c, landmarks, pairs, w, dtype=dt)
    assert bound.dtype == dt and bound.shape == (len(pairs),) and np.array_equal(_bits(bound), _bits(want))
    assert np.isposinf(bound[-3]) and np.isposinf(bound[-4]) and bound[-1] == bound[-2]        # unreachable; a repeated pair
    assert np.isfinite(bound).sum() > 30
    assert info["pairs"] == len(pairs) and info["distinct_pairs"] == len({(a, b) for a, b in pairs.tolist()}) < len(pairs)
    assert info["landmarks"] == 5 and info["launches"] == 1 and info["paths"]["rounds"] > 0
    # no pair, no landmark
    empty, info = graph.landmark_bounds(r, c, n, landmarks, [], w, dtype=dt, ctx=mctx)
    assert empty.shape == (0,) and info["launches"] == 0
    nothing, _ = graph.landmark_bounds(r, c, n, [], pairs, w, dtype=dt, ctx=mctx)
    assert np.isposinf(nothing).all()
    with pytest.raises(ValueError):
        graph.landmark_bounds(r, c, n, landmarks, [(0, n)], w, dtype=dt, ctx=mctx)


# ---- factorize ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted_model():
    case = model.planted_case()
    loss = model.factorize(**case)[2]["loss"]
    return case, loss[-1] / loss[0]


@pytest.mark.parametrize("dt", DTYPES)
def test_the_first_steps_library_outputs_equal_the_model(mctx, dt):
    """E, gU and gV of the first step -- the calls graph.factorize makes, on U0 and V0 -- are library outputs on equal inputs."""
    case, _ = _planted_model()
    M, N = case["shape"]
    U0, V0 = case["U0"].astype(dt), case["V0"].astype(dt)
    S, _ = mctx.build(M, N, case["rows"], case["cols"], case["vals"], dup="error", dtype=dt, space="host")
    E = Et = None
    try:
        csr = (S.rowptr.copy(), S.colidx.copy(), S.vals.copy())
        e, gU, gV = model.factorize_step(csr, (M, N), U0, V0)
        E, _ = S.sddmm(U0, V0, accum="minus", space="host")
        Et, _ = E.transpose()
        assert np.array_equal(E.rowptr, csr[0]) and np.array_equal(E.colidx, csr[1]) and np.array_equal(_bits(E.vals), _bits(e))
        assert np.array_equal(_bits(E.mxd(V0, space="host")[0]), _bits(gU))
        assert np.array_equal(_bits(Et.mxd(U0, space="host")[0]), _bits(gV))
    finally:
        for res in (S, E, Et):
            if res is not None:
                res.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_factorize_descends_as_the_float64_model_does(mctx, dt):
    """The loss history does not increase, and final / initial is at most twice the float64 model's: the two trajectories
    differ by rounding alone while the loss is orders above the floor.  Measured on an MI355X: see DESIGN.md section 23."""
    case, model_ratio = _planted_model()
    U, V, info = graph.factorize(**case, dtype=dt, ctx=mctx)
    loss = np.array(info["loss"])
    ratio = loss[-1] / loss[0]
    print(f"{np.dtype(dt).name}: loss {loss[0]:.6g} -> {loss[-1]:.6g}, ratio {ratio:.6e} (float64 model {model_ratio:.6e})")
    assert info["steps"] == case["steps"] == len(loss) and info["nnz"] == len(case["rows"])
    assert U.shape == (20, 3) and V.shape == (15, 3) and U.dtype == V.dtype == dt
    assert (np.diff(loss) <= 0).all()
    assert ratio <= 2 * model_ratio
    # the first step's loss is the model's first loss (the same E, summed in float64)
    first = model.factorize(**{**case, "steps": 1}, dtype=dt)[2]["loss"][0]
    assert abs(loss[0] - first) <= 1e-12 * first
    # what it returns reproduces the last loss's successor: U V^T on the observed entries
    R = case["vals"] - (U.astype(np.float64) @ V.astype(np.float64).T)[case["rows"], case["cols"]]
    assert (R ** 2).sum() <= loss[-1]


@pytest.mark.parametrize("dt", DTYPES)
def test_factorize_on_rank_zero_no_steps_and_an_empty_list(mctx, dt):
    case, _ = _planted_model()
    M, N = case["shape"]
    free = {k: case[k] for k in ("rows", "cols", "vals", "shape", "lr")}
    U, V, info = graph.factorize(**free, rank=0, steps=3, dtype=dt, ctx=mctx)
    s2 = float((case["vals"].astype(dt).astype(np.float64) ** 2).sum())
    assert U.shape == (M, 0) and V.shape == (N, 0) and info["steps"] == 3
    assert np.allclose(info["loss"], [s2] * 3, rtol=1e-12)        # e = s - 0 at every step
    U, V, info = graph.factorize(**free, rank=3, steps=0, U0=case["U0"], V0=case["V0"], dtype=dt, ctx=mctx)
    assert info["loss"] == [] and info["launches"] == 0
    assert np.array_equal(U, case["U0"].astype(dt)) and np.array_equal(V, case["V0"].astype(dt))
    U, V, info = graph.factorize([], [], [], (4, 3), 2, 3, 0.1, reg=0.5, seed=7, dtype=dt, ctx=mctx)
    mU, mV, minfo = model.factorize([], [], [], (4, 3), 2, 3, 0.1, reg=0.5, seed=7, dtype=dt)
    assert info["loss"] == minfo["loss"] == [0.0] * 3 and info["nnz"] == 0
    assert np.allclose(U, mU, rtol=1e-6) and np.allclose(V, mV, rtol=1e-6)   # three steps of weight decay
    with pytest.raises(ValueError):
        graph.factorize(**free, rank=3, steps=1, U0=np.ones((M, 2)), dtype=dt, ctx=mctx)
