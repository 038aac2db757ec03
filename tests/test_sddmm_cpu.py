"""CPU-side checks of the sampled dense-dense product (include/outerspace_spgemm_sddmm.h) and of what is built on it: the
symbol is exported and listed, the stats struct has the layout the C compiler gives it, null and illegal arguments are
argument errors that leave the outputs alone, the Python entries exist, validate operator names, shapes and the ``None`` cases
and fail loudly without a GPU, and the models that judge the GPU (tests/sddmm_model.py) equal things that share nothing with
them: scipy's ``X @ Y.T`` sampled at the pattern, a brute-force minimum, networkx's Dijkstra, plain float64 numpy -- and the
planted factorisation converges the way tests/test_gpu_edge_models.py relies on."""
import ctypes
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import sddmm_model as model
from tests import vector_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_sddmm.h")


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _declared(path):
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_sddmm_header_symbols_are_exported():
    hdr, declared = _declared(HEADER)
    L = _lib.lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert declared == set(_lib.SDDMM_EXPORTS) == {"osp_csr_sddmm"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS, _lib.MXV_EXPORTS, _lib.MXD_EXPORTS, _lib.EXTRACT_EXPORTS,
                  _lib.BUILD_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm_mxd.h"' in hdr
    # the mxd header still declares exactly its one function
    assert _declared(os.path.join(ROOT, "include", "outerspace_spgemm_mxd.h"))[1] == {"osp_csr_mxd"}
    # the model's tables are the binding's
    assert list(_lib.MXV_ADD_OPS) == model.ADD_OPS and list(_lib.MXM_MUL_OPS) == model.MUL_OPS
    assert sorted(_lib.SDDMM_ACCUM_OPS) == sorted(model.ACCUM_OPS) and "first" not in _lib.SDDMM_ACCUM_OPS
    assert model.MAX_COLS == _lib.MXD_MAX_COLS


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


def test_sddmm_stats_have_the_layout_the_c_compiler_gives(tmp_path):
    cname, struct = "osp_sddmm_stats_t", _lib.SddmmStats
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_sddmm.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "cols", "lanes_per_entry", "launches", "ms_total"}


def test_sddmm_null_and_illegal_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in`, whatever else is wrong with it, and a fake
    `in` with a null sr or out (the null checks come before `in` is touched; tests/test_gpu_sddmm.py passes the other bad
    arguments with real results)."""
    L = _lib.lib()
    x = np.ones((4, 2))
    xp = ctypes.c_void_p(x.ctypes.data)
    stats = _lib.SddmmStats()
    stats.nnz_in = 77
    out = ctypes.c_void_p(0x5555)

    def semiring(add, mul, reserved=0):
        sr = _lib.Semiring()
        sr.add, sr.mul = _lib.EWISE_OPS[add], _lib.EWISE_OPS[mul]
        sr.reserved[0] = reserved
        return sr

    sr = semiring("plus", "times")
    fake = ctypes.c_void_p(0x1000)
    host, st, op, second = _lib.OSP_HOST, ctypes.byref(stats), ctypes.byref(out), _lib.EWISE_OPS["second"]
    calls = [lambda: L.osp_csr_sddmm(None, ctypes.byref(sr), second, xp, xp, 2, host, op, st),
             lambda: L.osp_csr_sddmm(None, None, second, None, None, 0, host, None, None),
             lambda: L.osp_csr_sddmm(None, ctypes.byref(sr), second, None, xp, 2, 99, op, st),
             lambda: L.osp_csr_sddmm(None, ctypes.byref(semiring("first", "div")), second, xp, xp, 2, host, op, st),
             lambda: L.osp_csr_sddmm(None, ctypes.byref(semiring("plus", "times", 1)), second, xp, xp, 2, host, op, st),
             lambda: L.osp_csr_sddmm(None, ctypes.byref(sr), _lib.EWISE_OPS["first"], xp, xp, 2, host, op, st),
             lambda: L.osp_csr_sddmm(None, ctypes.byref(sr), second, xp, xp, model.MAX_COLS + 1, host, op, st),
             lambda: L.osp_csr_sddmm(fake, None, second, xp, xp, 2, host, op, st),
             lambda: L.osp_csr_sddmm(fake, ctypes.byref(sr), second, xp, xp, 2, host, None, st)]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert stats.nnz_in == 77 and out.value == 0x5555


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _handleless(shape=(3, 4)):
    res = object.__new__(S.CsrResult)   # (no handle: names and shapes are checked before anything is touched)
    res._h, res.shape, res.dtype, res._ctx = None, shape, np.float64, None
    return res


def test_python_entries_exist_and_validate_names_shapes_and_none():
    assert callable(S.CsrResult.sddmm)
    assert callable(graph.edge_scores) and callable(graph.landmark_bounds) and callable(graph.factorize)
    res = _handleless()
    X, Y = np.ones((3, 2)), np.ones((4, 2))
    for kw in ({"add": "first"}, {"add": "times"}, {"mul": "minus"}, {"mul": "div"}, {"accum": "first"}, {"accum": "sum"}):
        with pytest.raises(ValueError):
            res.sddmm(X, Y, space="host", **kw)
    with pytest.raises(ValueError):
        res.sddmm(X, Y, space="pinned")
    bad = [lambda: res.sddmm(np.ones((4, 2)), Y, space="host"),                     # M is 3
           lambda: res.sddmm(X, np.ones((3, 2)), space="host"),                     # N is 4
           lambda: res.sddmm(np.ones(3), Y, space="host"),                          # X is not 2-D
           lambda: res.sddmm(X, np.ones(4), space="host"),                          # Y is not 2-D
           lambda: res.sddmm(X, np.ones((4, 3)), space="host"),                     # the two k differ
           lambda: res.sddmm(X, Y, k=3, space="host"),                              # k contradicts the shapes
           lambda: res.sddmm(None, Y, space="host"),                                # None without mul="second"
           lambda: res.sddmm(X, None, space="host"),                                # None without mul="first"
           lambda: res.sddmm(None, Y, mul="first", space="host"),                   # first needs X
           lambda: res.sddmm(X, None, mul="second", space="host"),                  # second needs Y
           lambda: res.sddmm(torch.ones(3, 2, dtype=torch.float32), torch.ones(4, 2, dtype=torch.float32)),   # the wrong dtype
           lambda: res.sddmm(torch.ones(3, 4, dtype=torch.float64)[:, :2], torch.ones(4, 2, dtype=torch.float64)),   # not contiguous
           lambda: res.sddmm(0x1000, 0x2000, space="device"),                       # addresses without k
           lambda: res.sddmm(np.ones((3, model.MAX_COLS + 1)), None, mul="first", space="host"),
           lambda: res.sddmm(0x1000, 0x2000, k=-1)]
    for i, call in enumerate(bad):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_ARG, i
    assert [model.lanes_per_entry(k) for k in model.KS] == [1, 1, 2, 4, 4, 8, 16, 32, 64, 64, 64, 64]
    assert model.expected_launches(0) == 0 and model.expected_launches(1) == model.expected_launches(10 ** 9) == 1


def test_graph_functions_validate_their_arguments_first():
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    with pytest.raises(ValueError):
        graph.edge_scores(r, c, 3, None)
    with pytest.raises(ValueError):
        graph.edge_scores(r, c, 3, np.ones((3, 2)), kind="euclid")
    with pytest.raises(ValueError):
        graph.factorize(r, c, np.ones(3), (3, 3), -1, 1, 0.1)
    with pytest.raises(ValueError):
        graph.factorize(r, c, np.ones(3), (3, 3), 2, -1, 0.1)


def test_sddmm_of_a_result_without_a_handle_is_an_error_not_a_host_computation():
    """A call with nothing wrong but the missing handle reaches the C entry and comes back as its argument error: there is
    no path that computes the product on the host."""
    res = _handleless()
    X, Y = np.ones((3, 2)), np.ones((4, 2))
    for args, kw in (((X, Y), {}), ((X, Y), {"add": "min", "mul": "plus", "accum": "minus"}), ((X, None), {"mul": "first"}),
                     ((None, Y), {"mul": "second", "accum": None}), ((np.ones((3, 0)), np.ones((4, 0))), {})):
        with pytest.raises(S.OspError) as ei:
            res.sddmm(*args, space="host", **kw)
        assert ei.value.status == _lib.ERR_ARG and "null argument" in str(ei.value)
    sq = _handleless((3, 3))
    with pytest.raises(S.OspError) as ei:
        sq.sddmm(X, X, space="host")   # Y is X
    assert "null argument" in str(ei.value)


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(S.OspError) as ei:
        S.Context(0)   # (what every CsrResult, and so every sddmm call, needs first)
    assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.edge_scores(r, c, 3, np.ones((3, 2))),
                 lambda: graph.landmark_bounds(r, c, 3, [0], [(1, 2)]),
                 lambda: graph.factorize(r, c, np.ones(3), (3, 3), 2, 1, 0.1)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of sddmm against independent references ----------------------------------------------------------------------------
def _small_pattern(dt, seed=4):
    rng = np.random.default_rng(seed)
    M, N = 23, 31
    A = sp.random(M, N, density=0.3, random_state=seed, format="csr")
    A.sort_indices()
    return M, N, (A.indptr.astype(np.int64), A.indices.astype(np.uint32), rng.standard_normal(A.nnz).astype(dt)), rng


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("k", [0, 1, 5, 64, 70, 2049, 4100])
def test_the_model_is_scipys_sampled_product_on_exact_values(dt, k):
    """Small integers times powers of two: every product and every partial sum is exact in float32, so any order of
    summation gives the bits of scipy's (X @ Y.T) sampled at the pattern."""
    M, N, (rowptr, col, val), rng = _small_pattern(dt)
    X = (rng.integers(-4, 5, (M, k)) * 2.0 ** rng.integers(-2, 3, (M, k))).astype(dt)
    Y = (rng.integers(-4, 5, (N, k)) * 2.0 ** rng.integers(-2, 3, (N, k))).astype(dt)
    got, computed = model.sddmm(rowptr, col, val, X, Y)
    dense = X.astype(np.float64) @ Y.astype(np.float64).T
    rows = np.repeat(np.arange(M), np.diff(rowptr))
    want = np.asarray(sp.csr_matrix(dense)[rows, col.astype(np.int64)]).ravel() if k else np.zeros(len(col))
    assert computed and got.dtype == dt and np.array_equal(got, want.astype(dt)) and not np.signbit(got[got == 0]).any()
    # accum: in's value in a's place
    minus = model.sddmm(rowptr, col, val, X, Y, accum="minus")[0]
    assert np.array_equal(minus, val - want.astype(dt))
    assert np.array_equal(model.sddmm(rowptr, col, val, X, Y, accum=None)[0], got)
    with pytest.raises(ValueError):
        model.sddmm(rowptr, col, val, X, Y, accum="first")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_under_min_plus_is_a_brute_force_minimum(dt):
    M, N, (rowptr, col, val), rng = _small_pattern(dt, seed=6)
    for k in (0, 1, 7, 65, 2100):
        X, Y = rng.standard_normal((M, k)).astype(dt), rng.standard_normal((N, k)).astype(dt)
        if k > 1:
            X[3, 1], Y[5, 0] = np.inf, np.inf
        got, computed = model.sddmm(rowptr, col, val, X, Y, "min", "plus")
        rows = np.repeat(np.arange(M), np.diff(rowptr))
        want = np.array([min([X[i, c] + Y[j, c] for c in range(k)], default=dt(np.inf)) for i, j in zip(rows, col.astype(np.int64))], dt)
        assert not computed and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_is_mxv_of_the_one_row_csr(dt):
    """The equivalence the header states, on the model's side: every entry's d is mxv_model's y[0]."""
    M, N, (rowptr, col, val), rng = _small_pattern(dt, seed=8)
    for k in (3, 64, 100, 2050):
        X, Y = rng.standard_normal((M, k)).astype(dt), rng.standard_normal((N, k)).astype(dt)
        entries = rng.choice(len(col), size=12, replace=False)
        for add, mul in (("plus", "times"), ("min", "plus"), ("max", "second")):
            got = model.sddmm(rowptr, col, val, X, Y, add, mul)[0][entries]
            assert np.array_equal(_bits(got), _bits(model.sddmm_by_mxv(rowptr, col, X, Y, add, mul, entries)))


def test_the_fma_input_tells_a_fused_fold_from_two_roundings():
    X, Y = model.fma_telling_dense()
    n = len(X)
    rowptr, col = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.uint32)
    two = model.sddmm(rowptr, col, np.ones(n, np.float32), X, Y)[0]
    assert X.shape[1] > vector_model.WAVE and (_bits(two) != _bits(model.fma_diagonal(X, Y))).any()


# ---- the models of the graph functions -------------------------------------------------------------------------------------------
def _weighted_rmat():
    from tests import mxv_model
    n, r, c = mxv_model._rmat(7, 21)
    w = np.random.default_rng(22).integers(1, 10, len(r)).astype(np.float64)
    return n, r, c, w


def _nx_graph(n, r, c, w):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for a, b, x in zip(r.tolist(), c.tolist(), w.tolist()):
        if a != b and (not G.has_edge(a, b) or G[a][b]["weight"] > x):
            G.add_edge(a, b, weight=x)
    return G


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_landmark_model_against_networkx_dijkstra(dt):
    """Integer weights: every path length is exact, so the model equals min_c d(c, u) + d(c, v) of networkx's distances
    exactly; it is never below the true distance, and equals it when u is a landmark."""
    n, r, c, w = _weighted_rmat()
    G = _nx_graph(n, r, c, w)
    deg = np.bincount(np.concatenate([r, c]), minlength=n)
    landmarks = np.argsort(-deg, kind="stable")[:5].astype(np.int64)
    isolated = np.flatnonzero(deg == 0)
    assert len(isolated)
    rng = np.random.default_rng(23)
    pairs = np.concatenate([rng.integers(0, n, (60, 2)), [[landmarks[0], 7], [landmarks[2], 9], [3, 3], [isolated[0], 5]],
                            [[10, 11], [10, 11]]])
    got = model.landmark_bounds(n, r, c, landmarks, pairs, w, dtype=dt)
    dist = {int(s): nx.single_source_dijkstra_path_length(G, int(s)) for s in set(landmarks.tolist()) | set(pairs[:, 0].tolist())}
    want = np.array([min(dist[int(s)].get(int(u), np.inf) + dist[int(s)].get(int(v), np.inf) for s in landmarks) for u, v in pairs])
    true = np.array([dist[int(u)].get(int(v), np.inf) for u, v in pairs])
    assert got.dtype == dt and np.array_equal(got.astype(np.float64), want)
    assert (got >= true).all() and np.isinf(got[-3]) and got[-1] == got[-2]
    from_landmark = np.isin(pairs[:, 0], landmarks)
    assert from_landmark.sum() >= 2 and np.array_equal(got[from_landmark], true[from_landmark])
    assert len(model.landmark_bounds(n, r, c, landmarks, np.zeros((0, 2), np.int64), w, dtype=dt)) == 0
    assert np.isinf(model.landmark_bounds(n, r, c, [], pairs, w, dtype=dt)).all()


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("kind", ["dot", "cosine"])
def test_the_score_model_against_plain_numpy(kind, directed):
    """(k + 4) eps relative to ||x|| ||y||: one rounding per product and per addition, and the two scalings."""
    from tests import mxv_model
    n, r, c = mxv_model._rmat(7, 31)
    k = 6
    rng = np.random.default_rng(32)
    X, Y = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    X[5] = 0.0
    for dt in (np.float32, np.float64):
        for Yarg in (None, Y):
            u, v, score = model.edge_scores(n, r, c, X.astype(dt), None if Yarg is None else Y.astype(dt), kind, directed, dt)
            ru, rv, ref, scale = model.reference_edge_scores(n, r, c, X.astype(dt), None if Yarg is None else Y.astype(dt), kind, directed)
            assert np.array_equal(u, ru) and np.array_equal(v, rv) and score.dtype == dt and len(u) > 100
            assert directed or (u < v).all()
            bound = (k + 4) * float(np.finfo(dt).eps) * (scale if kind == "dot" else np.ones_like(scale))
            assert (np.abs(score.astype(np.float64) - ref) <= bound).all()
            if kind == "cosine":
                assert (score[(u == 5)] == 0).all() and (np.abs(score) <= 1 + bound).all()


def test_the_planted_factorisation_descends_far_above_the_rounding_floor():
    """What tests/test_gpu_edge_models.py relies on: in float64 the loss never increases over the chosen steps, and ends
    between 1e-4 and 1e-1 of where it began -- orders above what float32's rounding could blur."""
    case = model.planted_case()
    assert case["shape"] == (20, 15) and case["rank"] == 3
    share = len(case["rows"]) / 300
    assert 0.5 < share < 0.7
    U, V, info = model.factorize(**case)
    loss = np.array(info["loss"])
    ratio = loss[-1] / loss[0]
    print(f"planted case: nnz={info['nnz']} lr={case['lr']} steps={case['steps']} loss {loss[0]:.4g} -> {loss[-1]:.4g} ratio {ratio:.3e}")
    assert info["steps"] == case["steps"] == len(loss) and (np.diff(loss) <= 0).all()
    assert 1e-4 <= ratio <= 1e-1
    # the float32 model descends alongside it
    loss32 = np.array(model.factorize(**case, dtype=np.float32)[2]["loss"])
    assert (np.diff(loss32) <= 0).all() and loss32[-1] / loss32[0] <= 2 * ratio
    # the gradient the steps use is the gradient: e, gU and gV against dense float64 algebra on the mask
    M, N = case["shape"]
    S = sp.csr_matrix((case["vals"], (case["rows"], case["cols"])), shape=(M, N))
    S.sort_indices()
    csr = (S.indptr.astype(np.int64), S.indices.astype(np.uint32), S.data)
    e, gU, gV = model.factorize_step(csr, (M, N), case["U0"], case["V0"])
    mask = S.copy(); mask.data[:] = 1.0
    R = S.toarray() - mask.toarray() * (case["U0"] @ case["V0"].T)
    assert np.allclose(sp.csr_matrix((e, csr[1].astype(np.int64), csr[0]), shape=(M, N)).toarray(), R, atol=1e-12)
    assert np.allclose(gU, R @ case["V0"], atol=1e-12) and np.allclose(gV, R.T @ case["U0"], atol=1e-12)
    # the edge cases the GPU test repeats
    for kw in ({"rank": 0}, {"steps": 0}):
        U, V, info = model.factorize(**{**case, **kw, "U0": None, "V0": None})
        assert U.shape == (M, kw.get("rank", 3)) and info["steps"] == kw.get("steps", case["steps"])
    U, V, info = model.factorize([], [], [], (4, 3), 2, 3, 0.1, reg=0.5)
    assert info["loss"] == [0.0, 0.0, 0.0] and U.shape == (4, 2)
