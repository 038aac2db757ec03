"""CPU-side checks of the semiring product of two results (include/outerspace_spgemm_mxm.h) and of the path functions built on
it: the symbol is exported and listed, both structs have the layout the C compiler gives them, null arguments are argument
errors that leave the outputs alone, without a GPU the Python entries fail loudly, the model that judges the GPU
(tests/semiring_model.py) follows the header's definition -- a literal triple loop on a hand-written pair for all 24
semirings, scipy's product, a dense min-plus --, and its graph functions equal scipy's Dijkstra and a plain widest-path
Dijkstra AS FLOATS: with integer weights every path sum is exact, and with random float weights the frontier loop adds a
path's edges in the order Dijkstra does."""
import ctypes
import heapq
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import dijkstra

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import semiring_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_mxm.h")
SEMIRINGS = [(a, m) for a in model.ADD_OPS for m in model.MUL_OPS]


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _same(got, want):
    """Equal as bits; a NaN equals any NaN (a computed NaN's sign and payload are the machine's)."""
    nan = np.isnan(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.isnan(got[nan]).all()) and \
        np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def test_mxm_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    assert declared
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.MXM_EXPORTS) == {"osp_csr_mxm"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm_ewise.h"' in hdr
    assert len(SEMIRINGS) == 24
    assert set(_lib.MXM_ADD_OPS) == set(model.ADD_OPS) and set(_lib.MXM_MUL_OPS) == set(model.MUL_OPS)
    assert all(_lib.MXM_ADD_OPS[k] == _lib.EWISE_OPS[k] for k in model.ADD_OPS)
    assert all(_lib.MXM_MUL_OPS[k] == _lib.EWISE_OPS[k] for k in model.MUL_OPS)
    # the model's constants are the kernels'
    src = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_mxm.h")).read()
    assert int(re.search(r"kMxmShortMax\s*=\s*(\d+)", src).group(1)) == model.SHORT_CAP
    assert 1 << int(re.search(r"kMxmBatchDefault\s*=\s*1ull\s*<<\s*(\d+)", src).group(1)) == model.BATCH


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_semiring_t", _lib.Semiring), ("osp_mxm_stats_t", _lib.MxmStats)])
def test_mxm_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_mxm.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_mxm_stats_dict():
    assert set(_lib.MxmStats().as_dict()) == {"nnz_a", "nnz_b", "products", "nnz_out", "short_rows", "long_rows", "batches", "launches",
                                               "ms_total"}


def test_mxm_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: null operands, alone and with the other pointers null
    (tests/test_gpu_mxm.py passes the other bad arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.MxmStats()
    stats.products = 77
    sr = _lib.Semiring()
    sr.add, sr.mul = _lib.EWISE_OPS["min"], _lib.EWISE_OPS["plus"]
    fake = ctypes.c_void_p(0)
    calls = [lambda: L.osp_csr_mxm(None, None, ctypes.byref(sr), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_mxm(fake, fake, ctypes.byref(sr), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_mxm(None, None, None, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_mxm(None, None, ctypes.byref(sr), None, ctypes.byref(stats)),
             lambda: L.osp_csr_mxm(None, None, ctypes.byref(sr), ctypes.byref(out), None)]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.products == 77


def test_path_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.shortest_paths(r, c), lambda: graph.widest_paths(r, c, sources=[0, 1]), lambda: graph.min_plus_closure(r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


def test_bad_path_arguments_are_python_errors():
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for fn in (graph.shortest_paths, graph.widest_paths, graph.min_plus_closure):
        with pytest.raises(ValueError):
            fn(r, c, weights=[1.0, -2.0, 3.0])
        with pytest.raises(ValueError):
            fn(r, c, weights=[1.0, np.nan, 3.0])
        with pytest.raises(TypeError):
            fn(r, c, dtype=np.int32)


# ---- the model against the header's definition, written out -----------------------------------------------------------------
def _scalar_op(name, a, b):
    with np.errstate(all="ignore"):
        return {"plus": lambda: a + b, "times": lambda: a * b, "min": lambda: b if b < a else a, "max": lambda: b if b > a else a,
                "first": lambda: a, "second": lambda: b}[name]()


def _literal_mxm(A, B, add, mul):
    """Section 1 of the header, loop by loop, on dense arrays of (stored?, value): for every (i, j) the common k ascending,
    acc = p_0, acc = add(acc, p_t)."""
    (Ah, Av), (Bh, Bv) = A, B
    out = {}
    for i in range(Ah.shape[0]):
        for j in range(Bh.shape[1]):
            acc = None
            for k in range(Ah.shape[1]):
                if Ah[i, k] and Bh[k, j]:
                    p = _scalar_op(mul, Av[i, k], Bv[k, j])
                    acc = p if acc is None else _scalar_op(add, acc, p)
            if acc is not None:
                out[(i, j)] = acc
    return out


def _hand_pair(dt):
    """4 x 5 times 5 x 6 with NaN, both zeros and both infinities among the values, an empty row of A (2), an empty row of B
    (3) that A points at, and output entries fed by one to four products."""
    nan, inf = np.nan, np.inf
    Ah = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 1, 0, 1, 1]], bool)
    Av = np.array([[1e16, 1.0, -1e16, 7.0, -0.0], [nan, 0, -inf, 0, 0], [0, 0, 0, 0, 0], [0, 0.0, 0, 5.0, inf]], dt)
    Bh = np.array([[1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 1], [1, 1, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 1, 1]], bool)
    Bv = np.array([[1.0, nan, 0, 0, -0.0, 2.0], [1.0, 0, inf, 0, 0.0, -3.0], [1.0, -inf, 0, 0, -0.0, 0], [0] * 6, [-0.0, 0, 0, 0, nan, 0.5]], dt)
    return (Ah, Av), (Bh, Bv)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("add,mul", SEMIRINGS)
def test_model_follows_the_definition_on_a_hand_written_pair(add, mul, dt):
    A, B = _hand_pair(dt)
    want = _literal_mxm(A, B, add, mul)
    (rowptr, col, val), st = model.mxm(model._dense_to_csr(*A), model._dense_to_csr(*B), 6, add, mul)
    rows = np.repeat(np.arange(4), np.diff(rowptr))
    assert [(int(i), int(j)) for i, j in zip(rows, col)] == sorted(want)
    assert val.dtype == dt
    wv = np.array([want[k] for k in sorted(want)], dt)
    assert _same(val, wv), (val, wv)
    assert rowptr[2] == rowptr[3] and 3 not in col                      # the empty row of A; column 3 of B is empty
    assert st["products"] == sum(int(B[0][k].sum()) for i in range(4) for k in range(5) if A[0][i, k])
    assert st["nnz_out"] == len(want) and st["long_rows"] == 0 and st["short_rows"] == 3 and st["batches"] == 1
    if (add, mul) == ("plus", "times") and dt == np.float64:
        assert want[(0, 0)] == 0.0       # (1e16 + 1) - 1e16 in ascending k: the 1 is lost, the order is visible
    if (add, mul) == ("min", "first"):
        assert np.isnan(want[(1, 0)])    # MIN keeps p_0 when it is a NaN


def test_model_plus_times_is_scipy_on_integers():
    rng = np.random.default_rng(3)
    A = sp.random(70, 50, 0.1, random_state=1, format="csr", data_rvs=lambda k: rng.integers(1, 9, k).astype(np.float64))
    B = sp.random(50, 90, 0.1, random_state=2, format="csr", data_rvs=lambda k: rng.integers(1, 9, k).astype(np.float64))
    for M in (A, B):
        M.sort_indices()
    (rowptr, col, val), st = model.mxm((A.indptr, A.indices, A.data), (B.indptr, B.indices, B.data), 90)
    C = (A @ B).tocsr()
    C.sort_indices()
    assert np.array_equal(rowptr, C.indptr) and np.array_equal(col, C.indices) and np.array_equal(val, C.data)
    assert st["products"] == int((A.astype(bool).astype(np.int64) @ np.diff(B.indptr)).sum())


def test_model_min_plus_is_the_dense_one():
    rng = np.random.default_rng(5)
    a = np.where(rng.random((13, 17)) < 0.4, rng.integers(0, 20, (13, 17)).astype(np.float64), np.inf)
    b = np.where(rng.random((17, 11)) < 0.4, rng.integers(0, 20, (17, 11)).astype(np.float64), np.inf)
    (rowptr, col, val), _ = model.mxm(model._dense_to_csr(np.isfinite(a), a), model._dense_to_csr(np.isfinite(b), b), 11, "min", "plus")
    want = np.min(a[:, :, None] + b[None], axis=1)
    has, got = model._csr_to_dense((rowptr, col, val), (13, 11), np.float64)
    assert np.array_equal(has, np.isfinite(want)) and np.array_equal(got[has], want[has])


def test_model_batches_cut_as_the_header_says():
    assert model.cut_batches(np.array([0, 0, 5, 3, 0, 20, 1, 1]), 8) == [(0, 5), (5, 6), (6, 8)]
    assert model.cut_batches(np.array([9, 9]), 8) == [(0, 1), (1, 2)]
    assert model.cut_batches(np.array([3, 0, 0]), 100) == [(0, 3)]


# ---- the graph models against Dijkstra ----------------------------------------------------------------------------------------
def _graphs():
    n, r, c, _ = gen.rmat_coo(8, 4, seed=5)
    r, c = r.astype(np.int64), c.astype(np.int64)
    star = (np.zeros(9, np.int64), np.arange(1, 10))
    return {"rmat8": (n, r, c), "path": (12, np.arange(11), np.arange(1, 12)), "star": (10,) + star,
            "isolated": (7, np.array([0, 1, 4, 4, 2]), np.array([1, 2, 5, 4, 0])), "edgeless": (5, np.zeros(0, np.int64), np.zeros(0, np.int64))}


def _int_weights(m, seed):
    return np.random.default_rng(seed).integers(1, 10, m).astype(np.float64)


def _scipy_graph(W, n):
    return sp.csr_matrix((W[2], W[1].astype(np.int64), W[0]), shape=(n, n))


def _widest_dijkstra(W, n, s):
    rowptr, col, val = W
    width = np.zeros(n)
    width[s] = np.inf
    heap, done = [(-np.inf, s)], np.zeros(n, bool)
    while heap:
        _, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for e in range(rowptr[u], rowptr[u + 1]):
            v, w = int(col[e]), min(width[u], val[e])
            if w > width[v]:
                width[v] = w
                heapq.heappush(heap, (-w, v))
    return width


@pytest.mark.parametrize("name", ["rmat8", "path", "star", "isolated", "edgeless"])
def test_path_models_equal_dijkstra_on_integer_weights(name):
    n, r, c = _graphs()[name]
    w = _int_weights(len(r), 11)
    sources = [0, n - 1, n // 2]
    Wmin = model.weighted_adjacency(r, c, n, w)
    dist, info = model.shortest_paths(Wmin, n, sources)
    want = dijkstra(_scipy_graph(Wmin, n), directed=True, indices=sources) if len(Wmin[1]) else np.where(np.eye(n, dtype=bool)[sources], 0.0, np.inf)
    assert np.array_equal(dist, want)
    assert info["rounds"] == len(info["frontier_nnz"]) == len(info["products"]) and (info["rounds"] > 0) == (len(r) > 0)
    hops, _ = model.shortest_paths(model.weighted_adjacency(r, c, n), n, sources)
    assert np.array_equal(hops, dijkstra(_scipy_graph(Wmin, n), directed=True, indices=sources, unweighted=True) if len(Wmin[1]) else want)
    Wmax = model.weighted_adjacency(r, c, n, w, keep="max")
    width, _ = model.widest_paths(Wmax, n, sources)
    assert np.array_equal(width, np.stack([_widest_dijkstra(Wmax, n, s) for s in sources]))
    (rowptr, col, val), rounds = model.min_plus_closure(Wmin, n)
    has, D = model._csr_to_dense((rowptr, col, val), (n, n), np.float64)
    allp = dijkstra(_scipy_graph(Wmin, n), directed=True) if len(Wmin[1]) else np.where(np.eye(n, dtype=bool), 0.0, np.inf)
    assert np.array_equal(has, np.isfinite(allp)) and np.array_equal(D[has], allp[has])
    assert rounds <= max(int(np.ceil(np.log2(n))), 0)


def test_frontier_loop_equals_dijkstra_on_random_float_weights():
    n, r, c = _graphs()["rmat8"]
    w = np.random.default_rng(17).random(len(r)) + 0.1
    W = model.weighted_adjacency(r, c, n, w)
    dist, _ = model.shortest_paths(W, n, [0, 3, 100])
    assert np.array_equal(dist, dijkstra(_scipy_graph(W, n), directed=True, indices=[0, 3, 100]))


def test_weighted_adjacency_keeps_the_extreme_duplicate_and_drops_loops():
    r, c, w = [0, 1, 0, 2, 2], [1, 0, 1, 2, 0], [5.0, 2.0, 3.0, 9.0, 4.0]
    for keep, w01 in (("min", 2.0), ("max", 5.0)):
        rowptr, col, val = model.weighted_adjacency(r, c, 3, w, keep=keep)
        assert rowptr.tolist() == [0, 2, 3, 4] and col.tolist() == [1, 2, 0, 0] and val.tolist() == [w01, 4.0, w01, 4.0]
        n, rp, ci, va = graph.weighted_adjacency(r, c, 3, w, keep=keep)
        assert n == 3 and rp.tolist() == rowptr.tolist() and ci.tolist() == col.tolist() and va.tolist() == val.tolist()
    rowptr, col, val = model.weighted_adjacency(r, c, 3, w, directed=True)
    assert rowptr.tolist() == [0, 1, 2, 3] and col.tolist() == [1, 0, 0] and val.tolist() == [3.0, 2.0, 4.0]
    n, rp, ci, va = graph.weighted_adjacency(r, c, 3, w, directed=True)
    assert rp.tolist() == rowptr.tolist() and ci.tolist() == col.tolist() and va.tolist() == val.tolist()
