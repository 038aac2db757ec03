"""CPU-side checks of the product of a result with a dense vector (include/outerspace_spgemm_mxv.h) and of what is built on
it: the symbol is exported and listed, the stats struct has the layout the C compiler gives it, null and illegal arguments
are argument errors that leave the outputs alone, the Python entries exist, validate their operator names and fail loudly
without a GPU, and the models that judge the GPU (tests/mxv_model.py) equal things that share nothing with them: scipy's
``A @ x``, a literal loop, networkx's PageRank and scipy's components."""
import ctypes
import math
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import connected_components

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import mxv_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_mxv.h")
RANK_GRAPHS = model.rank_graphs()
COMPONENT_GRAPHS = model.component_graphs()
ALPHA, TOL = 0.85, 1e-10


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_mxv_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.MXV_EXPORTS) == {"osp_csr_mxv"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm_mxm.h"' in hdr
    # the model's block and wave are the kernels'
    src = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_vector.h")).read()
    assert int(re.search(r"kReduceBlock\s*=\s*(\d+)", src).group(1)) == model.vector_model.BLOCK
    assert list(_lib.MXV_ADD_OPS) == model.ADD_OPS and list(_lib.MXM_MUL_OPS) == model.MUL_OPS


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


def test_mxv_stats_have_the_layout_the_c_compiler_gives(tmp_path):
    cname, struct = "osp_mxv_stats_t", _lib.MxvStats
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_mxv.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "long_segments", "group", "launches", "ms_total"}


def test_mxv_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in`, and a fake `in` with a null sr or y (the
    null checks come before `in` is touched; tests/test_gpu_mxv.py passes the other bad arguments with real results)."""
    L = _lib.lib()
    y = np.full(4, 7.0)
    x = np.ones(4)
    yp, xp = ctypes.c_void_p(y.ctypes.data), ctypes.c_void_p(x.ctypes.data)
    stats = _lib.MxvStats()
    stats.nnz_in = 77
    sr = _lib.Semiring()
    sr.add, sr.mul = _lib.MXV_ADD_OPS["plus"], _lib.MXM_MUL_OPS["times"]
    bad = _lib.Semiring()
    bad.add, bad.mul = _lib.EWISE_OPS["first"], _lib.EWISE_OPS["div"]
    fake = ctypes.c_void_p(0x1000)
    calls = [lambda: L.osp_csr_mxv(None, ctypes.byref(sr), xp, yp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(None, ctypes.byref(bad), xp, yp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(None, None, None, None, _lib.OSP_HOST, None),
             lambda: L.osp_csr_mxv(None, ctypes.byref(sr), None, yp, 99, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(fake, None, xp, yp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv(fake, ctypes.byref(sr), xp, None, _lib.OSP_HOST, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert stats.nnz_in == 77 and (y == 7.0).all()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_entries_exist_and_validate_operator_names():
    assert callable(S.CsrResult.mxv) and callable(graph.pagerank) and callable(graph.connected_components)
    res = object.__new__(S.CsrResult)   # (no handle: the names are checked before anything is touched)
    res._h, res.shape, res.dtype = None, (3, 3), np.float64
    for kw in ({"add": "first"}, {"add": "times"}, {"mul": "minus"}, {"mul": "div"}, {"add": "sum"}):
        with pytest.raises(ValueError):
            res.mxv(np.ones(3), space="host", **kw)
    with pytest.raises(ValueError):
        res.mxv(np.ones(3), space="pinned")


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.pagerank(r, c), lambda: graph.pagerank(r, c, directed=True), lambda: graph.connected_components(r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of mxv ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_is_scipys_product_on_exact_values(dt):
    """Small integers times powers of two: every product and every partial sum is exact in float32, so any order of
    summation gives scipy's bits.  Rows of 0 to 5000 entries: one lane step, several, and two levels of blocks."""
    rng = np.random.default_rng(2)
    ncol = 6000
    lengths = [0, 1, 3, 64, 65, 700, 2048, 2049, 5000, 0, 17]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=k, replace=False)) for k in lengths]).astype(np.uint32)
    val = rng.integers(-8, 9, len(col)).astype(dt)
    x = (rng.integers(-4, 5, ncol) * 2.0 ** rng.integers(-2, 3, ncol)).astype(dt)
    got, nlong = model.mxv(rowptr, col, val, x, "plus", "times")
    want = sp.csr_matrix((val, col.astype(np.int64), rowptr), shape=(len(lengths), ncol)) @ x
    assert got.dtype == dt and nlong == 2
    assert np.array_equal(got, want.astype(dt)) and got[0] == 0 and not np.signbit(got[0])


def _loop(rowptr, col, val, x, add, mul):
    """A literal loop over R's definition for rows of at most 64 entries: 64 lane values, the butterfly 32 .. 1."""
    dt = val.dtype.type
    idv = {"min": dt(np.inf), "max": dt(-np.inf)}[add]
    comb = {"min": lambda a, b: b if b < a else a, "max": lambda a, b: b if b > a else a}
    mulf = {"plus": lambda a, b: a + b, "min": lambda a, b: b if b < a else a}[mul]
    out = []
    with np.errstate(all="ignore"):
        for i in range(len(rowptr) - 1):
            p = [idv] * 64
            for l, q in enumerate(range(rowptr[i], rowptr[i + 1])):
                p[l] = comb[add](p[l], mulf(val[q], x[col[q]]))
            d = 32
            while d:
                for l in range(d):
                    p[l] = comb[add](p[l], p[l + d])
                d //= 2
            out.append(p[0])
    return np.array(out, dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("add,mul", [("min", "plus"), ("max", "min")])
def test_the_model_is_a_literal_loop_on_a_hand_written_matrix(dt, add, mul):
    """4 x 6: row 2 is empty; a NaN, -0.0 and both infinities among the values and in x."""
    rowptr = np.array([0, 3, 5, 5, 9], np.int64)
    col = np.array([0, 2, 5, 1, 2, 0, 1, 4, 5], np.uint32)
    val = np.array([1.5, np.nan, -0.0, np.inf, -np.inf, 0.0, 2.0, -3.0, 4.0], dt)
    x = np.array([-0.0, np.nan, 2.5, 7.0, np.inf, -np.inf], dt)
    got, nlong = model.mxv(rowptr, col, val, x, add, mul)
    want = _loop(rowptr, col, val, x, add, mul)
    assert nlong == 0 and np.array_equal(_bits(got), _bits(want))
    assert not np.isnan(got).any()                                   # MIN and MAX never return a NaN
    assert got[2] == (np.inf if add == "min" else -np.inf)           # the empty row: the identity


def test_the_fma_input_tells_a_contracted_fold_from_the_model():
    ncol, (rowptr, col, val, ), x = model.fma_telling_input()
    want, _ = model.mxv(rowptr, col, val, x, "plus", "times")
    fused = model.fma_mxv_plus_times(rowptr, col, val, x)
    assert want.dtype == fused.dtype == np.float32
    assert (_bits(want) != _bits(fused)).any()


# ---- the models of the graph functions -------------------------------------------------------------------------------------------
def _networkx_rank(n, rows, cols, directed, tol):
    G = nx.from_scipy_sparse_array(model.pattern(n, rows, cols, directed), create_using=nx.DiGraph)
    pr = nx.pagerank(G, alpha=ALPHA, tol=tol, max_iter=1000, weight=None)
    return np.array([pr[v] for v in range(n)])


def rank_bound(n, tol):
    """Both iterations stop with an L1 change below n tol; the iteration contracts by alpha, so each iterate is within
    alpha / (1 - alpha) n tol of the fixed point, and two of them within twice that of each other."""
    return 2.0 * ALPHA / (1.0 - ALPHA) * n * tol


@pytest.mark.parametrize("name", list(RANK_GRAPHS))
def test_the_pagerank_model_is_networkx(name):
    n, r, c, directed = RANK_GRAPHS[name]
    rank, info = model.pagerank(n, r, c, directed, alpha=ALPHA, tol=TOL, max_iter=1000)
    want = _networkx_rank(n, r, c, directed, TOL)
    dist = float(np.abs(rank - want).sum())
    print(f"{name}: iterations={info['iterations']} L1 distance={dist:.3e} bound={rank_bound(n, TOL):.3e}")
    assert info["converged"] and rank.dtype == np.float64
    assert dist <= rank_bound(n, TOL)
    assert abs(rank.sum() - 1.0) < 1e-9
    if name == "edgeless":
        assert info["iterations"] == 0 and np.array_equal(rank, np.full(n, 1.0 / n))
    if name == "dangling":
        A = model.pattern(n, r, c, directed)
        assert (np.diff(A.indptr) == 0).sum() == 3


def test_the_pagerank_model_stops_at_max_iter():
    n, r, c, directed = RANK_GRAPHS["rmat8 directed"]
    _, info = model.pagerank(n, r, c, directed, tol=TOL, max_iter=3)
    assert info["iterations"] == 3 and not info["converged"] and info["err"] >= n * TOL


def _scipy_labels(n, rows, cols):
    A = sp.csr_matrix((np.ones(len(rows)), (np.asarray(rows), np.asarray(cols))), shape=(n, n))
    ncomp, label = connected_components(A, directed=False)
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, label, np.arange(n))
    return smallest[label], ncomp


@pytest.mark.parametrize("name", list(COMPONENT_GRAPHS))
def test_the_component_model_is_scipys_components(name):
    n, r, c = COMPONENT_GRAPHS[name]
    labels, info = model.connected_components(n, r, c)
    want, ncomp = _scipy_labels(n, r, c)
    print(f"{name}: rounds={info['rounds']} components={info['components']}")
    assert labels.dtype == np.int64 and np.array_equal(labels, want)
    assert info["components"] == ncomp
    if name == "path":
        assert info["rounds"] <= math.ceil(math.log2(n)) + 2         # the pointer jump: not the 1000 rounds of plain propagation
    if name == "two cliques":
        assert labels.tolist() == [0] * 6 + [6] + [7] * 6
    if name == "isolated vertices":
        assert labels.tolist() == [0, 1, 2, 1, 4, 5, 6, 5, 8]
    labels32, info32 = model.connected_components(n, r, c, np.float32)
    assert np.array_equal(labels32, labels) and info32 == info


def test_the_component_model_refuses_float32_above_2_24():
    with pytest.raises(ValueError):
        model.connected_components((1 << 24) + 1, np.zeros(0, np.int64), np.zeros(0, np.int64), np.float32)
