"""CPU-side checks of mxv with the winner's column (include/outerspace_spgemm_mxv_arg.h) and of what is built on it: the
symbol is exported and listed, the stats struct has the layout the C compiler gives it, null arguments are argument errors
that leave the outputs alone, the Python entries exist, validate their arguments before they need a GPU and fail loudly
without one, and the models that judge the GPU (tests/mxv_arg_model.py) equal things that share nothing with them: numpy's
argmin / argmax on dense rows, scipy's minimum spanning tree, networkx's spanning edges and its optimal matching."""
import ctypes
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import minimum_spanning_tree

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import mxv_arg_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_mxv_arg.h")
GRAPHS = model.graphs()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_mxv_arg_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.MXV_ARG_EXPORTS) == {"osp_csr_mxv_arg"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS, _lib.MXV_EXPORTS, _lib.MXD_EXPORTS, _lib.SDDMM_EXPORTS,
                  _lib.EXTRACT_EXPORTS, _lib.BUILD_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm_mxv.h"' in hdr
    assert list(_lib.MXV_ARG_ADD_OPS) == model.ADD_OPS == ["min", "max"] and list(_lib.MXM_MUL_OPS) == model.MUL_OPS
    assert all(_lib.MXV_ARG_ADD_OPS[a] == _lib.MXV_ADD_OPS[a] for a in model.ADD_OPS)


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


def test_mxv_arg_stats_have_the_layout_the_c_compiler_gives(tmp_path):
    cname, struct = "osp_mxv_arg_stats_t", _lib.MxvArgStats
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_mxv_arg.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "long_segments", "rows_without", "group", "launches", "ms_total"}


def test_mxv_arg_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in`, and a fake `in` with a null sr or arg (the
    null checks come before `in` is touched; tests/test_gpu_mxv_arg.py passes the other bad arguments with real results)."""
    L = _lib.lib()
    y, x, arg = np.full(4, 7.0), np.ones(4), np.full(4, 7, np.int64)
    yp, xp, ap = (ctypes.c_void_p(a.ctypes.data) for a in (y, x, arg))
    stats = _lib.MxvArgStats()
    stats.nnz_in = 77
    sr = _lib.Semiring()
    sr.add, sr.mul = _lib.MXV_ARG_ADD_OPS["min"], _lib.MXM_MUL_OPS["times"]
    bad = _lib.Semiring()
    bad.add, bad.mul = _lib.EWISE_OPS["plus"], _lib.EWISE_OPS["div"]
    fake = ctypes.c_void_p(0x1000)
    H = _lib.OSP_HOST
    calls = [lambda: L.osp_csr_mxv_arg(None, ctypes.byref(sr), xp, yp, ap, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv_arg(None, ctypes.byref(bad), xp, yp, ap, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv_arg(None, None, None, None, None, H, None),
             lambda: L.osp_csr_mxv_arg(None, ctypes.byref(sr), None, yp, ap, 99, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv_arg(fake, None, xp, yp, ap, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv_arg(fake, ctypes.byref(sr), xp, yp, None, H, ctypes.byref(stats)),
             lambda: L.osp_csr_mxv_arg(fake, ctypes.byref(sr), xp, None, None, H, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert stats.nnz_in == 77 and (y == 7.0).all() and (arg == 7).all()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_entries_exist_and_validate_before_they_need_a_gpu():
    assert callable(S.CsrResult.mxv_arg) and callable(graph.minimum_spanning_forest) and callable(graph.greedy_matching)
    res = object.__new__(S.CsrResult)   # (no handle: the names are checked before anything is touched)
    res._h, res.shape, res.dtype = None, (3, 3), np.float64
    for kw in ({"add": "plus"}, {"add": "first"}, {"add": "times"}, {"mul": "minus"}, {"mul": "div"}, {"add": "argmin"}):
        with pytest.raises(ValueError):
            res.mxv_arg(np.ones(3), space="host", **kw)
    with pytest.raises(ValueError):
        res.mxv_arg(np.ones(3), space="pinned")
    with pytest.raises(S.OspError):
        res.mxv_arg(None, "min", "times", space="host")                       # x may be None under "first" only
    with pytest.raises(S.OspError):
        res.mxv_arg(np.ones(3), out=np.zeros(3), values=False, space="host")  # positions only: there is no y to fill
    with pytest.raises(S.OspError):
        res.mxv_arg(np.ones(3), out_arg=np.zeros(3), space="host")            # out_arg is int64
    with pytest.raises(S.OspError):
        res.mxv_arg(np.ones(3), out_arg=np.zeros(4, np.int64), space="host")


@pytest.mark.parametrize("fn", [graph.minimum_spanning_forest, graph.greedy_matching])
def test_graph_functions_refuse_bad_arguments_without_a_gpu(fn):
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    with pytest.raises(TypeError):
        fn(r, c, dtype=np.int32)
    with pytest.raises(ValueError):
        fn(r, c, weights=[1.0, np.nan, 2.0])
    with pytest.raises(ValueError):
        fn(r, c, n=(1 << 24) + 1, dtype=np.float32)


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.minimum_spanning_forest(r, c), lambda: graph.greedy_matching(r, c, weights=[3.0, 1.0, 2.0])):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of mxv_arg ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("add", model.ADD_OPS)
def test_the_model_is_numpys_argmin_and_argmax_on_dense_rows(dt, add):
    """Random values without NaN and without zeros, rows of 0 to 5000 entries, repeated values among them: the dense row is
    filled with the identity, so numpy's first index of the extreme is the smallest column that holds it."""
    rng = np.random.default_rng(4)
    ncol = 6000
    lengths = [0, 1, 3, 64, 65, 700, 2049, 5000, 0, 17]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=k, replace=False)) for k in lengths]).astype(np.uint32)
    val = rng.integers(1, 40, len(col)).astype(dt)               # (many ties)
    x = rng.integers(1, 4, ncol).astype(dt)
    for mul in ("times", "plus", "first", "second"):
        y, arg, nlong, without = model.mxv_arg(rowptr, col, val, x, add, mul)
        prod = model.products(rowptr, col, val, x, mul)
        fill = np.inf if add == "min" else -np.inf
        for i, k in enumerate(lengths):
            if k == 0:
                assert arg[i] == -1 and y[i] == fill
                continue
            dense = np.full(ncol, fill, dt)
            dense[col[rowptr[i]:rowptr[i + 1]]] = prod[rowptr[i]:rowptr[i + 1]]
            assert arg[i] == (np.argmin(dense) if add == "min" else np.argmax(dense)), (mul, i)
            assert y[i] == dense[arg[i]]
        assert (nlong, without) == (2, 2) and arg.dtype == np.int64


def test_the_model_on_a_hand_written_matrix():
    """NaNs never win, the zeros tie (the earlier column wins whichever sign it has), a lone +inf under min has a position,
    an all-NaN row and an empty row have none."""
    nan, inf = np.nan, np.inf
    rows = [[(1, 3.0), (4, 1.0), (6, 1.0)],          # the minimum twice
            [(0, nan), (2, nan)],                    # all NaN
            [],                                      # empty
            [(2, 0.0), (5, -0.0), (7, 2.0)],         # +0.0 before -0.0
            [(2, -0.0), (5, 0.0), (7, -2.0)],        # -0.0 before +0.0
            [(3, nan), (8, inf)],                    # the identity of min as the only number
            [(3, -inf), (8, nan)]]                   # the identity of max as the only number
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], np.uint32)
    val = np.array([v for r in rows for _, v in r], np.float64)
    _, amin, _, wmin = model.mxv_arg(rowptr, col, val, None, "min", "first")
    _, amax, _, wmax = model.mxv_arg(rowptr, col, val, None, "max", "first")
    assert amin.tolist() == [4, -1, -1, 2, 7, 8, 3] and wmin == 2
    assert amax.tolist() == [1, -1, -1, 7, 2, 8, 3] and wmax == 2


# ---- the models of the graph functions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_kruskal_is_scipys_spanning_weight_and_networkxs_edges(name):
    n, r, c, w = GRAPHS[name]
    u, v, wt = model.simple_edges(n, r, c, w, "min", np.float64)
    fu, fv, fw = model.kruskal(n, u, v, wt)
    A = sp.csr_matrix((wt, (u, v)), shape=(n, n))
    T = minimum_spanning_tree(A)
    assert len(fu) == T.nnz and np.isclose(fw.sum(), T.sum(), rtol=1e-12, atol=0)
    assert (fu < fv).all() and np.array_equal(np.lexsort((fv, fu)), np.arange(len(fu)))
    # with distinct weights the forest is unique whatever the tie rule: networkx's edge set
    rng = np.random.default_rng(6)
    distinct = rng.permutation(len(u)).astype(np.float64) + 1.0
    du, dv, _ = model.kruskal(n, u, v, distinct)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from(zip(u.tolist(), v.tolist(), distinct.tolist()))
    want = sorted((min(a, b), max(a, b)) for a, b in nx.minimum_spanning_edges(G, data=False))
    assert list(zip(du.tolist(), dv.tolist())) == want


def _check_matching(n, u, v, mate):
    """valid (an involution on the matched vertices, every pair an edge) and maximal (no edge has both ends free)."""
    m = np.flatnonzero(mate >= 0)
    assert np.array_equal(mate[mate[m]], m) and (mate[m] != m).all()
    edges = set(zip(u.tolist(), v.tolist()))
    assert all((min(a, b), max(a, b)) in edges for a, b in zip(m.tolist(), mate[m].tolist()))
    assert not ((mate[u] < 0) & (mate[v] < 0)).any()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_matching_model_is_valid_and_maximal(name):
    n, r, c, w = GRAPHS[name]
    u, v, wt = model.simple_edges(n, r, c, w, "max", np.float64)
    mate = model.greedy_matching(n, u, v, wt)
    assert mate.dtype == np.int64 and mate.shape == (n,)
    _check_matching(n, u, v, mate)
    if name == "star":
        best = np.lexsort((v, u, -wt))[0]
        assert (mate >= 0).sum() == 2 and mate[u[best]] == v[best]


@pytest.mark.parametrize("seed", range(6))
def test_the_matching_model_has_half_the_optimal_weight_on_small_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(4, 13))
    m = int(rng.integers(n, 3 * n))
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    u, v, wt = model.simple_edges(n, r, c, rng.integers(1, 6, m).astype(np.float64), "max", np.float64)
    mate = model.greedy_matching(n, u, v, wt)
    _check_matching(n, u, v, mate)
    weight = {(a, b): x for a, b, x in zip(u.tolist(), v.tolist(), wt.tolist())}
    got = sum(weight[(a, int(mate[a]))] for a in range(n) if 0 <= a < mate[a])
    G = nx.Graph()
    G.add_weighted_edges_from(zip(u.tolist(), v.tolist(), wt.tolist()))
    best = sum(weight[(min(a, b), max(a, b))] for a, b in nx.max_weight_matching(G))
    print(f"n={n} edges={len(u)} greedy={got} optimum={best}")
    assert 2 * got >= best
