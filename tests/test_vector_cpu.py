"""CPU-side checks of the boundary between CSR results and dense vectors (include/outerspace_spgemm_vector.h) and of the graph
functions built on it: the symbols are exported and listed, both structs have the layout the C compiler gives them, null
arguments are argument errors, without a GPU the Python entries fail loudly, the model that judges the GPU
(tests/vector_model.py) follows the header's definition of R on hand-written inputs, and its graph functions agree with
networkx -- the Jaccard coefficients and the clustering coefficients as FLOATS: each is one correctly rounded division of two
exact integers, so there is no tolerance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import bfs_model
from tests import vector_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_vector.h")


def test_vector_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    assert declared
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.VECTOR_EXPORTS)
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS):
        assert not declared & set(other)
    # the enums' values are the binding's
    axes = dict((name.lower(), int(v)) for name, v in re.findall(r"OSP_AXIS_([A-Z]+)\s*=\s*(\d+)", hdr))
    assert axes == _lib.AXES and list(axes) == model.AXES
    ops = dict((name.lower(), int(v)) for name, v in re.findall(r"OSP_REDUCE_([A-Z]+)\s*=\s*(\d+)", hdr))
    assert ops == _lib.REDUCE_OPS and list(ops) == model.REDUCE_OPS
    assert int(re.search(r"#define\s+OSP_VECTOR_NONE\s+\((-?\d+)\)", hdr).group(1)) == _lib.VECTOR_NONE == -1
    assert set(_lib.VECTOR_APPLY_OPS) == set(model.APPLY_OPS) == set(_lib.EWISE_OPS) - {"first"}
    assert all(_lib.VECTOR_APPLY_OPS[k] == _lib.EWISE_OPS[k] for k in model.APPLY_OPS)
    assert '#include "outerspace_spgemm.h"' in hdr and '#include "outerspace_spgemm_ewise.h"' in hdr


@pytest.mark.parametrize("cname,struct", [("osp_vector_apply_t", _lib.VectorApply), ("osp_vector_stats_t", _lib.VectorStats)])
def test_vector_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_vector.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_vector_struct_dicts():
    assert set(_lib.VectorStats().as_dict()) == {"nnz_in", "nnz_out", "long_segments", "ms_total", "launches"}
    assert set(_lib.VectorApply().as_dict()) == {"row_op", "col_op"}


def test_vector_null_arguments_are_argument_errors():
    """Without a device there is no result to pass as `in`: a null `in`, alone and with the other pointers null
    (tests/test_gpu_vector.py passes the other null arguments with a real result)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.VectorStats()
    stats.nnz_in = 77
    vec = np.full(4, 5.0)
    keep = np.ones(4, np.uint8)
    ap = _lib.VectorApply()
    ap.row_op, ap.col_op = _lib.EWISE_OPS["plus"], _lib.VECTOR_NONE
    vp, kp = ctypes.c_void_p(vec.ctypes.data), ctypes.c_void_p(keep.ctypes.data)
    calls = [lambda: L.osp_csr_reduce(None, 0, 0, vp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_reduce(None, 0, 0, None, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_reduce(None, 0, 0, vp, _lib.OSP_HOST, None),
             lambda: L.osp_csr_apply_vectors(None, ctypes.byref(ap), vp, vp, _lib.OSP_HOST, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_apply_vectors(None, None, vp, vp, _lib.OSP_HOST, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_apply_vectors(None, ctypes.byref(ap), vp, vp, _lib.OSP_HOST, None, ctypes.byref(stats)),
             lambda: L.osp_csr_apply_vectors(None, ctypes.byref(ap), None, None, _lib.OSP_HOST, ctypes.byref(out), None),
             lambda: L.osp_csr_select_vertices(None, kp, kp, _lib.OSP_HOST, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_select_vertices(None, None, None, _lib.OSP_HOST, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_select_vertices(None, kp, kp, _lib.OSP_HOST, None, ctypes.byref(stats)),
             lambda: L.osp_csr_select_vertices(None, kp, kp, _lib.OSP_HOST, ctypes.byref(out), None)]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77 and np.all(vec == 5.0)


def test_vector_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.core_numbers(r, c), lambda: graph.k_core(r, c, k=2), lambda: graph.jaccard_similarity(r, c),
                 lambda: graph.local_clustering(r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


def test_k_below_zero_is_a_value_error():
    with pytest.raises(ValueError):
        graph.k_core(np.array([0]), np.array([1]), k=-1)
    with pytest.raises(ValueError):
        model.k_core(bfs_model.symmetric_adjacency([0], [1], 2), -1)


# ---- the model's rules on a hand-written matrix ------------------------------------------------------------------------------
# 3 x 6, rectangular; row 1 and columns 3 are empty
_ROWPTR = np.array([0, 5, 5, 9])
_COL = np.array([0, 1, 2, 4, 5, 0, 1, 2, 5], np.uint32)
_NCOL = 6


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _literal_R(e, op):
    """The header's definition of R, loop by loop, on numpy scalars of e's dtype."""
    def comb(a, b):
        with np.errstate(all="ignore"):
            return a + b if op == "plus" else (b if b < a else a) if op == "min" else (b if b > a else a)
    m = len(e)
    if m > 2048:
        return _literal_R(np.array([_literal_R(e[b:b + 2048], op) for b in range(0, m, 2048)], e.dtype), op)
    p = [model.identity(op, e.dtype)] * 64
    for lane in range(64):
        t = 0
        while lane + 64 * t < m:
            p[lane] = comb(p[lane], e[lane + 64 * t])
            t += 1
    for d in (32, 16, 8, 4, 2, 1):
        for lane in range(d):
            p[lane] = comb(p[lane], p[lane + d])
    return p[0]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_model_plus_equals_scipy_on_exact_values(dt):
    val = np.array([1, 2, -3, 0.5, 8, 4, 0.25, -16, 2], dt)
    A = sp.csr_matrix((val, _COL.astype(np.int64), _ROWPTR), shape=(3, _NCOL))
    rows, nlong = model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", "plus")
    assert nlong == 0 and rows.dtype == dt and np.array_equal(rows, np.asarray(A.sum(1)).ravel())
    cols, _ = model.reduce(_ROWPTR, _COL, val, _NCOL, "cols", "plus")
    assert np.array_equal(cols, np.asarray(A.sum(0)).ravel())
    assert model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", "count")[0].tolist() == [5, 0, 4]
    assert model.reduce(_ROWPTR, _COL, val, _NCOL, "cols", "count")[0].tolist() == [2, 2, 2, 0, 1, 2]
    assert model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", "min")[0].tolist() == [-3, np.inf, -16]
    assert model.reduce(_ROWPTR, _COL, val, _NCOL, "cols", "max")[0].tolist() == [4, 2, -3, -np.inf, 0.5, 8]
    # the column view keeps ascending row order
    colptr, r, v = model.column_view(_ROWPTR, _COL, val, _NCOL)
    assert colptr.tolist() == [0, 2, 4, 6, 6, 7, 9] and r.tolist() == [0, 2, 0, 2, 0, 2, 0, 0, 2]
    assert v.tolist() == [1, 4, 2, 0.25, -3, -16, 0.5, 8, 2]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("op", ["plus", "min", "max"])
@pytest.mark.parametrize("m", [0, 1, 3, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5])
def test_model_R_equals_the_literal_definition(m, op, dt):
    rng = np.random.default_rng(m + 7)
    e = (rng.standard_normal(m) * 10.0 ** rng.integers(-6, 6, m)).astype(dt)   # (sums whose order shows in the last bits)
    pad = rng.standard_normal(5).astype(dt)                                    # the segment does not start at 0
    got, nlong = model.reduce_segments(np.array([0, 5, 5 + m, 5 + m]), np.concatenate([pad, e]), op)
    assert nlong == (m > 2048)
    assert _bits(got[1:2]) == _bits(np.array([_literal_R(e, op)], dt))
    assert _bits(got[2:3]) == _bits(np.array([model.identity(op, dt)], dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_model_min_max_ignore_nan_and_plus_propagates_it(dt):
    nan = np.array([np.nan], dt)[0]
    val = np.array([nan, 1.0, -nan, 2.0, 3.0, nan, nan, nan, nan], dt)
    mn, mx = (model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", op)[0] for op in ("min", "max"))
    assert mn.tolist() == [1.0, np.inf, np.inf] and mx.tolist() == [3.0, -np.inf, -np.inf]   # (a row of NaNs alone: the identity)
    plus = model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", "plus")[0]
    assert np.isnan(plus).tolist() == [True, False, True] and plus[1] == 0.0
    cmn = model.reduce(_ROWPTR, _COL, val, _NCOL, "cols", "min")[0]
    assert cmn.tolist() == [np.inf, 1.0, np.inf, np.inf, 2.0, 3.0]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_model_zeros_and_empty_segments(dt):
    val = np.array([-0.0, 1.0, -1.0, -0.0, 5.0, -0.0, -0.0, -0.0, -0.0], dt)
    cols, _ = model.reduce(_ROWPTR, _COL, val, _NCOL, "cols", "plus")
    # column 4 holds a lone -0.0: +0.0 + -0.0; column 0 holds two; column 3 is empty
    assert cols.tolist() == [0.0, 1.0, -1.0, 0.0, 0.0, 5.0]
    assert np.signbit(cols).tolist() == [False, False, True, False, False, False]
    rows, _ = model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", "plus")
    assert rows.tolist() == [5.0, 0.0, 0.0] and not np.signbit(rows).any()
    for op, want in (("plus", 0.0), ("min", np.inf), ("max", -np.inf), ("count", 0.0)):
        got = model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", op)[0]
        assert got[1] == want and not (op in ("plus", "count") and np.signbit(got[1]))
        assert model.reduce(_ROWPTR, _COL, val, _NCOL, "cols", op)[0][3] == want
    # min and max return one entry's bits
    assert np.signbit(model.reduce(_ROWPTR, _COL, val, _NCOL, "rows", "max")[0][2])   # a row of -0.0 only


def test_model_apply_vectors_and_select_vertices_on_the_rectangle():
    val = np.arange(1.0, 10.0)
    x, y = np.array([10.0, 20.0, 30.0]), np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    got, computed = model.apply_vectors(_ROWPTR, _COL, val, x, "second", y, "plus")
    assert computed and got.tolist() == [11, 12, 13, 15, 16, 31, 32, 33, 36]
    got, computed = model.apply_vectors(_ROWPTR, _COL, val, x, "times", None, None)
    assert computed and got.tolist() == [10, 20, 30, 40, 50, 180, 210, 240, 270]
    got, computed = model.apply_vectors(_ROWPTR, _COL, val, None, None, y, "min")
    assert not computed and got.tolist() == [1, 2, 3, 4, 5, 1, 2, 3, 6]
    with pytest.raises(ValueError):
        model.apply_vectors(_ROWPTR, _COL, val)
    with pytest.raises(ValueError):
        model.apply_vectors(_ROWPTR, _COL, val, x, "first")
    rp, c, v = model.select_vertices(_ROWPTR, _COL, val, np.array([1, 1, 0], np.uint8), None)
    assert rp.tolist() == [0, 5, 5, 5] and c.tolist() == [0, 1, 2, 4, 5] and v.tolist() == [1, 2, 3, 4, 5]
    rp, c, v = model.select_vertices(_ROWPTR, _COL, val, None, np.array([0, 7, 0, 1, 0, 1], np.uint8))
    assert rp.tolist() == [0, 2, 2, 4] and c.tolist() == [1, 5, 1, 5] and v.tolist() == [2, 5, 7, 9]
    rp, c, v = model.select_vertices(_ROWPTR, _COL, val, np.array([0, 1, 1], np.uint8), np.array([0, 7, 0, 1, 0, 1], np.uint8))
    assert rp.tolist() == [0, 0, 0, 2] and c.tolist() == [1, 5] and v.tolist() == [7, 9]
    with pytest.raises(ValueError):
        model.select_vertices(_ROWPTR, _COL, val)


def test_model_reduces_many_short_rows_quickly():
    import time
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 5, 1 << 18)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    val = rng.standard_normal(ptr[-1])
    t0 = time.perf_counter()
    got, _ = model.reduce_segments(ptr, val, "plus")
    assert time.perf_counter() - t0 < 1.0
    some = np.flatnonzero(lens == 4)[:50]
    for s in some:   # lanes 0..3: (e0 + e2) + (e1 + e3)
        e = val[ptr[s]:ptr[s] + 4]
        assert got[s] == (e[0] + e[2]) + (e[1] + e[3])


# ---- the graph models against networkx -------------------------------------------------------------------------------------------
def _graphs():
    n, r, c, _ = gen.rmat_coo(8, 16, "g500", seed=1)
    yield "rmat8", n, r, c
    yield "path", 12, np.arange(11), np.arange(1, 12)
    yield ("k6pendant",) + model.clique_with_pendant(6)
    yield "edgeless", 5, np.zeros(0, np.int64), np.zeros(0, np.int64)


@pytest.mark.parametrize("name,n,rows,cols", list(_graphs()), ids=lambda x: x if isinstance(x, str) else "")
def test_model_core_numbers_equal_networkx(name, n, rows, cols):
    import networkx as nx
    adj = bfs_model.symmetric_adjacency(rows, cols, n)
    G = nx.from_scipy_sparse_array(adj)
    core, info = model.core_numbers(adj)
    want = nx.core_number(G)
    assert core.tolist() == [want[i] for i in range(n)]
    assert info["k_max"] == max(want.values()) and info["rounds"] == len(info["nnz_graph"])
    if name == "k6pendant":
        assert core.tolist() == [5] * 6 + [1] and info["k_max"] == 5
    if name == "path":
        assert core.tolist() == [1] * 12
    if name == "edgeless":
        assert core.tolist() == [0] * 5 and info["rounds"] == 0
    for k in (0, 1, 2, 3, info["k_max"], info["k_max"] + 1):
        u, v, _ = model.k_core(adj, k)
        assert list(zip(u.tolist(), v.tolist())) == sorted(tuple(sorted(e)) for e in nx.k_core(G, k).edges()), k


@pytest.mark.parametrize("name,n,rows,cols", list(_graphs()), ids=lambda x: x if isinstance(x, str) else "")
def test_model_jaccard_and_clustering_equal_networkx_as_floats(name, n, rows, cols):
    import networkx as nx
    adj = bfs_model.symmetric_adjacency(rows, cols, n)
    G = nx.from_scipy_sparse_array(adj)
    u, v, jac = model.jaccard_similarity(adj)
    assert len(u) == adj.nnz // 2
    want = {(a, b): p for a, b, p in nx.jaccard_coefficient(G, list(zip(u.tolist(), v.tolist())))}
    assert jac.tolist() == [want[e] for e in zip(u.tolist(), v.tolist())]
    cc = model.local_clustering(adj)
    wc = nx.clustering(G)
    assert cc.tolist() == [float(wc[i]) for i in range(n)]
    if name == "rmat8":
        assert (jac == 0).any() and (jac > 0).any() and (cc > 0).any()
    if name == "k6pendant":
        assert cc.tolist() == [20 / 30] + [1.0] * 5 + [0.0]
        assert (u[5], v[5], jac[5]) == (0, 6, 0.0) and jac[0] == 4 / 7 and jac[6] == 4 / 6   # the pendant edge; {0, 1}; {1, 2}
