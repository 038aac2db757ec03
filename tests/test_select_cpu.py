"""CPU-side checks of the entry filter's boundary (include/outerspace_spgemm_select.h) and of the truss functions built on
it: the symbol is exported and listed, both structs have the layout the C compiler gives them, null arguments are argument
errors, without a GPU the Python entries fail loudly, and the models that judge the GPU (tests/truss_model.py) follow the
filter's rules on a hand-written matrix and agree with networkx's k-truss."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import generators as gen
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import bfs_model
from tests import truss_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_select.h")


def test_select_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    assert declared
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.SELECT_EXPORTS)
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS):
        assert not declared & set(other)
    # the enum's values are the binding's
    ops = dict((name.lower(), int(v)) for name, v in re.findall(r"OSP_SELECT_([A-Z]+)\s*=\s*(\d+)", hdr))
    assert ops == _lib.SELECT_OPS and list(ops) == model.OPS


@pytest.mark.parametrize("cname,struct", [("osp_select_t", _lib.Select), ("osp_select_stats_t", _lib.SelectStats)])
def test_select_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_select.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_select_struct_dicts():
    assert set(_lib.SelectStats().as_dict()) == {"nnz_in", "nnz_out", "ms_total", "launches"}
    assert set(_lib.Select().as_dict()) == {"op", "fill", "threshold", "diag", "fill_value"}


def test_select_null_arguments_are_argument_errors():
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.SelectStats()
    stats.nnz_in = 77
    sel = _lib.Select()
    # without a device there is no result to pass as `in`: a null `in`, alone, with a null sel and with a null out
    # (tests/test_gpu_select.py passes a null sel and a null out with a real result)
    for args in ((None, ctypes.byref(sel), ctypes.byref(out), ctypes.byref(stats)),
                 (None, None, ctypes.byref(out), ctypes.byref(stats)),
                 (None, ctypes.byref(sel), None, ctypes.byref(stats)),
                 (None, ctypes.byref(sel), ctypes.byref(out), None)):
        assert L.osp_csr_select(*args) == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77


def test_truss_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.edge_support(r, c), lambda: graph.k_truss(r, c, k=3), lambda: graph.truss_decomposition(r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


def test_k_below_two_is_a_value_error():
    with pytest.raises(ValueError):
        graph.k_truss(np.array([0]), np.array([1]), k=1)
    with pytest.raises(ValueError):
        model.k_truss(bfs_model.symmetric_adjacency([0], [1], 2), 1)


# ---- the model's select rules on a hand-written matrix ---------------------------------------------------------------------
# 3 x 6, rectangular; row 1 is empty
_ROWPTR = np.array([0, 5, 5, 9])
_COL = np.array([0, 1, 2, 4, 5, 0, 1, 2, 5], np.uint32)


def _kept(op, val, **kw):
    rp, c, v = model.select(_ROWPTR, _COL, val, op, **kw)
    assert rp[0] == 0 and rp[-1] == len(c) == len(v) and v.dtype == val.dtype
    return rp.tolist(), c.tolist(), v


def test_model_select_nan_fails_every_comparison_but_ne():
    val = np.array([np.nan, 1.0, -np.nan, 2.0, 3.0, 0.5, np.nan, 2.0, -1.0])
    n_nan = int(np.isnan(val).sum())
    for op in ("lt", "le", "gt", "ge", "eq"):
        for thr in (2.0, np.nan, np.inf, -np.inf):
            _, _, v = _kept(op, val, threshold=thr)
            assert not np.isnan(v).any()
            if np.isnan(thr):
                assert len(v) == 0
    for thr in (2.0, np.nan):
        _, _, v = _kept("ne", val, threshold=thr)
        assert np.isnan(v).sum() == n_nan
    assert len(_kept("ne", val, threshold=np.nan)[2]) == len(val)
    # lt and ge partition the NaN-free entries only; eq and ne partition everything
    assert len(_kept("lt", val, threshold=2.0)[2]) + len(_kept("ge", val, threshold=2.0)[2]) == len(val) - n_nan
    assert len(_kept("eq", val, threshold=2.0)[2]) + len(_kept("ne", val, threshold=2.0)[2]) == len(val)
    assert _kept("ge", val, threshold=2.0)[:2] == ([0, 2, 2, 3], [4, 5, 2])
    assert _kept("le", val, threshold=np.inf)[1] == [1, 4, 5, 0, 2, 5]


def test_model_select_zeros_and_fill():
    val = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 5e-324, -5e-324, 0.0])
    rp, c, v = _kept("eq", val, threshold=0.0)
    assert c == [0, 1, 5, 0, 5] and np.signbit(v).tolist() == [False, True, False, True, False]     # -0.0 == +0.0, bits kept
    assert _kept("eq", val, threshold=-0.0)[1] == c
    assert _kept("gt", val, threshold=0.0)[1] == [2, 1] and _kept("lt", val, threshold=-0.0)[1] == [4, 2]   # denormals are numbers
    rp, c, v = _kept("ge", val, threshold=0.0, fill=1.0)
    assert v.tolist() == [1.0] * 7 and rp == [0, 4, 4, 7]
    assert _kept("ge", val.astype(np.float32), threshold=0.0, fill=0.1)[2].tolist() == [float(np.float32(0.1))] * 8   # (+-5e-324 round to +-0 in f32: all but the -1)


def test_model_select_threshold_that_is_no_f32():
    # 0.1f = 0.100000001490116...: above the double 0.1, below the double 0.1 + 2e-9
    val = np.array([0.1] * 9, np.float32)
    assert len(_kept("gt", val, threshold=0.1)[2]) == 9 and len(_kept("eq", val, threshold=0.1)[2]) == 0
    assert len(_kept("lt", val, threshold=0.1 + 2e-9)[2]) == 9
    assert len(_kept("eq", val, threshold=float(np.float32(0.1)))[2]) == 9
    assert len(_kept("le", val.astype(np.float64), threshold=0.1)[2]) == 0   # (the widened f32, not 0.1)


def test_model_select_positions_on_a_rectangle():
    val = np.arange(9.0)
    assert _kept("diag", val)[1] == [0, 2] and _kept("diag", val)[0] == [0, 1, 1, 2]
    assert _kept("offdiag", val)[1] == [1, 2, 4, 5, 0, 1, 5]
    assert _kept("tril", val)[1] == [0, 0, 1, 2] and _kept("triu", val, diag=1)[1] == [1, 2, 4, 5, 5]
    assert _kept("tril", val, diag=-1)[1] == [0, 1] and _kept("triu", val, diag=-2)[1] == [0, 1, 2, 4, 5, 0, 1, 2, 5]
    assert _kept("diag", val, diag=-2)[1] == [0] and _kept("diag", val, diag=3)[1] == [5]     # row 2 col 0; row 2 col 5
    assert _kept("diag", val, diag=5)[1] == [5] and _kept("diag", val, diag=6)[1] == []      # row 0 col 5; beyond the matrix
    for d in (-(1 << 63), -(1 << 40), -7, 7, 1 << 40, (1 << 63) - 1):
        far_low = d < 0
        assert len(_kept("tril", val, diag=d)[1]) == (0 if far_low else 9)
        assert len(_kept("triu", val, diag=d)[1]) == (9 if far_low else 0)
        assert len(_kept("diag", val, diag=d)[1]) == 0 and len(_kept("offdiag", val, diag=d)[1]) == 9
    for d in range(-4, 8):
        assert len(_kept("tril", val, diag=d)[1]) + len(_kept("triu", val, diag=d + 1)[1]) == 9
        assert len(_kept("diag", val, diag=d)[1]) + len(_kept("offdiag", val, diag=d)[1]) == 9


# ---- the truss models against networkx ---------------------------------------------------------------------------------------
def _nx_truss_edges(G, k):
    import networkx as nx
    return sorted(tuple(sorted(e)) for e in nx.k_truss(G, k).edges())


def _graphs():
    for scale in (8, 10):
        n, r, c, _ = gen.rmat_coo(scale, 16, "g500", seed=1)
        yield f"rmat{scale}", n, r, c
    yield ("k9path",) + model.clique_with_path(9, 21)


# edges, and per k in (3, 4, 8, 16) (edges of the truss, rounds): DESIGN.md section 12's table
_EXPECTED = {"rmat8": (2101, {3: (2049, 1), 4: (1949, 2), 8: (1397, 5), 16: (468, 6)}, 16, 56),
             "rmat10": (10502, {3: (10167, 1), 4: (9626, 3), 8: (7686, 7), 16: (4281, 7)}, 28, 131)}


@pytest.mark.parametrize("name,n,rows,cols", list(_graphs()), ids=lambda x: x if isinstance(x, str) else "")
def test_model_k_truss_equals_networkx(name, n, rows, cols):
    import networkx as nx
    adj = bfs_model.symmetric_adjacency(rows, cols, n)
    G = nx.from_scipy_sparse_array(adj)
    for k in (3, 4, 8, 16):
        u, v, info = model.k_truss(adj, k)
        assert list(zip(u.tolist(), v.tolist())) == _nx_truss_edges(G, k), k
        assert info["rounds"] == len(info["nnz_graph"]) == len(info["nnz_support"]) == len(info["nnz_kept"]) >= 1
        assert info["nnz_kept"][-1] == 2 * len(u) and info["nnz_graph"][0] == adj.nnz
        if name in _EXPECTED:
            assert (len(u), info["rounds"]) == _EXPECTED[name][1][k]
    if name in _EXPECTED:
        assert adj.nnz // 2 == _EXPECTED[name][0]
    u, v, info = model.k_truss(adj, 2)
    assert len(u) == adj.nnz // 2 and info["rounds"] == 0
    if name == "k9path":
        u, v, info = model.k_truss(adj, 9)
        cr, cc = np.triu_indices(9, 1)
        assert len(u) == 36 and np.array_equal(u, cr) and np.array_equal(v, cc)
        assert len(model.k_truss(adj, 10)[0]) == 0
        assert len(model.k_truss(adj, 3)[0]) == 36 and len(model.k_truss(adj, 2)[0]) == 36 + 21


@pytest.mark.parametrize("name,n,rows,cols", list(_graphs()), ids=lambda x: x if isinstance(x, str) else "")
def test_model_trussness_equals_networkx(name, n, rows, cols):
    import networkx as nx
    adj = bfs_model.symmetric_adjacency(rows, cols, n)
    G = nx.from_scipy_sparse_array(adj)
    u, v, trussness, info = model.truss_decomposition(adj)
    assert len(u) == adj.nnz // 2 and trussness.min() >= 2 and trussness.max() == info["k_max"]
    edges = np.array(list(zip(u.tolist(), v.tolist())))
    for k in range(2, info["k_max"] + 2):
        assert [tuple(e) for e in edges[trussness >= k].tolist()] == _nx_truss_edges(G, k), k
    if name in _EXPECTED:
        assert (info["k_max"], info["products"]) == _EXPECTED[name][2:]
    if name == "k9path":
        assert info["k_max"] == 9 and sorted(np.unique(trussness).tolist()) == [2, 9]


def test_model_edge_support_counts_triangles():
    import networkx as nx
    n, r, c, _ = gen.rmat_coo(10, 16, "g500", seed=1)
    adj = bfs_model.symmetric_adjacency(r, c, n)
    u, v, support = model.edge_support(adj)
    assert support.sum() // 3 == sum(nx.triangles(nx.from_scipy_sparse_array(adj)).values()) // 3 == 75692
    assert (support == 0).any() and len(u) == 10502
    # the masked product's formulation gives the same numbers
    S = model._supports(adj)
    su, sv, sval = model._upper(S)
    full = np.zeros(len(u), np.int64)
    full[np.searchsorted(u * n + v, su * n + sv)] = sval.astype(np.int64)
    assert np.array_equal(full, support)
