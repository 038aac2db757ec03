"""CPU-side checks of the submatrix of a result (include/outerspace_spgemm_extract.h) and of what is built on it: the
symbol is exported and listed, both structs have the layout the C compiler gives them, null and illegal arguments are
argument errors that leave the outputs alone, the Python entries exist, validate ``space`` and fail loudly without a GPU,
and the models that judge the GPU (tests/extract_model.py) equal things that share nothing with them: scipy's
``A[I][:, J]``, networkx's ``subgraph`` and ``ego_graph`` and scipy's components."""
import ctypes
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
from tests import extract_model as model
from tests import mxv_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_extract.h")
GRAPHS = {name: g for name, g in mxv_model.component_graphs().items() if name in ("rmat8", "rmat10")}


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_extract_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.EXTRACT_EXPORTS) == {"osp_csr_extract"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS, _lib.MXV_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm.h"' in hdr


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_extract_t", _lib.Extract), ("osp_extract_stats_t", _lib.ExtractStats)])
def test_extract_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_extract.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    if struct is _lib.ExtractStats:
        assert set(struct().as_dict()) == {"nnz_in", "nnz_gathered", "nnz_out", "ms_total", "launches", "readbacks"}


def test_extract_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in` (whatever else is wrong with it), and a fake
    `in` with a null ex or out (the null checks come before `in` is touched; tests/test_gpu_extract.py passes the other bad
    arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.ExtractStats()
    stats.nnz_in = 77
    rows = np.array([0, 1], np.uint32)
    ok = _lib.Extract()
    ok.rows, ok.n_rows, ok.space = rows.ctypes.data, 2, _lib.OSP_HOST
    bad_space = _lib.Extract()
    bad_space.space = 99
    bad_word = _lib.Extract()
    bad_word.reserved[6] = 1
    huge = _lib.Extract()
    huge.rows, huge.n_rows, huge.space = rows.ctypes.data, 1 << 32, _lib.OSP_HOST
    fake = ctypes.c_void_p(0x1000)
    calls = [lambda: L.osp_csr_extract(None, ctypes.byref(ok), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_extract(None, ctypes.byref(bad_space), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_extract(None, ctypes.byref(bad_word), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_extract(None, ctypes.byref(huge), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_extract(None, None, None, None),
             lambda: L.osp_csr_extract(fake, None, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_extract(fake, ctypes.byref(ok), None, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_entries_exist_and_validate_space():
    assert callable(S.CsrResult.extract) and callable(S.CsrResult.permute)
    assert callable(graph.induced_subgraph) and callable(graph.ego_network) and callable(graph.largest_component)
    res = object.__new__(S.CsrResult)   # (no handle: the arguments are checked before anything is touched)
    res._h, res.shape, res.dtype, res.nnz = None, (3, 3), np.float64, 0
    for kw in ({"rows": [0]}, {"cols": [0]}, {}):
        with pytest.raises(ValueError):
            res.extract(space="pinned", **kw)
    with pytest.raises(ValueError):
        res.permute([0, 1, 2], space="pinned")
    for bad in ([-1], [1 << 32], [0.5], [[0, 1]]):
        with pytest.raises(S.OspError) as ei:
            res.extract(rows=bad, space="host")
        assert ei.value.status == _lib.ERR_ARG
    res.shape = (3, 4)
    with pytest.raises(S.OspError) as ei:
        res.permute([0, 1, 2], space="host")
    assert ei.value.status == _lib.ERR_DIM


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.induced_subgraph(r, c, 3, [0, 1]), lambda: graph.induced_subgraph(r, c, 3, [0, 1], directed=True),
                 lambda: graph.ego_network(r, c, 3, 0, 1), lambda: graph.largest_component(r, c, 3)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of extract --------------------------------------------------------------------------------------------------------
def _random_matrix(dt, seed, ncol=6000):
    """Rows of 0 to 5000 entries, the empty ones first, last and in the middle."""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, 3, 64, 65, 700, 0, 2048, 2049, 5000, 17, 0]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=k, replace=False)) for k in lengths]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    val[::5] = 0.0                                               # explicit zeros are entries
    return ncol, (rowptr, col, val)


def _scipy_extract(csr, ncol, rows, cols):
    """scipy's A[I][:, J] with sorted indices, on the PATTERN'S positions (the values are looked up, so that an explicit zero
    stays an entry): (rowptr, col, positions in csr's arrays)."""
    rowptr, col, _ = csr
    M = len(rowptr) - 1
    P = sp.csr_matrix((np.arange(1, len(col) + 1, dtype=np.float64), col.astype(np.int64), rowptr), shape=(M, ncol))
    I = np.arange(M) if rows is None else np.asarray(rows, np.int64)
    J = np.arange(ncol) if cols is None else np.asarray(cols, np.int64)
    sub = P[I] if len(I) else sp.csr_matrix((0, ncol))
    sub = sub[:, J] if len(J) else sp.csr_matrix((len(I), 0))
    sub = sp.csr_matrix(sub)
    sub.sort_indices()
    return sub.indptr.astype(np.int64), sub.indices.astype(np.uint32), sub.data.astype(np.int64) - 1


def _lists(M, ncol, rng):
    rows = {"none": None, "identity": np.arange(M), "reversed": np.arange(M)[::-1], "twice": np.repeat(np.arange(M), 2),
            "random with duplicates": rng.integers(0, M, 3 * M), "empty": np.zeros(0, np.int64), "one": np.array([9])}
    cols = {"none": None, "all": np.arange(ncol), "half": np.sort(rng.choice(ncol, ncol // 2, replace=False)),
            "every 64th": np.arange(0, ncol, 64), "first": np.array([0]), "last": np.array([ncol - 1]), "empty": np.zeros(0, np.int64)}
    return rows, cols


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_is_scipys_fancy_indexing(dt):
    ncol, csr = _random_matrix(dt, 3)
    M = len(csr[0]) - 1
    rows, cols = _lists(M, ncol, np.random.default_rng(4))
    for rn, I in rows.items():
        for cn, J in cols.items():
            (rowptr, col, val), st = model.extract(*csr, ncol, I, J)
            wp, wc, wpos = _scipy_extract(csr, ncol, I, J)
            assert np.array_equal(rowptr, wp) and np.array_equal(col, wc), (rn, cn)
            assert val.dtype == dt and np.array_equal(_bits(val), _bits(csr[2][wpos])), (rn, cn)
            assert st["nnz_out"] == len(wc) and st["nnz_in"] == len(csr[1])
            gathered = len(csr[1]) if I is None else int(np.diff(csr[0])[I].sum()) if len(I) and (J is None or len(J)) else 0
            assert st["nnz_gathered"] == gathered, (rn, cn)
            empty = len(wp) == 1 or (J is not None and len(J) == 0)
            want_rb = 0 if empty or (I is None and J is None) else 1 if I is None or J is None or gathered == 0 else 2
            assert st["readbacks"] == want_rb, (rn, cn)


def test_the_model_refuses_bad_lists_but_reads_none_in_an_empty_shape():
    ncol, csr = _random_matrix(np.float64, 5)
    M = len(csr[0]) - 1
    for kw in ({"rows": [M]}, {"cols": [ncol]}, {"cols": [5, 4]}, {"cols": [5, 5]}, {"rows": [0, M], "cols": [1, 2]}):
        with pytest.raises(ValueError):
            model.extract(*csr, ncol, **kw)
    assert model.extract(*csr, ncol, rows=[M], cols=[])[1]["nnz_out"] == 0
    assert model.extract(*csr, ncol, rows=[], cols=[ncol])[0][0].tolist() == [0]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_composed_path_is_scipys_on_general_column_lists(dt):
    ncol, csr = _random_matrix(dt, 6, ncol=5200)
    M = len(csr[0]) - 1
    rng = np.random.default_rng(7)
    cases = {"permutation": (None, rng.permutation(ncol)), "reversed": (np.arange(M)[::-1], np.arange(ncol)[::-1]),
             "duplicates": (rng.integers(0, M, 20), np.concatenate([[7, 7, 7], rng.integers(0, ncol, 900), [7]])),
             "ascending": (rng.integers(0, M, 20), np.arange(0, ncol, 3))}
    for name, (I, J) in cases.items():
        rowptr, col, val = model.extract_any(*csr, ncol, I, J)
        # scipy keeps a repeated column's copies in list order as well: its indices are the list positions
        wp, wc, wpos = _scipy_extract(csr, ncol, I, J)
        assert np.array_equal(rowptr, wp) and np.array_equal(col, wc), name
        assert np.array_equal(_bits(val), _bits(csr[2][wpos])), name


# ---- the models of the graph functions -------------------------------------------------------------------------------------------
def _nx_graph(n, rows, cols):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(rows, cols) if a != b)
    return G


def _nx_edges(H, vertices):
    """The edges of the networkx graph H on ``vertices``, relabelled by position in ``vertices``, u < v, ascending."""
    new = {int(v): i for i, v in enumerate(vertices)}
    e = sorted((min(new[a], new[b]), max(new[a], new[b])) for a, b in H.edges())
    return np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_induced_subgraph_model_is_networkx(name):
    n, r, c = GRAPHS[name]
    G = _nx_graph(n, r, c)
    rng = np.random.default_rng(8)
    for vertices in (np.sort(rng.choice(n, n // 2, replace=False)), rng.permutation(n)[:n // 3], np.arange(n), np.zeros(0, np.int64)):
        u, v = model.induced_subgraph(n, r, c, vertices)
        wu, wv = _nx_edges(G.subgraph(vertices.tolist()), vertices)
        assert np.array_equal(u, wu) and np.array_equal(v, wv)
    with pytest.raises(ValueError):
        model.induced_subgraph(n, r, c, [1, 2, 1])
    # directed: every edge u -> v, self loops kept
    D = nx.DiGraph()
    D.add_edges_from(zip(r.tolist(), c.tolist()))
    vertices = rng.permutation(n)
    u, v = model.induced_subgraph(n, r, c, vertices, directed=True)
    new = {int(x): i for i, x in enumerate(vertices)}
    want = sorted((new[a], new[b]) for a, b in D.subgraph(vertices.tolist()).edges())
    assert list(zip(u.tolist(), v.tolist())) == want and any(a == b for a, b in want) == bool((r == c).any())


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_ego_network_model_is_networkx(name, radius):
    n, r, c = GRAPHS[name]
    G = _nx_graph(n, r, c)
    deg = np.bincount(np.concatenate([r[r != c], c[r != c]]), minlength=n)
    for center in (int(np.argmax(deg)), int(np.flatnonzero(deg == deg[deg > 0].min())[0]), int(np.flatnonzero(deg == 0)[0])):
        vertices, u, v = model.ego_network(n, r, c, center, radius)
        E = nx.ego_graph(G, center, radius=radius)
        assert vertices.tolist() == sorted(E.nodes())
        wu, wv = _nx_edges(E, vertices)
        assert np.array_equal(u, wu) and np.array_equal(v, wv)
    assert model.ego_network(n, r, c, 3, 0)[0].tolist() == [3]


@pytest.mark.parametrize("name", list(mxv_model.component_graphs()))
def test_the_largest_component_model_is_scipys_components(name):
    n, r, c = mxv_model.component_graphs()[name]
    vertices, u, v = model.largest_component(n, r, c)
    A = sp.csr_matrix((np.ones(len(r)), (np.asarray(r), np.asarray(c))), shape=(n, n))
    ncomp, label = connected_components(A, directed=False)
    sizes = np.bincount(label, minlength=ncomp)
    # the largest; on a tie the one whose smallest vertex is smallest (scipy numbers components by their first vertex)
    best = int(np.flatnonzero(sizes == sizes.max())[0])
    want = np.flatnonzero(label == best)
    assert np.array_equal(vertices, want)
    wu, wv = _nx_edges(_nx_graph(n, r, c).subgraph(want.tolist()), want)
    assert np.array_equal(u, wu) and np.array_equal(v, wv)
    if name == "two cliques":
        assert vertices.tolist() == list(range(6)) and len(u) == 15       # a tie: the clique of the smaller ids
