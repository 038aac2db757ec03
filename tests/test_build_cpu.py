"""CPU-side checks of the build of a result from a COO list (include/outerspace_spgemm_build.h) and of what is built on
it: the symbol is exported and listed, both structs have the layout the C compiler gives them, null and illegal arguments
are argument errors that leave the outputs alone, the Python entries exist, validate ``space`` and ``dup`` and fail loudly
without a GPU, and the models that judge the GPU (tests/build_model.py) equal things that share nothing with them: scipy's
``coo_matrix.tocsr``, numpy's ``minimum.at`` / ``maximum.at``, a dict, the arrays of ``symmetric_adjacency`` and
``weighted_adjacency``, scipy's ``csgraph.laplacian`` and networkx's ``incidence_matrix`` and ``line_graph``."""
import ctypes
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import laplacian as scipy_laplacian

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import build_model as model
from tests import mxv_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_build.h")
_ALL = mxv_model.component_graphs()
GRAPHS = {name: _ALL[name] for name in ("rmat8", "rmat10", "path", "two cliques")}
GRAPHS["edgeless"] = (5, np.zeros(0, np.int64), np.zeros(0, np.int64))
GRAPHS["no vertex"] = (0, np.zeros(0, np.int64), np.zeros(0, np.int64))
bits = model.bits


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_build_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.BUILD_EXPORTS) == {"osp_csr_build"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS, _lib.MXV_EXPORTS, _lib.EXTRACT_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm.h"' in hdr
    enum = re.search(r"typedef enum \{(.*?)\} osp_dup_op_t;", hdr, flags=re.S).group(1)
    names = re.findall(r"OSP_DUP_([A-Z]+)", enum)
    assert [n.lower() for n in names] == list(model.DUP_OPS) == sorted(_lib.DUP_OPS, key=_lib.DUP_OPS.get)
    assert sorted(_lib.DUP_OPS.values()) == list(range(7))


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_build_t", _lib.Build), ("osp_build_stats_t", _lib.BuildStats)])
def test_build_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_build.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    if struct is _lib.BuildStats:
        assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "long_runs", "ms_total", "launches", "readbacks"}


def _ok_build(idx):
    b = _lib.Build()
    b.M, b.N, b.nnz = 4, 4, 2
    b.rows = b.cols = idx.ctypes.data
    b.dtype, b.space, b.dup = _lib.OSP_F64, _lib.OSP_HOST, _lib.DUP_OPS["plus"]
    return b


def test_build_null_and_illegal_arguments_are_argument_errors():
    """Without a device there is no context to pass: every call with a null context (whatever else is wrong with it), and a
    fake context with a null or illegal description (all of these are refused before the context is touched;
    tests/test_gpu_build.py passes them with a real one)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.BuildStats()
    stats.nnz_in = 77
    idx = np.array([0, 1], np.uint32)
    bad = {}
    for name, change in {"dtype": lambda b: setattr(b, "dtype", 2), "negative dtype": lambda b: setattr(b, "dtype", -1),
                         "space": lambda b: setattr(b, "space", 99), "dup": lambda b: setattr(b, "dup", 7),
                         "negative dup": lambda b: setattr(b, "dup", -1), "reserved": lambda b: b.reserved.__setitem__(6, 1),
                         "first reserved": lambda b: b.reserved.__setitem__(0, 1), "M": lambda b: setattr(b, "M", 0xffffffff),
                         "N": lambda b: setattr(b, "N", 1 << 32), "nnz": lambda b: setattr(b, "nnz", 0xffffffff),
                         "rows": lambda b: setattr(b, "rows", None), "cols": lambda b: setattr(b, "cols", None)}.items():
        bad[name] = _ok_build(idx)
        change(bad[name])
    ok = _ok_build(idx)
    fake = ctypes.c_void_p(0x1000)
    calls = {"null ctx": lambda: L.osp_csr_build(None, ctypes.byref(ok), ctypes.byref(out), ctypes.byref(stats)),
             "all null": lambda: L.osp_csr_build(None, None, None, None),
             "null b": lambda: L.osp_csr_build(fake, None, ctypes.byref(out), ctypes.byref(stats)),
             "null out": lambda: L.osp_csr_build(fake, ctypes.byref(ok), None, ctypes.byref(stats))}
    for name, b in bad.items():
        calls["null ctx, bad " + name] = lambda b=b: L.osp_csr_build(None, ctypes.byref(b), ctypes.byref(out), ctypes.byref(stats))
        calls["bad " + name] = lambda b=b: L.osp_csr_build(fake, ctypes.byref(b), ctypes.byref(out), ctypes.byref(stats))
        calls["bad " + name + ", no stats"] = lambda b=b: L.osp_csr_build(fake, ctypes.byref(b), ctypes.byref(out), None)
    for name, call in calls.items():
        assert call() == _lib.ERR_ARG, name
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77, name


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_entries_exist_and_validate_space_and_dup():
    assert callable(S.Context.build)
    for f in (graph.adjacency_matrix, graph.laplacian, graph.incidence_matrix, graph.line_graph):
        assert callable(f)
    ctx = object.__new__(S.Context)   # (no handle: the arguments are checked before anything is touched)
    ctx._h = None
    with pytest.raises(ValueError):
        ctx.build(3, 3, [0], [1], space="pinned")
    with pytest.raises(ValueError):
        ctx.build(3, 3, [0], [1], dup="sum")
    with pytest.raises(ValueError):
        ctx.build(3, 3, object(), object(), dup="sum", space="device")
    with pytest.raises(TypeError):
        ctx.build(3, 3, [0], [1], dtype=np.float16)
    for kw in ({"rows": [-1], "cols": [0]}, {"rows": [0], "cols": [1 << 32]}, {"rows": [0.5], "cols": [0]}, {"rows": [0, 1], "cols": [0]},
               {"rows": [0, 1], "cols": [0, 1], "vals": [1.0]}):
        with pytest.raises(S.OspError) as ei:
            ctx.build(3, 3, **kw)
        assert ei.value.status == _lib.ERR_ARG
    ctx._h = None   # (nothing to destroy)


def test_graph_builders_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.adjacency_matrix(r, c, 3), lambda: graph.laplacian(r, c, 3), lambda: graph.incidence_matrix(r, c, 3),
                 lambda: graph.line_graph(r, c, 3), lambda: S.Context().build(3, 3, r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of build ----------------------------------------------------------------------------------------------------------
def _list(seed, M=40, N=70, nnz=3000, integer=False):
    """A shuffled list with many repeats, a run longer than the wave path's threshold among them."""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(1, M - 1, nnz), rng.integers(0, N, nnz)
    r[:model.LONG_RUN + 9], c[:model.LONG_RUN + 9] = 7, 11
    v = rng.integers(-50, 50, nnz).astype(np.float64) if integer else rng.standard_normal(nnz)
    p = rng.permutation(nnz)
    return M, N, r[p], c[p], v[p]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_plus_of_integers_is_scipys_tocsr(dt):
    M, N, r, c, v = _list(1, integer=True)
    (rowptr, col, val), st, lay = model.build(M, N, r, c, v, "plus", dt)
    want = sp.coo_matrix((v, (r, c)), shape=(M, N)).tocsr()   # (sums duplicates; integers: exact in any order)
    want.sort_indices()
    # scipy may drop nothing: explicit zero sums stay entries in tocsr
    assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices)
    assert val.dtype == dt and np.array_equal(val, want.data.astype(dt))
    assert rowptr[1] == 0 and rowptr[-1] == rowptr[-2]           # the first and the last row are empty
    assert st["nnz_in"] == len(r) and st["nnz_out"] == want.nnz and st["readbacks"] == 2
    assert st["long_runs"] == int((lay["length"] > model.LONG_RUN).sum()) >= 1
    assert np.array_equal(np.sort(lay["order"]), np.arange(len(r))) and lay["length"].sum() == len(r)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("op", ["min", "max"])
def test_min_and_max_are_numpys_ufunc_at(op, dt):
    M, N, r, c, v = _list(2)
    v = v.astype(dt)
    (rowptr, col, val), st, _ = model.build(M, N, r, c, v, op, dt)
    dense = np.full((M, N), np.inf if op == "min" else -np.inf, dt)
    (np.minimum if op == "min" else np.maximum).at(dense, (r, c), v)
    rr = np.repeat(np.arange(M), np.diff(rowptr))
    assert np.array_equal(val, dense[rr, col]) and len(col) == np.isfinite(dense).sum()
    assert st["nnz_out"] == len(col)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_first_last_and_count_are_a_dict(dt):
    M, N, r, c, v = _list(3)
    v = v.astype(dt)
    seen = {}
    for t, key in enumerate(zip(r.tolist(), c.tolist())):
        seen.setdefault(key, []).append(t)
    keys = sorted(seen)
    for op, pick in (("first", lambda ts: v[ts[0]]), ("last", lambda ts: v[ts[-1]]), ("count", lambda ts: dt(len(ts)))):
        (rowptr, col, val), st, _ = model.build(M, N, r, c, v, op, dt)
        rr = np.repeat(np.arange(M), np.diff(rowptr))
        assert list(zip(rr.tolist(), col.tolist())) == keys
        assert np.array_equal(bits(val), bits(np.array([pick(seen[k]) for k in keys], dt))), op
        assert st["long_runs"] == 0 and st["readbacks"] == 1
    # without values: every value is 1
    for op in model.DUP_OPS[1:]:
        val = model.build(M, N, r, c, None, op, dt)[0][2]
        want = [len(seen[k]) if op in ("plus", "count") else 1 for k in keys]
        assert np.array_equal(val, np.array(want, dt)), op


def test_list_order_decides_the_bits_of_plus():
    """Two of the three orders of 1e16, 1.0, -1e16 lose the 1.0: a sum that ignored list order could not give both."""
    got = {}
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2)):
        v = np.array([1e16, 1.0, -1e16])[list(order)]
        (_, _, val), _, _ = model.build(2, 2, [1, 1, 1], [0, 0, 0], v, "plus", np.float64)
        got[order] = float(val[0])
    assert got == {(0, 1, 2): 0.0, (0, 2, 1): 1.0, (1, 0, 2): 0.0}
    # the same list, shuffled around OTHER coordinates: the run's own order is what counts
    v = np.array([5.0, 1e16, 7.0, 1.0, 9.0, -1e16])
    (_, col, val), _, _ = model.build(2, 3, [0, 1, 1, 1, 0, 1], [2, 0, 1, 0, 1, 0], v, "plus", np.float64)
    assert col.tolist() == [1, 2, 0, 1] and val.tolist() == [9.0, 5.0, 0.0, 7.0]


def test_single_entries_keep_their_bits_and_min_max_follow_ewise():
    nan1, nan2 = np.array([0x7ff8000000000123, 0xfff0000000000456], np.uint64).view(np.float64)
    v = np.array([nan1, -0.0, 5e-324, np.inf, 0.0])
    (_, _, val), _, _ = model.build(1, 5, [0] * 5, [0, 1, 2, 3, 4], v, "plus", np.float64)
    assert np.array_equal(bits(val), bits(v))
    # a NaN first stays (nothing compares below or above it), a NaN in the middle never replaces acc
    for op in ("min", "max"):
        assert bits(model.build(1, 1, [0] * 3, [0] * 3, [nan2, 1.0, 2.0], op)[0][2])[0] == bits(np.array([nan2]))[0]
        assert model.build(1, 1, [0] * 3, [0] * 3, [1.0, nan1, 2.0], op)[0][2][0] == (1.0 if op == "min" else 2.0)
        # -0.0 and +0.0 compare equal: the earlier one stays
        assert bits(model.build(1, 1, [0, 0], [0, 0], [-0.0, 0.0], op)[0][2])[0] == 1 << 63
        assert bits(model.build(1, 1, [0, 0], [0, 0], [0.0, -0.0], op)[0][2])[0] == 0


def test_the_model_refuses_what_the_library_refuses():
    for kw, status in (({"rows": [3], "cols": [0]}, model.ERR_RANGE), ({"rows": [0], "cols": [4]}, model.ERR_RANGE),
                       ({"rows": [0xffffffff], "cols": [0]}, model.ERR_RANGE), ({"rows": [1, 1], "cols": [2, 2], "dup": "error"}, model.ERR_DUPLICATE),
                       ({"rows": [1, 1, 3], "cols": [2, 2, 0], "dup": "error"}, model.ERR_RANGE), ({"rows": [1], "cols": [2], "dup": "sum"}, model.ERR_ARG)):
        with pytest.raises(model.BuildError) as ei:
            model.build(3, 4, **kw)
        assert ei.value.status == status
    assert model.build(3, 4, [1, 2], [2, 2], dup="error")[1]["nnz_out"] == 2
    for shape in ((0, 4), (3, 0)):   # an empty shape reads no list
        (rowptr, col, _), st, _ = model.build(*shape, [9], [9])
        assert len(rowptr) == shape[0] + 1 and len(col) == 0 and st["launches"] == 0 and st["readbacks"] == 0


# ---- the models of the graph functions -------------------------------------------------------------------------------------------
def _weights(n_edges, seed, integer=False):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 9, n_edges).astype(np.float64) if integer else rng.random(n_edges) + 0.5   # (no -0.0, no NaN)


@pytest.mark.parametrize("name", ["rmat8", "rmat10"])
def test_the_adjacency_model_is_the_existing_helpers(name):
    n, r, c = GRAPHS[name]
    wn, wp, wc, wv = graph.symmetric_adjacency(r, c, n)
    rowptr, col, val = model.adjacency_matrix(n, r, c)
    assert wn == n and np.array_equal(rowptr, wp.numpy()) and np.array_equal(col, wc.numpy()) and np.array_equal(val, wv.numpy())
    w = _weights(len(r), 5)
    for directed in (False, True):
        for keep in ("min", "max"):
            _, wp, wc, wv = graph.weighted_adjacency(r, c, n, w, directed=directed, keep=keep)
            rowptr, col, val = model.adjacency_matrix(n, r, c, w, directed=directed, dup=keep)
            assert np.array_equal(rowptr, wp.numpy()) and np.array_equal(col, wc.numpy())
            assert np.array_equal(bits(val), bits(wv.numpy()))
    # loops=True keeps the diagonal; "count" gives multiplicities
    rowptr, col, val = model.adjacency_matrix(n, r, c, directed=True, loops=True, dup="count")
    want = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)).tocsr()
    want.sort_indices()
    assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices) and np.array_equal(val, want.data)
    assert (r == c).any() and want.diagonal().sum() > 0


def _summed_adjacency(n, r, c, w):
    keep = r != c
    u, v, w = r[keep], c[keep], w[keep]
    return sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n)).tocsr()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_laplacian_model_is_scipys(name):
    n, r, c = GRAPHS[name]
    for integer in (True, False):
        w = _weights(len(r), 6, integer)
        rowptr, col, val = model.laplacian(n, r, c, w)
        A = _summed_adjacency(n, r, c, w)
        if n == 0:
            assert rowptr.tolist() == [0] and len(col) == 0
            continue
        want = sp.csr_matrix(scipy_laplacian(A))
        L = sp.csr_matrix((val, col.astype(np.int64), rowptr), shape=(n, n))
        # the pattern: A's, and the diagonal of every vertex that has an edge
        deg = np.diff(A.indptr)
        assert len(col) == A.nnz + int((deg > 0).sum())
        diff = abs(L - want)
        if integer:
            assert diff.nnz == 0 or diff.max() == 0
        else:
            # a sum of k terms, reordered: each partial sum is off by at most eps * (sum of |terms|), k - 1 times; a row's
            # longest sum is its diagonal, of 2 * (parallel edges) <= 2 * (list entries of the row) terms
            absrow = np.asarray(abs(A).sum(axis=1)).ravel()
            terms = np.bincount(np.concatenate([r[r != c], c[r != c]]), minlength=n)
            bound = (terms.max() if len(terms) else 0) * np.finfo(np.float64).eps * absrow
            assert (diff.toarray() <= bound[:, None]).all()
    # without weights: every edge weighs 1, parallel edges add
    rowptr, col, val = model.laplacian(n, r, c)
    if n:
        want = sp.csr_matrix(scipy_laplacian(_summed_adjacency(n, r, c, np.ones(len(r)))))
        assert abs(sp.csr_matrix((val, col.astype(np.int64), rowptr), shape=(n, n)) - want).sum() == 0


def _nx_graph(n, rows, cols):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(rows, cols) if a != b)
    return G


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_incidence_model_is_networkx(name):
    n, r, c = GRAPHS[name]
    G = _nx_graph(n, r, c)
    (rowptr, col, val), u, v = model.incidence_matrix(n, r, c)
    edges = sorted((min(a, b), max(a, b)) for a, b in G.edges())
    assert list(zip(u.tolist(), v.tolist())) == edges
    assert len(rowptr) == n + 1 and (val == 1).all()
    if n == 0 or not edges:
        assert len(col) == 0
        return
    want = sp.csr_matrix(nx.incidence_matrix(G, nodelist=range(n), edgelist=edges))
    want.sort_indices()
    assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices) and np.array_equal(val, want.data)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_line_graph_model_is_networkx(name):
    n, r, c = GRAPHS[name]
    (rowptr, col, val), u, v = model.line_graph(n, r, c)
    edges = list(zip(u.tolist(), v.tolist()))
    number = {e: i for i, e in enumerate(edges)}
    LG = nx.line_graph(_nx_graph(n, r, c))
    want = sorted({(number[tuple(sorted(a))], number[tuple(sorted(b))]) for a, b in LG.edges()}
                  | {(number[tuple(sorted(b))], number[tuple(sorted(a))]) for a, b in LG.edges()})
    rr = np.repeat(np.arange(len(edges)), np.diff(rowptr))
    assert list(zip(rr.tolist(), col.tolist())) == want and (val == 1).all()
    assert len(rowptr) == len(edges) + 1
