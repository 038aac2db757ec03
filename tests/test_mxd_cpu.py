"""CPU-side checks of the product of a result with a dense matrix (include/outerspace_spgemm_mxd.h) and of what is built on
it: the symbol is exported and listed, the stats struct has the layout the C compiler gives it, null and illegal arguments
are argument errors that leave the outputs alone, the Python entries exist, validate operator names and shapes and fail
loudly without a GPU, and the models that judge the GPU (tests/mxd_model.py) equal things that share nothing with them:
``vector_model.reduce_segments`` for the one-lane order, scipy's ``A @ X``, networkx's local and global consistency, scipy's
float64 products."""
import ctypes
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from networkx.algorithms import node_classification

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import mxd_model as model
from tests import vector_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_mxd.h")
GRAPHS = model.propagate_graphs()
ALPHA, MAX_ITER = 0.99, 30


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _declared(path):
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_mxd_header_symbols_are_exported():
    hdr, declared = _declared(HEADER)
    L = _lib.lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert declared == set(_lib.MXD_EXPORTS) == {"osp_csr_mxd"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS, _lib.MXV_EXPORTS, _lib.EXTRACT_EXPORTS, _lib.BUILD_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm_mxm.h"' in hdr
    # the mxv header still declares exactly its one function
    assert _declared(os.path.join(ROOT, "include", "outerspace_spgemm_mxv.h"))[1] == {"osp_csr_mxv"}
    # the model's constants are the header's and the kernels'
    assert int(re.search(r"#define OSP_MXD_MAX_COLS (\d+)u", hdr).group(1)) == model.MAX_COLS == _lib.MXD_MAX_COLS
    src = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_mxd.h")).read()
    assert int(re.search(r"kMxdMaxCols\s*=\s*(\d+)", src).group(1)) == model.MAX_COLS
    assert list(_lib.MXV_ADD_OPS) == model.ADD_OPS and list(_lib.MXM_MUL_OPS) == model.MUL_OPS


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


def test_mxd_stats_have_the_layout_the_c_compiler_gives(tmp_path):
    cname, struct = "osp_mxd_stats_t", _lib.MxdStats
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_mxd.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "cols", "long_segments", "lanes_per_row", "launches", "ms_total"}


def test_mxd_null_and_illegal_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in`, whatever else is wrong with it, and a fake
    `in` with a null sr or y (the null checks come before `in` is touched; tests/test_gpu_mxd.py passes the other bad
    arguments with real results)."""
    L = _lib.lib()
    y = np.full((4, 2), 7.0)
    x = np.ones((4, 2))
    yp, xp = ctypes.c_void_p(y.ctypes.data), ctypes.c_void_p(x.ctypes.data)
    stats = _lib.MxdStats()
    stats.nnz_in = 77

    def semiring(add, mul, reserved=0):
        sr = _lib.Semiring()
        sr.add, sr.mul = _lib.EWISE_OPS[add], _lib.EWISE_OPS[mul]
        sr.reserved[0] = reserved
        return sr

    sr = semiring("plus", "times")
    fake = ctypes.c_void_p(0x1000)
    host, st = _lib.OSP_HOST, ctypes.byref(stats)
    calls = [lambda: L.osp_csr_mxd(None, ctypes.byref(sr), xp, 2, yp, host, st),
             lambda: L.osp_csr_mxd(None, None, None, 0, None, host, None),
             lambda: L.osp_csr_mxd(None, ctypes.byref(sr), None, 2, yp, 99, st),
             lambda: L.osp_csr_mxd(None, ctypes.byref(semiring("first", "div")), xp, 2, yp, host, st),
             lambda: L.osp_csr_mxd(None, ctypes.byref(semiring("plus", "times", 1)), xp, 2, yp, host, st),
             lambda: L.osp_csr_mxd(None, ctypes.byref(sr), xp, model.MAX_COLS + 1, yp, host, st),
             lambda: L.osp_csr_mxd(fake, None, xp, 2, yp, host, st),
             lambda: L.osp_csr_mxd(fake, ctypes.byref(sr), xp, 2, None, host, st)]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert stats.nnz_in == 77 and (y == 7.0).all()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_entries_exist_and_validate_names_and_shapes():
    assert callable(S.CsrResult.mxd) and callable(graph.label_spreading) and callable(graph.propagate_features)
    res = object.__new__(S.CsrResult)   # (no handle: names and shapes are checked before anything is touched)
    res._h, res.shape, res.dtype = None, (3, 4), np.float64
    X = np.ones((4, 2))
    for kw in ({"add": "first"}, {"add": "times"}, {"mul": "minus"}, {"mul": "div"}, {"add": "sum"}):
        with pytest.raises(ValueError):
            res.mxd(X, space="host", **kw)
    with pytest.raises(ValueError):
        res.mxd(X, space="pinned")
    bad = [lambda: res.mxd(np.ones((3, 2)), space="host"),                        # N is 4
           lambda: res.mxd(np.ones(4), space="host"),                             # not 2-D
           lambda: res.mxd(None, space="host"),                                   # None without mul="first"
           lambda: res.mxd(None, mul="first", space="host"),                      # no X and no k
           lambda: res.mxd(X, out=np.ones((3, 3)), space="host"),                 # out is not (M, k)
           lambda: res.mxd(X, out=np.ones((3, 2), np.float32), space="host"),     # out's dtype
           lambda: res.mxd(X, out=np.ones((2, 3)).T, space="host"),               # out is not contiguous
           lambda: res.mxd(torch.ones(4, 2, dtype=torch.float32)),                # a tensor of the wrong dtype
           lambda: res.mxd(torch.ones(4, 4, dtype=torch.float64)[:, :2]),         # a tensor that is not contiguous
           lambda: res.mxd(torch.ones(4, 2, dtype=torch.float64), out=torch.ones(4, 2, dtype=torch.float64)),
           lambda: res.mxd(0x1000, space="device"),                               # an address without k
           lambda: res.mxd(None, mul="first", k=model.MAX_COLS + 1, space="host"),
           lambda: res.mxd(None, mul="first", k=-1, space="host")]
    for call in bad:
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_ARG
    assert [model.lanes_per_row(k) for k in model.KS] == [1, 2, 4, 4, 8, 16, 32, 64, 64, 64, 64]


def test_graph_functions_validate_their_arguments_first():
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    with pytest.raises(ValueError):
        graph.label_spreading(r, c, 3, None)
    with pytest.raises(ValueError):
        graph.label_spreading(r, c, 3, {0: 0}, alpha=1.0)
    with pytest.raises(ValueError):
        graph.propagate_features(r, c, 3, None)
    with pytest.raises(ValueError):
        graph.propagate_features(r, c, 3, np.ones((3, 1)), hops=-1)


def test_mxd_of_a_result_without_a_handle_is_an_error_not_a_host_computation():
    """A call with nothing wrong but the missing handle reaches the C entry and comes back as its argument error: there
    is no path that computes the product on the host."""
    res = object.__new__(S.CsrResult)
    res._h, res.shape, res.dtype = None, (3, 4), np.float64
    out = np.full((3, 2), 7.0)
    for kw in ({}, {"add": "min", "mul": "plus"}, {"out": out}):
        with pytest.raises(S.OspError) as ei:
            res.mxd(np.ones((4, 2)), space="host", **kw)
        assert ei.value.status == _lib.ERR_ARG and "null argument" in str(ei.value)
    assert (out == 7.0).all()


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(S.OspError) as ei:
        S.Context(0)   # (what every CsrResult, and so every mxd call, needs first)
    assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.label_spreading(r, c, 3, {0: 0, 2: 1}), lambda: graph.propagate_features(r, c, 3, np.ones((3, 2)))):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the one-lane order -------------------------------------------------------------------------------------------------------------
LENGTHS = list(range(10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4097, 2048 * 64 + 5]


def _special_values(length, dt, rng):
    """Random values with a NaN, both infinities and -0.0 among them (where they fit), and nothing but -0.0 when asked."""
    e = rng.standard_normal(length).astype(dt)
    if length >= 2:
        where = rng.choice(length, size=min(length, 8), replace=False)
        e[where] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 0.0, -0.0], dt), len(where))
    return e


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("add", model.ADD_OPS)
def test_serial_R_is_the_vector_models_R_in_bits(dt, add):
    rng = np.random.default_rng(7)
    for length in LENGTHS:
        inputs = [rng.standard_normal(length).astype(dt), np.full(length, -0.0, dt), _special_values(length, dt, rng),
                  np.where(rng.random(length) < 0.5, -0.0, rng.standard_normal(length)).astype(dt)]
        for e in inputs:
            want = vector_model.reduce_segments(np.array([0, length]), e, add)[0]
            got = model.serial_R(e, add)
            assert got.dtype == dt
            if add == "plus" and np.isnan(want[0]):
                assert np.isnan(got), (length, add)
            else:
                assert _bits(want)[0] == _bits(np.array([got]))[0], (length, add)


# ---- the model of mxd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_is_scipys_product_on_exact_values(dt):
    """Small integers times powers of two: every product and every partial sum is exact in float32, so any order of
    summation gives scipy's bits.  Rows of 0 to 5000 entries, 5 columns."""
    rng = np.random.default_rng(2)
    ncol, k = 6000, 5
    lengths = [0, 1, 3, 64, 65, 700, 2048, 2049, 5000, 0, 17]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=m, replace=False)) for m in lengths]).astype(np.uint32)
    val = rng.integers(-8, 9, len(col)).astype(dt)
    X = (rng.integers(-4, 5, (ncol, k)) * 2.0 ** rng.integers(-2, 3, (ncol, k))).astype(dt)
    got, nlong = model.mxd(rowptr, col, val, X, "plus", "times")
    want = sp.csr_matrix((val, col.astype(np.int64), rowptr), shape=(len(lengths), ncol)) @ X
    assert got.dtype == dt and got.shape == (len(lengths), k) and nlong == 2
    assert np.array_equal(got, want.astype(dt)) and not np.signbit(got[0]).any()
    assert model.expected_launches(rowptr, scan_launches=1) == 7 and model.expected_launches(rowptr[:6]) == 1
    assert model.expected_launches(np.array([0, 2000, 4000])) == 3 and model.expected_launches(np.array([0, 0])) == 0


# ---- the models of the graph functions -------------------------------------------------------------------------------------------
def _networkx_predictions(n, rows, cols, labels):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(rows, cols) if a != b)
    for v, cls in labels.items():
        G.nodes[v]["label"] = cls
    return node_classification.local_and_global_consistency(G, alpha=ALPHA, max_iter=MAX_ITER)


@pytest.mark.parametrize("nclasses", [2, 3, 5])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_label_model_predicts_what_networkx_predicts(name, nclasses):
    """The model in float64 against networkx wherever the float64 scipy evaluation's two largest entries of a row are further
    apart, relatively, than twice the bound of the float32 run -- the widest margin tests/test_gpu_propagate.py uses.

    A vertex that no labelled vertex reaches (an isolated one, the unlabelled component; a quarter of R-MAT 8's vertices have
    no edge) has a row of exact zeros: it has no margin in ANY arithmetic, so it is checked for that -- exactly 0 -- and the
    share of decided vertices is taken among the reached ones."""
    n, r, c = GRAPHS[name]
    labels = model.labellings(name, n, nclasses)
    assert len(set(labels.values())) == nclasses
    F, predicted, info = model.label_spreading(n, r, c, labels, ALPHA, MAX_ITER)
    ref, maxdeg = model.reference_label_spreading(n, r, c, labels, ALPHA, MAX_ITER)
    want = _networkx_predictions(n, r, c, labels)
    assert info["iterations"] == MAX_ITER and info["max_degree"] == maxdeg and info["classes"] == list(range(nclasses))
    reached = ref.max(axis=1) > 0
    assert np.array_equal(F[~reached], np.zeros_like(F[~reached]))
    with np.errstate(all="ignore"):
        rel = np.abs(F - ref)[ref > 0] / ref[ref > 0]
    assert not (F[ref == 0] != 0).any() and rel.max() <= model.label_bound(MAX_ITER, maxdeg, np.float64)
    for dt in (np.float32, np.float64):
        decided = model.margins(ref) > 2 * model.label_bound(MAX_ITER, maxdeg, dt)
        share = decided[reached].mean()
        print(f"{name} classes={nclasses} {dt.__name__}: reached={reached.sum()}/{n} decided among them={share:.3f} max rel={rel.max():.2e}")
        assert share >= 0.9 and not decided[~reached].any()
        assert [p for p, d in zip(predicted, decided) if d] == [w for w, d in zip(want, decided) if d]
    if "isolated" in name:
        assert (~reached).sum() == 4 and (np.diff(model.mxv_model.pattern(n, r, c, False).indptr) == 0).sum() == 1


@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_feature_model_is_scipy_in_float64(name, self_loops):
    n, r, c = GRAPHS[name]
    X = np.random.default_rng(3).standard_normal((n, 5))
    for hops in (1, 2, 3):
        got, info = model.propagate_features(n, r, c, X, hops, self_loops)
        want, scale, maxdeg = model.reference_propagate(n, r, c, X, hops, self_loops)
        assert info["max_degree"] == maxdeg and got.shape == want.shape
        assert (np.abs(got - want) <= model.propagate_bound(hops, maxdeg, np.float64) * scale).all()
    assert np.array_equal(model.propagate_features(n, r, c, X, 0, self_loops)[0], X)


def test_the_graph_models_on_empty_and_edgeless_graphs():
    none = np.zeros(0, np.int64)
    F, predicted, info = model.label_spreading(5, none, none, {1: 0, 3: 1}, ALPHA, MAX_ITER)
    assert info["nnz"] == 0 and predicted == [0, 0, 0, 1, 0]
    assert np.array_equal(F, (1 - ALPHA) * np.array([[0, 0], [1, 0], [0, 0], [0, 1], [0, 0.0]]))
    X = np.arange(10.0).reshape(5, 2)
    assert np.array_equal(model.propagate_features(5, none, none, X, 2, True)[0], X)           # A^ is the identity
    assert np.array_equal(model.propagate_features(5, none, none, X, 2, False)[0], 0 * X)
    assert model.propagate_features(0, none, none, np.zeros((0, 3)), 2)[0].shape == (0, 3)
