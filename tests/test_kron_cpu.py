"""CPU-side checks of the Kronecker product of two results (include/outerspace_spgemm_kron.h) and of what is built on it:
the symbol is exported and listed, both structs have the layout the C compiler gives them, null arguments are argument
errors that leave the outputs alone, the Python entries exist, validate before they touch a handle and fail loudly without
a GPU, and the models that judge the GPU (tests/kron_model.py) equal things that share nothing with them:
``scipy.sparse.kron``, a dense construction, the header's closed form of the row pointers, networkx's three graph products
and ``numpy.kron`` applied k times."""
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
from tests import kron_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_kron.h")
KERNELS = os.path.join(ROOT, "outerspace_amd", "csrc", "osp_kron.h")


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_kron_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.KRON_EXPORTS) == {"osp_csr_kron"}
    others = [name for name in dir(_lib) if name.endswith("EXPORTS") and name != "KRON_EXPORTS"]
    assert len(others) >= 17
    for name in others:
        assert not declared & set(getattr(_lib, name)), name
    assert _lib.KRON_OPS == {name: _lib.EWISE_OPS[name] for name in model.OPS}
    # the header states the kernels of the general path; the kernels' header and the model agree
    launches = int(re.search(r"#define OSP_KRON_LAUNCHES (\d+)", hdr).group(1))
    src = open(KERNELS).read()
    assert launches == _lib.KRON_LAUNCHES == model.LAUNCHES == int(re.search(r"kKronLaunches\s*=\s*(\d+)", src).group(1))
    assert re.search(r"kKronThreads\s*=\s*(\d+)", src) and re.search(r"kKronEntries\s*=\s*(\d+)", src)


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_kron_t", _lib.Kron), ("osp_kron_stats_t", _lib.KronStats)])
def test_kron_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_kron.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    if struct is _lib.KronStats:
        assert set(struct().as_dict()) == {"nnz_a", "nnz_b", "nnz_out", "ms_total", "launches", "readbacks"}


def test_kron_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null a or b (whatever else is wrong with it), and fake
    operands with a null kr or out (the null checks come before an operand is touched; tests/test_gpu_kron.py passes the
    other bad arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.KronStats()
    stats.nnz_a = 77
    ok = _lib.Kron()
    ok.op = _lib.KRON_OPS["times"]
    bad_op = _lib.Kron()
    bad_op.op = _lib.EWISE_OPS["minus"]
    bad_word = _lib.Kron()
    bad_word.reserved[6] = 1
    fake = ctypes.c_void_p(0x1000)
    refs = (ctypes.byref(out), ctypes.byref(stats))
    calls = [lambda: L.osp_csr_kron(None, None, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_kron(None, fake, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_kron(fake, None, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_kron(None, None, ctypes.byref(bad_op), *refs),
             lambda: L.osp_csr_kron(None, None, ctypes.byref(bad_word), *refs),
             lambda: L.osp_csr_kron(None, None, None, None, None),
             lambda: L.osp_csr_kron(fake, fake, None, *refs),
             lambda: L.osp_csr_kron(fake, fake, ctypes.byref(ok), None, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_a == 77


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _fake(shape=(3, 3)):
    res = object.__new__(S.CsrResult)   # (no handle: the arguments are checked before anything is touched)
    res._h, res._ctx, res.shape, res.dtype, res.nnz = None, None, shape, np.float64, 0
    return res


def test_python_entries_exist_and_validate_before_touching_a_handle():
    assert callable(S.CsrResult.kron)
    for name in ("tensor_product", "cartesian_product", "strong_product", "kronecker_power"):
        assert callable(getattr(graph, name))
    a, b = _fake(), _fake((2, 5))
    for bad in ("minus", "div", "xor", None, 1):
        with pytest.raises(ValueError):
            a.kron(b, bad)
    with pytest.raises(TypeError):
        a.kron("b")
    wrong = _fake()
    wrong.dtype = np.float32
    with pytest.raises(S.OspError) as ei:
        a.kron(wrong)
    assert ei.value.status == _lib.ERR_ARG
    foreign = _fake()
    foreign._ctx = object()
    with pytest.raises(S.OspError) as ei:
        a.kron(foreign, "first")
    assert ei.value.status == _lib.ERR_ARG


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    g = (r, c, 3)
    for call in (lambda: graph.tensor_product(g, g), lambda: graph.cartesian_product(g, g), lambda: graph.strong_product(g, g),
                 lambda: graph.kronecker_power(r, c, 3, 2)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of kron -----------------------------------------------------------------------------------------------------------
def _csr(lengths, ncol, dt, seed, zeros=5):
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=k, replace=False)) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    val[::zeros] = 0.0                                               # explicit zeros are entries
    return rowptr, col, val


# (name: row lengths, columns) -- empty first rows, empty last rows, runs of empty rows, a full row, a single entry
OPERANDS = {"ragged": ([0, 1, 0, 0, 2, 3, 0, 1, 0], 11), "first_empty": ([0, 0, 4, 1], 6), "last_empty": ([3, 7, 0, 0, 0], 7),
            "full": ([5, 5, 5], 5), "one": ([1], 1), "row": ([9], 13), "column": ([1, 0, 1, 0, 1], 1), "empty": ([0, 0, 0], 4),
            "no_rows": ([], 3)}


def _positions(csr, ncol):
    """scipy's view of a pattern whose data are the entries' positions + 1 (so that explicit zeros stay entries)."""
    rowptr, col, _ = csr
    return sp.csr_matrix((np.arange(1, len(col) + 1, dtype=np.float64), col.astype(np.int64), rowptr), shape=(len(rowptr) - 1, ncol))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_under_times_is_scipys_kron(dt):
    seed = 0
    for an, (la, na) in OPERANDS.items():
        for bn, (lb, nb) in OPERANDS.items():
            seed += 2
            a, b = _csr(la, na, dt, seed), _csr(lb, nb, dt, seed + 1)
            (rowptr, col, val), shape, st = model.kron(a, na, b, nb, "times")
            # the structure from scipy on positions (never zero, so that scipy's padding of a dense b can be dropped)
            P = sp.csr_matrix(sp.kron(_positions(a, na), _positions(b, nb), format="csr"))
            P.eliminate_zeros()
            P.sort_indices()
            assert shape == P.shape == (len(la) * len(lb), na * nb), (an, bn)
            assert np.array_equal(rowptr, P.indptr) and np.array_equal(col, P.indices), (an, bn)
            # which pair of entries stands where, from the header's definition: scipy's data are (pa + 1) (pb + 1)
            pa, pb = _pairs(a, b)
            assert np.array_equal(P.data, (pa + 1.0) * (pb + 1.0)), (an, bn)
            assert val.dtype == dt and np.array_equal(_bits(val), _bits(a[2][pa] * b[2][pb])), (an, bn)   # (explicit zeros included)
            # scipy's values, bit for bit, on the operands without their explicit zeros' values (1 in their place)
            a1, b1 = (a[0], a[1], np.where(a[2] == 0, dt(1), a[2])), (b[0], b[1], np.where(b[2] == 0, dt(1), b[2]))
            V = sp.csr_matrix(sp.kron(sp.csr_matrix(a1[::-1], shape=(len(la), na)), sp.csr_matrix(b1[::-1], shape=(len(lb), nb)), format="csr"))
            V.eliminate_zeros()
            V.sort_indices()
            got = model.kron(a1, na, b1, nb, "times")[0]
            assert (V.dtype == dt or V.nnz == 0) and np.array_equal(got[0], V.indptr) and np.array_equal(got[1], V.indices), (an, bn)
            assert np.array_equal(_bits(got[2]), _bits(V.data)), (an, bn)
            no_work = len(a[1]) == 0 or len(b[1]) == 0 or shape[0] == 0
            assert st == {"nnz_a": len(a[1]), "nnz_b": len(b[1]), "nnz_out": len(col), "launches": 0 if no_work else 2, "readbacks": 0,
                          "no_work": no_work}


def _pairs(a, b):
    """(pa, pb) of every entry of a (x) b in out's order, from the DEFINITION of the header: entry q of row ia mB + ib comes
    from pa = rpA[ia] + q / lenB[ib] and pb = rpB[ib] + q % lenB[ib] (a loop over rows; the model repeats and tiles)."""
    pa, pb = [], []
    for ia in range(len(a[0]) - 1):
        for ib in range(len(b[0]) - 1):
            la, lb = int(a[0][ia + 1] - a[0][ia]), int(b[0][ib + 1] - b[0][ib])
            for q in range(la * lb):
                pa.append(int(a[0][ia]) + q // lb)
                pb.append(int(b[0][ib]) + q % lb)
    return np.array(pa, np.int64), np.array(pb, np.int64)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("op", model.OPS)
def test_the_model_equals_a_dense_construction(op, dt):
    special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1.0, -2.5], dt)
    for (an, bn) in (("ragged", "last_empty"), ("first_empty", "ragged"), ("row", "column"), ("full", "one"), ("column", "full")):
        (la, na), (lb, nb) = OPERANDS[an], OPERANDS[bn]
        a, b = _csr(la, na, dt, 40), _csr(lb, nb, dt, 41)
        a[2][::3] = np.resize(special, len(a[2][::3]))
        b[2][1::4] = np.resize(special[::-1], len(b[2][1::4]))
        (rowptr, col, val), (M, N), _ = model.kron(a, na, b, nb, op)
        # dense: values and pattern of each operand, then the block structure spelled out index by index
        D, Pd = np.zeros((M, N), dt), np.zeros((M, N), bool)
        ra, rb = np.repeat(np.arange(len(la)), la), np.repeat(np.arange(len(lb)), lb)
        for i, j, x in zip(ra.tolist(), a[1].tolist(), a[2]):
            for k, l, y in zip(rb.tolist(), b[1].tolist(), b[2]):
                D[i * len(lb) + k, j * nb + l] = model.apply_op(op, np.array([x], dt), np.array([y], dt))[0]
                Pd[i * len(lb) + k, j * nb + l] = True
        r, c = np.nonzero(Pd)
        assert np.array_equal(rowptr, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))])), (an, bn)
        assert np.array_equal(col, c), (an, bn)
        assert np.array_equal(_bits(val), _bits(D[r, c])), (an, bn)
        assert (np.diff(col.astype(np.int64))[np.diff(np.repeat(np.arange(M), np.diff(rowptr))) == 0] > 0).all()   # columns ascend


def test_the_closed_form_row_pointer_is_the_models():
    for an, (la, na) in OPERANDS.items():
        for bn, (lb, nb) in OPERANDS.items():
            a, b = _csr(la, na, np.float64, 50), _csr(lb, nb, np.float64, 51)
            rowptr = model.kron(a, na, b, nb)[0][0]
            assert np.array_equal(model.closed_form_rowptr(a[0], b[0]), rowptr), (an, bn)
            assert rowptr[-1] == len(a[1]) * len(b[1])


def test_the_model_refuses_what_the_library_refuses():
    one = (np.array([0, 1], np.int64), np.zeros(1, np.uint32), np.ones(1))
    tall = (np.zeros(65536, np.int64), np.zeros(0, np.uint32), np.zeros(0))   # 65535 rows
    taller = (np.zeros(65538, np.int64), np.zeros(0, np.uint32), np.zeros(0))  # 65537 rows
    with pytest.raises(ValueError):
        model.kron(one, 1, one, 1, "minus")
    with pytest.raises(ValueError):
        model.kron(one, 65536, one, 65536)
    with pytest.raises(ValueError):
        model.kron(tall, 1, taller, 1)
    with pytest.raises(ValueError):
        model.kron(one, 1, (one[0], one[1], np.ones(1, np.float32)), 1)
    assert model.kron(one, 65535, one, 65537)[1] == (1, (1 << 32) - 1)


# ---- the models of the graph functions -------------------------------------------------------------------------------------------------
def _graph(G):
    G = nx.convert_node_labels_to_integers(G)
    e = np.array(G.edges(), np.int64).reshape(-1, 2)
    return G, (e[:, 0], e[:, 1], G.number_of_nodes())


GRAPHS = {"path": nx.path_graph(5), "cycle": nx.cycle_graph(6), "star": nx.star_graph(4), "petersen": nx.petersen_graph()}
PAIRS = [("path", "cycle"), ("cycle", "star"), ("star", "petersen"), ("petersen", "path"), ("cycle", "cycle")]


def _edge_set(csr):
    u = np.repeat(np.arange(len(csr[0]) - 1), np.diff(csr[0]))
    return set(zip(u.tolist(), csr[1].astype(np.int64).tolist()))


@pytest.mark.parametrize("product", ["tensor_product", "cartesian_product", "strong_product"])
@pytest.mark.parametrize("pair", PAIRS)
def test_the_product_models_are_networkx(pair, product):
    (G, g), (H, h) = _graph(GRAPHS[pair[0]]), _graph(GRAPHS[pair[1]])
    n2 = h[2]
    P = getattr(nx, product)(G, H)
    want = {(u * n2 + v, x * n2 + y) for (u, v), (x, y) in P.edges()}
    want |= {(b, a) for a, b in want}
    out = getattr(model, product)(g, h)
    assert len(out[0]) == g[2] * n2 + 1 == P.number_of_nodes() + 1
    assert _edge_set(out) == want
    assert (out[2] == 1.0).all()   # (loop-free graphs: the three parts of a strong product do not overlap)


def test_the_directed_product_models_are_networkx():
    G, H = nx.gnp_random_graph(6, 0.4, seed=1, directed=True), nx.gnp_random_graph(5, 0.5, seed=2, directed=True)
    G.add_edge(2, 2)
    H.add_edge(0, 0)
    H.add_edge(3, 3)
    g, h = _graph(G)[1], _graph(H)[1]
    for product in ("tensor_product", "cartesian_product", "strong_product"):
        P = getattr(nx, product)(G, H)
        want = {(u * 5 + v, x * 5 + y) for (u, v), (x, y) in P.edges()}
        assert _edge_set(getattr(model, product)(g, h, directed=True)) == want, product


@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_kronecker_power_model_is_numpys_kron(k):
    r, c, n = np.array([0, 0, 1, 2, 2]), np.array([0, 1, 2, 2, 0]), 3   # two self loops
    for directed in (False, True):
        for loops in (False, True):
            A = np.zeros((n, n))
            for u, v in zip(r, c):
                if u != v or loops:
                    A[u, v] = 1
                    if not directed:
                        A[v, u] = 1
            D = A
            for _ in range(k - 1):
                D = np.kron(D, A)
            rowptr, col, val = model.kronecker_power(r, c, n, k, directed, loops)
            assert len(rowptr) == n ** k + 1 and len(col) == int(A.sum()) ** k
            rr, cc = np.nonzero(D)
            assert np.array_equal(col, cc) and np.array_equal(np.diff(rowptr), np.bincount(rr, minlength=n ** k)) and (val == 1).all()


@pytest.mark.parametrize("pair", PAIRS + [("petersen", "petersen")])
def test_the_triangle_identity_on_the_model(pair):
    """t(G (x) H) = 6 t(G) t(H) for loop-free symmetric graphs: trace((A (x) B)^3) = trace(A^3) trace(B^3)."""
    K4, W = nx.complete_graph(4), nx.wheel_graph(6)
    for G, H in ((GRAPHS[pair[0]], GRAPHS[pair[1]]), (K4, GRAPHS[pair[1]]), (K4, W), (W, W)):
        g, h = _graph(G)[1], _graph(H)[1]
        tg, th = sum(nx.triangles(G).values()) // 3, sum(nx.triangles(H).values()) // 3
        assert model.triangles(model.tensor_product(g, h)) == 6 * tg * th
    assert model.triangles(model.tensor_product(_graph(K4)[1], _graph(W)[1])) == 6 * 4 * 5
