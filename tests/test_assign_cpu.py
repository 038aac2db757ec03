"""CPU-side checks of the assignment into a region of a result (include/outerspace_spgemm_assign.h) and of what is built on
it: the symbol is exported and listed, both structs have the layout the C compiler gives them, null and illegal arguments
are argument errors that leave the outputs alone, the Python entries exist, validate ``space`` and their lists before they
touch a handle and fail loudly without a GPU, and the models that judge the GPU (tests/assign_model.py) equal things that
share nothing with them: scipy's ``lil`` assignment of a region and its union, ``scipy.sparse.bmat``, and networkx's
``from_biadjacency_matrix``, ``disjoint_union_all`` and edge removal and insertion."""
import ctypes
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from networkx.algorithms import bipartite

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import assign_model as model
from tests import extract_model
from tests import mxv_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_assign.h")
GRAPHS = {name: g for name, g in mxv_model.component_graphs().items() if name in ("rmat8", "rmat10")}


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_assign_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.ASSIGN_EXPORTS) == {"osp_csr_assign"}
    others = [name for name in dir(_lib) if name.endswith("EXPORTS") and name != "ASSIGN_EXPORTS"]
    assert len(others) >= 16
    for name in others:
        assert not declared & set(getattr(_lib, name)), name
    assert "#define OSP_ASSIGN_NO_ACCUM (-1)" in hdr and _lib.ASSIGN_NO_ACCUM == -1
    assert _lib.ASSIGN_ACCUM_OPS == {name: _lib.EWISE_OPS[name] for name in model.ACCUM_OPS}


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_assign_t", _lib.Assign), ("osp_assign_stats_t", _lib.AssignStats)])
def test_assign_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_assign.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    if struct is _lib.AssignStats:
        assert set(struct().as_dict()) == {"nnz_c", "nnz_a", "nnz_region", "nnz_both", "nnz_out", "ms_total", "launches", "readbacks"}


def test_assign_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null c or a (whatever else is wrong with it), and fake
    operands with a null as or out (the null checks come before an operand is touched; tests/test_gpu_assign.py passes the
    other bad arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.AssignStats()
    stats.nnz_c = 77
    rows = np.array([0, 1], np.uint32)
    ok = _lib.Assign()
    ok.rows, ok.n_rows, ok.space, ok.accum = rows.ctypes.data, 2, _lib.OSP_HOST, _lib.ASSIGN_NO_ACCUM
    bad_space = _lib.Assign()
    bad_space.space = 99
    bad_accum = _lib.Assign()
    bad_accum.accum = _lib.EWISE_OPS["minus"]
    bad_word = _lib.Assign()
    bad_word.reserved[5] = 1
    huge = _lib.Assign()
    huge.rows, huge.n_rows, huge.space = rows.ctypes.data, 1 << 32, _lib.OSP_HOST
    fake = ctypes.c_void_p(0x1000)
    refs = (ctypes.byref(out), ctypes.byref(stats))
    calls = [lambda: L.osp_csr_assign(None, None, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_assign(None, fake, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_assign(fake, None, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_assign(None, None, ctypes.byref(bad_space), *refs),
             lambda: L.osp_csr_assign(None, None, ctypes.byref(bad_accum), *refs),
             lambda: L.osp_csr_assign(None, None, ctypes.byref(bad_word), *refs),
             lambda: L.osp_csr_assign(None, None, ctypes.byref(huge), *refs),
             lambda: L.osp_csr_assign(None, None, None, None, None),
             lambda: L.osp_csr_assign(fake, fake, None, *refs),
             lambda: L.osp_csr_assign(fake, fake, ctypes.byref(ok), None, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_c == 77


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _fake(shape=(3, 3)):
    res = object.__new__(S.CsrResult)   # (no handle: the arguments are checked before anything is touched)
    res._h, res._ctx, res.shape, res.dtype, res.nnz = None, None, shape, np.float64, 0
    return res


def test_python_entries_exist_and_validate_before_touching_a_handle():
    assert callable(S.CsrResult.assign) and callable(S.CsrResult.embed) and callable(S.block_matrix)
    assert callable(graph.bipartite_adjacency) and callable(graph.disjoint_union) and callable(graph.replace_subgraph)
    res, a = _fake(), _fake((1, 1))
    for kw in ({"rows": [0]}, {"cols": [0]}, {}):
        with pytest.raises(ValueError):
            res.assign(a, space="pinned", **kw)
        with pytest.raises(ValueError):
            a.embed((3, 3), space="pinned", **kw)
    with pytest.raises(ValueError):
        res.assign(a, [0], [0], accum="minus", space="host")
    for bad in ([-1], [1 << 32], [0.5], [[0, 1]]):
        for call in (lambda: res.assign(a, rows=bad, space="host"), lambda: res.assign(a, cols=bad, space="host"),
                     lambda: a.embed((3, 3), rows=bad, space="host"), lambda: a.embed((3, 3), cols=bad, space="host")):
            with pytest.raises(S.OspError) as ei:
                call()
            assert ei.value.status == _lib.ERR_ARG
    with pytest.raises(TypeError):
        res.assign("a", [0], [0], space="host")
    wrong = _fake((1, 1))
    wrong.dtype = np.float32
    with pytest.raises(S.OspError) as ei:
        res.assign(wrong, [0], [0], space="host")
    assert ei.value.status == _lib.ERR_ARG
    with pytest.raises(S.OspError) as ei:      # the composed path knows a's width before it calls anything
        res.assign(a, [0], [2, 1], space="host")
    assert ei.value.status == _lib.ERR_DIM
    # block_matrix checks its grid without a handle
    for grid in ([], [[]], [[res], [res, res]], [[None]], [[res, None], [None, None]]):
        with pytest.raises(ValueError):
            S.block_matrix(grid)
    with pytest.raises(TypeError):
        S.block_matrix([["x"]])
    with pytest.raises(ValueError):
        S.block_matrix([[res], [_fake((2, 4))]])
    with pytest.raises(S.OspError):
        S.block_matrix([[a, wrong]])
    a._ctx = object()
    with pytest.raises(S.OspError):
        S.block_matrix([[a, _fake((1, 1))]])


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.bipartite_adjacency(r, c, (3, 3)), lambda: graph.disjoint_union([(r, c, 3), (r, c, 3)]),
                 lambda: graph.replace_subgraph(r, c, 3, [0, 1], [0], [1])):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of assign ---------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 64, 65, 700, 0, 2048, 2049, 5000, 17, 0]
NCOL = 6000


def _csr(lengths, ncol, dt, seed, zeros=5):
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncol, size=k, replace=False)) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    val[::zeros] = 0.0                                               # explicit zeros are entries
    return rowptr, col, val


def _lists(M, ncol, rng):
    rows = {"none": None, "identity": np.arange(M), "reversed": np.arange(M)[::-1], "one": np.array([9]),
            "some": np.array([7, 10, 0, 11, 6, 9]), "empty": np.zeros(0, np.int64)}
    cols = {"none": None, "all": np.arange(ncol), "half": np.sort(rng.choice(ncol, ncol // 2, replace=False)),
            "every 64th": np.arange(0, ncol, 64), "first": np.array([0]), "last": np.array([ncol - 1]), "empty": np.zeros(0, np.int64)}
    return rows, cols


def _a_for(m, n, dt, seed):
    """An a of m x n: rows of 0 to n entries."""
    rng = np.random.default_rng(seed)
    lengths = [0 if n == 0 else int(x) for x in rng.integers(0, min(n, 3000) + 1, m)]
    if m > 1:
        lengths[0], lengths[-1] = min(n, 5000), 0
    return _csr(lengths, max(n, 1), dt, seed + 1, zeros=3) if m else (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))


def _dense_parts(csr, M, ncol):
    """(values, pattern) as dense arrays."""
    rowptr, col, val = csr
    row = np.repeat(np.arange(M), np.diff(rowptr))
    V, P = np.zeros((M, ncol), val.dtype), np.zeros((M, ncol), bool)
    V[row, col.astype(np.int64)], P[row, col.astype(np.int64)] = val, True
    return V, P


def _scipy_assign(c, ncol, a, rows, cols, accum):
    """scipy's side: the region of c assigned through ``lil`` (no accum: after the region is cleared) or united with it
    (accum), on PATTERNS and on positions, so that explicit zeros stay entries.  Returns (rowptr, col, position in c or -1,
    position in a or -1)."""
    M = len(c[0]) - 1
    I = np.arange(M) if rows is None else np.asarray(rows, np.int64)
    J = np.arange(ncol) if cols is None else np.asarray(cols, np.int64)
    Pc = sp.csr_matrix((np.arange(1, len(c[1]) + 1, dtype=np.float64), c[1].astype(np.int64), c[0]), shape=(M, ncol)).tolil()
    Pa = sp.csr_matrix((np.arange(1, len(a[1]) + 1, dtype=np.float64), a[1].astype(np.int64), a[0]), shape=(len(I), len(J)))
    big_a = sp.lil_matrix((M, ncol))
    if len(I) and len(J):
        big_a[np.ix_(I, J)] = Pa.toarray()
        if accum is None:
            Pc[np.ix_(I, J)] = 0
    Pc, big_a = sp.csr_matrix(Pc), sp.csr_matrix(big_a)
    Pc.eliminate_zeros()
    big_a.eliminate_zeros()
    pattern = sp.csr_matrix(((Pc != 0) + (big_a != 0)).astype(np.float64))
    pattern.sort_indices()
    row = np.repeat(np.arange(M), np.diff(pattern.indptr))
    pc = np.asarray(Pc[row, pattern.indices]).ravel().astype(np.int64) - 1 if pattern.nnz else np.zeros(0, np.int64)
    pa = np.asarray(big_a[row, pattern.indices]).ravel().astype(np.int64) - 1 if pattern.nnz else np.zeros(0, np.int64)
    return pattern.indptr.astype(np.int64), pattern.indices.astype(np.uint32), pc, pa


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_is_scipys_region_assignment(dt):
    c = _csr(LENGTHS, NCOL, dt, 3)
    M = len(LENGTHS)
    rows, cols = _lists(M, NCOL, np.random.default_rng(4))
    assert len(rows) >= 6 and len(cols) >= 6
    seed = 100
    for rn, I in rows.items():
        for cn, J in cols.items():
            m, n = M if I is None else len(I), NCOL if J is None else len(J)
            seed += 1
            a = _a_for(m, n, dt, seed)
            scipy_side = {acc: _scipy_assign(c, NCOL, a, I, J, acc) for acc in (None, "plus")}
            for accum in (None,) + tuple(model.ACCUM_OPS):
                (rowptr, col, val), computed, st = model.assign(c, NCOL, a, n, I, J, accum)
                wp, wc, pc, pa = scipy_side[None if accum is None else "plus"]
                assert np.array_equal(rowptr, wp) and np.array_equal(col, wc), (rn, cn, accum)
                both = (pc >= 0) & (pa >= 0)
                assert accum is not None or not both.any()
                want = np.empty(len(wc), dt)
                want[pc >= 0] = c[2][pc[pc >= 0]]
                want[pa >= 0] = a[2][pa[pa >= 0]]
                if accum is not None:
                    want[both] = model.ewise_model.apply_op(accum, c[2][pc[both]], a[2][pa[both]])
                assert val.dtype == dt and np.array_equal(_bits(val), _bits(want)), (rn, cn, accum)
                assert np.array_equal(computed, both) or st["no_work"], (rn, cn, accum)
                assert (st["nnz_c"], st["nnz_a"], st["nnz_out"]) == (len(c[1]), len(a[1]), len(wc))
                no_work = m == 0 or n == 0 or (I is None and J is None and accum is None) or (accum is not None and len(a[1]) == 0)
                assert st["no_work"] == no_work and st["readbacks"] == (0 if no_work else 1), (rn, cn, accum)
                if not no_work:
                    Vc, Pcd = _dense_parts(c, M, NCOL)
                    ii, jj = (np.arange(M) if I is None else I), (np.arange(NCOL) if J is None else J)
                    assert st["nnz_region"] == int(Pcd[np.ix_(ii, jj)].sum()), (rn, cn, accum)
                    assert st["nnz_both"] == (int(both.sum()) if accum is not None else
                                              int((Pcd[np.ix_(ii, jj)] & _dense_parts(a, m, n)[1]).sum())), (rn, cn, accum)


def test_the_model_refuses_bad_lists_but_reads_none_in_a_no_work_shape():
    c = _csr(LENGTHS, NCOL, np.float64, 5)
    M = len(LENGTHS)
    one = _csr([2], 2, np.float64, 6, zeros=99)
    two = (np.array([0, 1, 2], np.int64), np.array([0, 1], np.uint32), np.ones(2))
    for a, n, kw in ((two, 2, {"rows": [3, 3], "cols": [1, 2]}), (two, 2, {"rows": [0, M], "cols": [1, 2]}), (one, 2, {"rows": [0], "cols": [5, 4]}),
                     (one, 2, {"rows": [0], "cols": [5, 5]}), (one, 2, {"rows": [0], "cols": [5, NCOL]}), (one, 2, {"rows": [0, 1], "cols": [1, 2]}),
                     (one, 2, {"rows": [0], "cols": [1, 2, 3]}), (one, 2, {"rows": [0]}), (one, 2, {"cols": [1, 2]})):
        with pytest.raises(ValueError):
            model.assign(c, NCOL, a, n, **kw)
    with pytest.raises(ValueError):
        model.assign(c, NCOL, one, 2, [0], [1, 2], "minus")
    # no-work shapes read no list
    none_rows = (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    assert model.assign(c, NCOL, none_rows, 2, rows=[], cols=[NCOL, 0])[2]["nnz_out"] == len(c[1])
    no_cols = (np.zeros(3, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    assert model.assign(c, NCOL, no_cols, 0, rows=[M, M], cols=[])[2]["no_work"]
    empty_a = (np.zeros(3, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    assert model.assign(c, NCOL, empty_a, 2, rows=[M, M], cols=[9, 3], accum="plus")[2]["no_work"]
    with pytest.raises(ValueError):      # without accum an empty a deletes the region: the lists are read
        model.assign(c, NCOL, empty_a, 2, rows=[M, M], cols=[9, 3])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_assign_and_extract_are_inverse(dt):
    c = _csr(LENGTHS, NCOL, dt, 7)
    M = len(LENGTHS)
    rows, cols = _lists(M, NCOL, np.random.default_rng(8))
    for rn, I in rows.items():
        for cn, J in cols.items():
            m, n = M if I is None else len(I), NCOL if J is None else len(J)
            # assign(extract(I, J), I, J) == c
            sub = extract_model.extract(*c, NCOL, I, J)[0]
            back = model.assign(c, NCOL, sub, n, I, J)[0]
            for got, want in zip(back, c):
                assert np.array_equal(_bits(got) if got.dtype == dt else got, _bits(want) if want.dtype == dt else want), (rn, cn)
            # extract(assign(a, I, J), I, J) == a
            a = _a_for(m, n, dt, 50 + m + n % 97)
            put = model.assign(c, NCOL, a, n, I, J)[0]
            again = extract_model.extract(*put, NCOL, I, J)[0]
            if m == 0 or n == 0:
                assert len(again[1]) == 0
                continue
            assert np.array_equal(again[0], a[0]) and np.array_equal(again[1], a[1]) and np.array_equal(_bits(again[2]), _bits(a[2])), (rn, cn)


@pytest.mark.parametrize("accum", [None, "plus"])
def test_the_composed_column_path_on_a_permuted_list(accum):
    c = _csr(LENGTHS, NCOL, np.float64, 9)
    rng = np.random.default_rng(10)
    I, J = np.array([9, 2, 7, 5]), rng.permutation(NCOL)[:900]
    a = _a_for(4, 900, np.float64, 11)
    (rowptr, col, val), _ = model.assign_any(c, NCOL, a, 900, I, J, accum)
    wp, wc, pc, pa = _scipy_assign(c, NCOL, a, I, J, accum)
    assert np.array_equal(rowptr, wp) and np.array_equal(col, wc)
    both = (pc >= 0) & (pa >= 0)
    want = np.where(pc >= 0, c[2][np.maximum(pc, 0)], 0.0)
    want[pa >= 0] = a[2][pa[pa >= 0]]
    want[both] = c[2][pc[both]] + a[2][pa[both]]
    assert np.array_equal(_bits(val), _bits(want))
    with pytest.raises(ValueError):      # a repeated column fails as not strictly ascending
        model.assign_any(c, NCOL, _a_for(4, 3, np.float64, 12), 3, I, [5, 2, 5], accum)
    # embed is the assign into nothing
    out = model.embed(a, 900, (len(LENGTHS), NCOL), I, J)
    assert np.array_equal(out[0], model.assign_any((np.zeros(len(LENGTHS) + 1, np.int64), c[1][:0], c[2][:0]), NCOL, a, 900, I, J)[0][0])
    assert len(out[1]) == len(a[1])


# ---- block matrices ------------------------------------------------------------------------------------------------------------------
def _as_scipy(b):
    (rowptr, col, val), ncol = b
    return sp.csr_matrix((np.arange(1, len(col) + 1, dtype=np.float64), col.astype(np.int64), rowptr), shape=(len(rowptr) - 1, ncol))


def test_the_block_matrix_model_is_scipys_bmat():
    def blk(m, n, seed):
        rng = np.random.default_rng(seed)
        return _csr([int(x) for x in rng.integers(0, n + 1, m)], max(n, 1), np.float64, seed) if n else \
            (np.zeros(m + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0)), n
    grids = {"2x2 with None": [[None, blk(5, 70, 1)], [blk(8, 3, 2), None]],
             "full 2x3": [[blk(4, 9, 3), blk(4, 1, 4), blk(4, 130, 5)], [blk(70, 9, 6), blk(70, 1, 7), blk(70, 130, 8)]],
             "a 0-wide block": [[blk(3, 0, 9), blk(3, 5, 10)], [None, blk(2, 5, 11)]],
             "1x1": [[blk(6, 6, 12)]],
             "a 0-high block": [[blk(0, 4, 13)], [blk(3, 4, 14)]]}
    for name, grid in grids.items():
        (rowptr, col, val), shape = model.block_matrix(grid)
        want = sp.csr_matrix(sp.bmat([[None if b is None else _as_scipy(b) for b in row] for row in grid], format="csr"))
        want.sort_indices()
        assert shape == want.shape, name
        assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices), name
        # scipy's data are positions: block by block in the grid's order within the sorted result
        flat = [b for row in grid for b in row if b is not None]
        assert len(val) == sum(len(b[0][1]) for b in flat), name
        assert sorted(_bits(val).tolist()) == sorted(np.concatenate([_bits(b[0][2]) for b in flat]).tolist()), name
    for bad in ([[None]], [[blk(2, 2, 1), None], [None, None]], [[blk(2, 2, 1)], [blk(3, 3, 2)]], []):
        with pytest.raises(ValueError):
            model.block_matrix(bad)


# ---- the models of the graph functions -------------------------------------------------------------------------------------------------
def _edge_set(csr):
    u = np.repeat(np.arange(len(csr[0]) - 1), np.diff(csr[0]))
    return set(zip(u.tolist(), csr[1].astype(np.int64).tolist()))


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_bipartite_model_is_networkx(name):
    n, r, c = GRAPHS[name]
    m, k = n, n // 2
    cc = c % k                                               # an m x k biadjacency with repeated edges
    w = np.random.default_rng(13).integers(1, 9, len(r)).astype(np.float64)
    out = model.bipartite_adjacency(r, cc, (m, k), w)
    B = sp.csr_matrix((w, (r, cc)), shape=(m, k))            # (repeats summed)
    G = bipartite.from_biadjacency_matrix(B)
    want = {}
    for a, b, d in G.edges(data=True):
        want[(a, b)] = want[(b, a)] = d["weight"]
    assert len(out[0]) == m + k + 1 and _edge_set(out) == set(want)
    u = np.repeat(np.arange(m + k), np.diff(out[0]))
    assert all(want[(a, b)] == v for a, b, v in zip(u.tolist(), out[1].tolist(), out[2].tolist()))


def test_the_disjoint_union_model_is_networkx():
    graphs = [GRAPHS["rmat8"], GRAPHS["rmat10"], (0, np.zeros(0, np.int64), np.zeros(0, np.int64)), (4, np.zeros(0, np.int64), np.zeros(0, np.int64)),
              GRAPHS["rmat8"]]
    nxg = []
    for n, r, c in graphs:
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from((int(a), int(b)) for a, b in zip(r, c) if a != b)
        nxg.append(G)
    U = nx.disjoint_union_all(nxg)
    out, offsets = model.disjoint_union([(r, c, n) for n, r, c in graphs])
    assert offsets.tolist() == [0, 256, 1280, 1280, 1284, 1540] and len(out[0]) == U.number_of_nodes() + 1
    assert _edge_set(out) == {(a, b) for a, b in U.edges()} | {(b, a) for a, b in U.edges()}
    assert model.disjoint_union([])[1].tolist() == [0]


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_replace_subgraph_model_is_networkx(name, directed):
    n, r, c = GRAPHS[name]
    rng = np.random.default_rng(14)
    G = (nx.DiGraph if directed else nx.Graph)()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(r, c) if directed or a != b)
    for V in (rng.permutation(n)[:n // 3], np.sort(rng.choice(n, n // 2, replace=False)), np.array([5]), np.zeros(0, np.int64), np.arange(n)):
        k = len(V)
        sr, sc = (rng.integers(0, k, 3 * k), rng.integers(0, k, 3 * k)) if k else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        u, v = model.replace_subgraph(n, r, c, V, sr, sc, directed)
        H = G.copy()
        inside = set(V.tolist())
        H.remove_edges_from([(a, b) for a, b in G.edges() if a in inside and b in inside])
        H.add_edges_from((int(V[a]), int(V[b])) for a, b in zip(sr, sc) if directed or a != b)
        want = sorted((a, b) if directed else (min(a, b), max(a, b)) for a, b in H.edges())
        assert list(zip(u.tolist(), v.tolist())) == want
        # the inverse of induced_subgraph: putting back what was cut out changes nothing
        iu, iv = extract_model.induced_subgraph(n, r, c, V, directed)
        u, v = model.replace_subgraph(n, r, c, V, iu, iv, directed)
        assert list(zip(u.tolist(), v.tolist())) == sorted((a, b) if directed else (min(a, b), max(a, b)) for a, b in G.edges())
    for bad in ([1, 2, 1], [n], [-1]):
        with pytest.raises(ValueError):
            model.replace_subgraph(n, r, c, bad, [0], [0], directed)
