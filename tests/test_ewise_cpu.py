"""CPU-side checks of the element-wise union / intersection's boundary (include/outerspace_spgemm_ewise.h) and of the models
that judge the GPU (tests/ewise_model.py): the symbol is exported and listed, both structs have the layout the C compiler
gives them, null arguments are argument errors, the model agrees with scipy on a hand-written pair, and the model's
personalised PageRank agrees with networkx's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import bfs_model
from tests import ewise_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_ewise.h")


def test_ewise_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    assert declared
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.EWISE_EXPORTS)
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS):
        assert not declared & set(other)
    # the enums' values are the binding's, and the model's order
    names = dict((name.lower(), int(v)) for name, v in re.findall(r"OSP_EWISE_([A-Z]+)\s*=\s*(\d+)", hdr))
    modes = {k: v for k, v in names.items() if k in ("union", "intersect")}
    ops = {k: v for k, v in names.items() if k not in modes}
    assert modes == _lib.EWISE_MODES and list(modes) == model.MODES
    assert ops == _lib.EWISE_OPS and list(ops) == model.OPS and sorted(ops.values()) == list(range(8))


@pytest.mark.parametrize("cname,struct", [("osp_ewise_t", _lib.Ewise), ("osp_ewise_stats_t", _lib.EwiseStats)])
def test_ewise_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_ewise.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_ewise_stats_dict():
    assert set(_lib.EwiseStats().as_dict()) == {"nnz_a", "nnz_b", "nnz_both", "nnz_out", "ms_total", "launches"}


def test_ewise_null_arguments_are_argument_errors():
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.EwiseStats()
    stats.nnz_a = 77
    ew = _lib.Ewise()
    # without a device there is no result to pass as an operand: null operands, alone and with a null ew or out
    # (tests/test_gpu_ewise.py passes a null ew and a null out with real results)
    for args in ((None, None, ctypes.byref(ew), ctypes.byref(out), ctypes.byref(stats)),
                 (None, None, None, ctypes.byref(out), ctypes.byref(stats)),
                 (None, None, ctypes.byref(ew), None, ctypes.byref(stats)),
                 (None, None, ctypes.byref(ew), ctypes.byref(out), None)):
        assert L.osp_csr_ewise(*args) == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_a == 77


def test_pagerank_fails_loudly_without_a_gpu_and_checks_its_arguments_first():
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for kw in ({"alpha": 0.0}, {"alpha": 1.0}, {"alpha": -0.5}, {"tol": 0.0}):
        with pytest.raises(ValueError):
            graph.personalized_pagerank(r, c, **kw)
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(S.OspError) as ei:
        graph.personalized_pagerank(r, c)
    assert ei.value.status == _lib.ERR_HIP


def test_step_count_is_the_smallest_k_whose_tail_is_below_tol():
    for alpha, tol in ((0.85, 1e-6), (0.5, 1e-3), (0.99, 1e-2), (0.85, 0.9), (0.1, 1e-12)):
        k = graph.ppr_steps(alpha, tol)
        assert k == model.ppr_steps(alpha, tol)
        assert alpha ** (k + 1) < tol and (k == 0 or alpha ** k >= tol)
    assert graph.ppr_steps(0.85, 1e-6) == 85
    assert graph.ppr_steps(0.85, 1e-6, max_iter=30) == model.ppr_steps(0.85, 1e-6, 30) == 30
    assert graph.ppr_steps(0.85, 1e-6, max_iter=0) == 0


# ---- the model on a hand-written pair against scipy ------------------------------------------------------------------------
# 4 x 8; row 1 is empty in a, row 2 in b, row 3 in both; (0, 1), (0, 5) and (2, ...) one-sided, (0, 2), (0, 7), (1, ...) mixed
_A = (np.array([0, 4, 4, 6, 6]), np.array([1, 2, 5, 7, 0, 3], np.uint32), np.array([1.5, -2.0, 4.0, 0.25, 3.0, -1.0]))
_B = (np.array([0, 3, 5, 5, 5]), np.array([0, 2, 7, 3, 4], np.uint32), np.array([8.0, 2.0, -0.5, 6.0, 7.0]))
_NCOL = 8


def _scipy(t):
    return sp.csr_matrix((t[2], t[1].astype(np.int64), t[0]), shape=(len(t[0]) - 1, _NCOL))


def _dense(t):
    return _scipy(t).toarray()


def test_model_on_a_hand_written_pair_against_scipy():
    A, B = _scipy(_A), _scipy(_B)
    pa, pb = A.toarray() != 0, B.toarray() != 0
    rp, c, v = model.ewise(_A, _B, _NCOL, "union", "plus")
    assert rp.tolist() == [0, 5, 7, 9, 9] and c.tolist() == [0, 1, 2, 5, 7, 3, 4, 0, 3]
    assert np.array_equal(_dense((rp, c, v)), (A + B).toarray())
    assert v[2] == 0.0        # -2 + 2: a computed zero stays an entry
    rp, c, v = model.ewise(_A, _B, _NCOL, "intersect", "times")
    assert rp.tolist() == [0, 2, 2, 2, 2] and c.tolist() == [2, 7] and v.tolist() == [-4.0, -0.125]
    assert np.array_equal(_dense((rp, c, v)), A.multiply(B).toarray())
    # max / min: scipy's treat an absent entry as 0, the model's union keeps the one-sided value: they agree where both hold
    # the coordinate, and the model's one-sided entries are the operand's own
    for op, ref in (("max", A.maximum(B)), ("min", A.minimum(B))):
        d = _dense(model.ewise(_A, _B, _NCOL, "union", op))
        both = pa & pb
        assert np.array_equal(d[both], ref.toarray()[both])
        assert np.array_equal(d[pa & ~pb], A.toarray()[pa & ~pb]) and np.array_equal(d[pb & ~pa], B.toarray()[pb & ~pa])
        di = _dense(model.ewise(_A, _B, _NCOL, "intersect", op))
        assert np.array_equal(di[both], ref.toarray()[both]) and not di[~both].any()
    assert model.ewise(_A, _B, _NCOL, "intersect", "minus")[2].tolist() == [-4.0, 0.75]
    assert model.ewise(_A, _B, _NCOL, "intersect", "div")[2].tolist() == [-1.0, -0.5]
    assert model.ewise(_A, _B, _NCOL, "union", "first")[2].tolist() == [8.0, 1.5, -2.0, 4.0, 0.25, 6.0, 7.0, 3.0, -1.0]
    assert model.ewise(_A, _B, _NCOL, "union", "second")[2].tolist() == [8.0, 1.5, 2.0, 4.0, -0.5, 6.0, 7.0, 3.0, -1.0]
    for op in ("minus", "div"):
        with pytest.raises(ValueError):
            model.ewise(_A, _B, _NCOL, "union", op)
    # nnz(union) + nnz(intersect) = nnz(a) + nnz(b), and a with itself
    assert len(model.ewise(_A, _B, _NCOL, "union", "plus")[1]) + len(model.ewise(_A, _B, _NCOL, "intersect", "plus")[1]) == 11
    rp, c, v = model.ewise(_A, _A, _NCOL, "union", "plus")
    assert np.array_equal(rp, _A[0]) and np.array_equal(c, _A[1]) and np.array_equal(v, 2 * _A[2])


def test_model_min_max_keep_a_with_a_nan_on_either_side():
    nan = np.array([0x7ff8000000000abc], np.uint64).view(np.float64)[0]
    a = (np.array([0, 2]), np.array([0, 1], np.uint32), np.array([nan, 1.0]))
    b = (np.array([0, 2]), np.array([0, 1], np.uint32), np.array([2.0, nan]))
    for op in ("min", "max"):
        v = model.ewise(a, b, 2, "intersect", op)[2]
        assert np.array_equal(v.view(np.uint64), a[2].view(np.uint64))


def test_model_pagerank_against_networkx():
    import networkx as nx
    G = nx.karate_club_graph()
    n = G.number_of_nodes()
    e = np.array(G.edges())
    adj = bfs_model.symmetric_adjacency(e[:, 0], e[:, 1], n)
    sources = [0, 33, 5, 0]
    got, info = model.ppr(adj, sources, alpha=0.85, tol=1e-12)
    assert info["steps"] == info["iterations"] == model.ppr_steps(0.85, 1e-12) and 0.85 ** (info["steps"] + 1) < 1e-12
    H = nx.Graph(G)
    for u, v in H.edges():
        H[u][v].clear()      # unit weights
    for i, s in enumerate(sources):
        want = nx.pagerank(H, alpha=0.85, personalization={s: 1.0}, tol=1e-14, max_iter=2000, weight=None)
        w = np.array([want[v] for v in range(n)])
        # the series' tail is below 1e-12 in all; networkx stops at an L1 step below n * 1e-14
        assert np.abs(got[i] - w).sum() < 1e-11, (s, np.abs(got[i] - w).sum())
    assert np.array_equal(got[0], got[3])
    assert np.allclose(got.sum(1), 1 - 0.85 ** (info["steps"] + 1), rtol=1e-13)


def test_model_pagerank_isolated_source_and_pruning():
    adj = bfs_model.symmetric_adjacency([0, 1], [1, 2], 5)       # a path 0-1-2, vertices 3 and 4 isolated
    got, info = model.ppr(adj, [3, 1], alpha=0.5, tol=1e-3)
    assert got[0].tolist() == [0, 0, 0, 0.5, 0] and abs(got[1].sum() - (1 - 0.5 ** (info["steps"] + 1))) < 1e-15
    pruned, pinfo = model.ppr(adj, [1], alpha=0.5, tol=1e-3, prune=0.1)
    assert pinfo["iterations"] < pinfo["steps"] and pinfo["frontiers"][-1].nnz == 0     # ended early: F became empty
    assert pruned.sum() < got[1].sum()
