"""CPU-side checks of the semiring product at a mask (include/outerspace_spgemm_mxm_masked.h) and of graph.bfs_parents: the
symbol is exported and listed, the stats struct has the layout the C compiler gives it, null arguments are argument errors
that leave the outputs alone, the Python entries validate their arguments before they need a GPU, and the models that judge
the GPU (tests/mxm_masked_model.py) equal things that share nothing with them: a dense brute force of three loops, and
breadth-first trees written down by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import mxm_masked_model as model
from tests import semiring_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_mxm_masked.h")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_mxm_masked_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.MXM_MASKED_EXPORTS) == {"osp_csr_mxm_masked"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS, _lib.TRANSPOSE_EXPORTS, _lib.MXV_EXPORTS, _lib.MXV_ARG_EXPORTS, _lib.MXD_EXPORTS,
                  _lib.SDDMM_EXPORTS, _lib.EXTRACT_EXPORTS, _lib.BUILD_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm_mxm.h"' in hdr
    assert set(re.findall(r"\btypedef struct (\w+)", hdr)) == {"osp_mxm_masked_stats"}


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


def test_mxm_masked_stats_have_the_layout_the_c_compiler_gives(tmp_path):
    cname, struct = "osp_mxm_masked_stats_t", _lib.MxmMaskedStats
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_mxm_masked.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    assert list(struct().as_dict()) == ["nnz_a", "nnz_b", "nnz_mask", "products", "products_kept", "nnz_out", "short_rows", "long_rows",
                                        "batches", "launches", "ms_total"]
    # the plain product's struct is what it was
    assert list(_lib.MxmStats().as_dict()) == ["nnz_a", "nnz_b", "products", "nnz_out", "short_rows", "long_rows", "batches", "launches",
                                               "ms_total"]


def test_mxm_masked_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call has a null among a, b, mask, sr and out, and the null checks
    come before any handle is touched, so the others may be fakes (tests/test_gpu_mxm_masked.py passes the other bad
    arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.MxmMaskedStats()
    stats.products_kept = 77
    sr = _lib.Semiring()
    sr.add, sr.mul = _lib.MXM_ADD_OPS["min"], _lib.MXM_MUL_OPS["first"]
    bad = _lib.Semiring()
    bad.add, bad.mul = _lib.EWISE_OPS["div"], _lib.EWISE_OPS["minus"]
    fake = ctypes.c_void_p(0x1000)
    o, st, s = ctypes.byref(out), ctypes.byref(stats), ctypes.byref(sr)
    calls = [lambda: L.osp_csr_mxm_masked(None, fake, fake, 0, s, o, st),
             lambda: L.osp_csr_mxm_masked(fake, None, fake, 1, s, o, st),
             lambda: L.osp_csr_mxm_masked(fake, fake, None, 0, s, o, st),
             lambda: L.osp_csr_mxm_masked(fake, fake, fake, 1, None, o, st),
             lambda: L.osp_csr_mxm_masked(fake, fake, fake, 0, s, None, st),
             lambda: L.osp_csr_mxm_masked(None, None, None, 0, ctypes.byref(bad), o, st),
             lambda: L.osp_csr_mxm_masked(None, None, None, 1, None, None, None)]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.products_kept == 77


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_entries_exist_and_validate_before_they_need_a_gpu():
    assert callable(graph.bfs_parents)
    res = object.__new__(S.CsrResult)   # (no handle: the names are checked before anything is touched)
    res._h, res._ctx, res.shape, res.dtype = None, object(), (3, 3), np.float64
    with pytest.raises(ValueError):
        res.mxm(res, complement=True)                      # a sense without a mask
    for kw in ({"add": "times"}, {"mul": "minus"}, {"add": "argmin"}):
        with pytest.raises(ValueError):
            res.mxm(res, mask=res, **kw)
    with pytest.raises(TypeError):
        res.mxm(res, mask=(np.zeros(4, np.int64), np.zeros(0, np.uint32)))
    with pytest.raises(TypeError):
        res.mxm(res, "plus", "times", res)                 # mask and complement are keywords
    foreign = object.__new__(S.CsrResult)
    foreign._h, foreign._ctx, foreign.shape, foreign.dtype = None, object(), (3, 3), np.float64
    with pytest.raises(S.OspError) as ei:
        res.mxm(res, mask=foreign)
    assert ei.value.status == _lib.ERR_ARG
    for r in (res, foreign):
        r._ctx = None    # (nothing to close)


# ---- the model of the masked product -----------------------------------------------------------------------------------------------
def _random_dense(rng, shape, density, dtype):
    has = rng.random(shape) < density
    val = rng.integers(-4, 5, shape).astype(dtype)          # (zeros among them: an explicit zero is an entry)
    return has, np.where(has, val, 0).astype(dtype)


@pytest.mark.parametrize("complement", [False, True])
def test_the_model_is_a_dense_brute_force_on_12_by_9_by_11(complement):
    rng = np.random.default_rng(12)
    hasA, A = _random_dense(rng, (12, 9), 0.4, np.float64)
    hasB, B = _random_dense(rng, (9, 11), 0.4, np.float64)
    hasM, _ = _random_dense(rng, (12, 11), 0.5, np.float64)
    hasA[3], hasM[5], hasM[6] = False, False, True          # an empty row of a, an empty and a full row of the mask
    a, b = semiring_model._dense_to_csr(hasA, A), semiring_model._dense_to_csr(hasB, B)
    m = semiring_model._dense_to_csr(hasM, np.zeros((12, 11)))
    plain = semiring_model.mxm(a, b, 11)[1]
    seen = 0
    for add, mul in (("plus", "times"), ("min", "plus"), ("max", "min"), ("first", "second"), ("min", "first")):
        (rowptr, col, val), st = model.mxm_masked(a, b, m, 11, complement, add, mul)
        has, out = model.dense_masked(A, hasA, B, hasB, hasM, complement, add, mul)
        want = semiring_model._dense_to_csr(has, out)
        assert np.array_equal(rowptr, want[0]) and np.array_equal(col, want[1])
        assert np.array_equal(val.view(np.uint64), want[2].view(np.uint64)), (add, mul)
        # products_kept by hand: the k common to A's row and B's column, at every admitted coordinate
        common = hasA.astype(np.int64) @ hasB.astype(np.int64)
        assert st["products_kept"] == int(common[hasM != complement].sum())
        assert st["products"] == int(common.sum()) == plain["products"] and st["nnz_mask"] == int(hasM.sum())
        assert (st["short_rows"], st["long_rows"], st["batches"]) == (plain["short_rows"], plain["long_rows"], plain["batches"])
        seen += st["nnz_out"]
    assert seen > 0


def test_the_two_senses_partition_the_product():
    rng = np.random.default_rng(5)
    hasA, A = _random_dense(rng, (12, 9), 0.5, np.float32)
    hasB, B = _random_dense(rng, (9, 11), 0.5, np.float32)
    hasM, _ = _random_dense(rng, (12, 11), 0.5, np.float32)
    a, b = semiring_model._dense_to_csr(hasA, A), semiring_model._dense_to_csr(hasB, B)
    m = semiring_model._dense_to_csr(hasM, np.zeros((12, 11), np.float32))
    full, fst = semiring_model.mxm(a, b, 11)
    (_, c0, _), s0 = model.mxm_masked(a, b, m, 11, False)
    (_, c1, _), s1 = model.mxm_masked(a, b, m, 11, True)
    assert len(c0) + len(c1) == len(full[1]) == fst["nnz_out"] and s0["products_kept"] + s1["products_kept"] == fst["products"]
    empty = (np.zeros(13, np.int64), np.zeros(0, np.uint32))
    assert model.mxm_masked(a, b, empty, 11, False)[1]["nnz_out"] == 0
    got = model.mxm_masked(a, b, empty, 11, True)[0]
    assert all(np.array_equal(x, y) for x, y in zip(got, full))


# ---- the model of the parent trees ---------------------------------------------------------------------------------------------------
def test_the_bfs_model_on_a_path():
    r, c = np.arange(5), np.arange(1, 6)
    parent, level, deepest = model.bfs_parents(r, c, 6, [0, 3])
    assert parent.tolist() == [[0, 0, 1, 2, 3, 4], [1, 2, 3, 3, 3, 4]]
    assert level.tolist() == [[0, 1, 2, 3, 4, 5], [3, 2, 1, 0, 1, 2]] and deepest == 5
    parent, level, deepest = model.bfs_parents(r, c, 6, [0], max_levels=2)
    assert parent.tolist() == [[0, 0, 1, -1, -1, -1]] and level.tolist() == [[0, 1, 2, -1, -1, -1]] and deepest == 2


def test_the_bfs_model_on_a_star():
    r, c = np.zeros(5, np.int64), np.arange(1, 6)
    parent, level, deepest = model.bfs_parents(r, c, 6, [0, 4])
    assert parent.tolist() == [[0, 0, 0, 0, 0, 0], [4, 0, 0, 0, 4, 0]]
    assert level.tolist() == [[0, 1, 1, 1, 1, 1], [1, 2, 2, 2, 0, 2]] and deepest == 2


def test_the_bfs_model_on_two_components_takes_the_smallest_parent():
    # a square 0-1, 0-2, 1-3, 2-3 (vertex 3 has the parents 1 and 2: the smaller wins), an edge 4-5, the isolated vertex 6
    r, c = np.array([0, 0, 1, 2, 4, 3]), np.array([1, 2, 3, 3, 5, 3])      # (a self loop at 3 is dropped)
    parent, level, deepest = model.bfs_parents(r, c, 7, [0, 5, 6])
    assert parent.tolist() == [[0, 0, 0, 1, -1, -1, -1], [-1, -1, -1, -1, 5, 5, -1], [-1, -1, -1, -1, -1, -1, 6]]
    assert level.tolist() == [[0, 1, 1, 2, -1, -1, -1], [-1, -1, -1, -1, 1, 0, -1], [-1, -1, -1, -1, -1, -1, 0]] and deepest == 2


def test_the_bfs_model_on_a_directed_cycle():
    r, c = np.arange(4), (np.arange(4) + 1) % 4
    parent, level, deepest = model.bfs_parents(r, c, 4, [2], directed=True)
    assert parent.tolist() == [[3, 0, 2, 2]] and level.tolist() == [[2, 3, 0, 1]] and deepest == 3
    parent, level, _ = model.bfs_parents(r, c, 4, [2])                       # undirected: both ways round
    assert parent.tolist() == [[1, 2, 2, 2]] and level.tolist() == [[2, 1, 0, 1]]
