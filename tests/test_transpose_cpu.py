"""CPU-side checks of the transpose of a result (include/outerspace_spgemm_transpose.h) and of what is built on it: the symbol
is exported and listed, both structs have the layout the C compiler gives them, null arguments are argument errors that leave
the outputs alone, the Python entries exist and fail loudly without a GPU, and the models that judge the GPU
(tests/transpose_model.py) equal scipy: the transpose on a hand-written matrix bit for bit, the components on six graphs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import connected_components

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import transpose_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_transpose.h")
GRAPHS = model.graphs()


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def test_transpose_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.TRANSPOSE_EXPORTS) == {"osp_csr_transpose"}
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS, _lib.APPLY_MASK_EXPORTS, _lib.SELECT_EXPORTS, _lib.EWISE_EXPORTS,
                  _lib.VECTOR_EXPORTS, _lib.MXM_EXPORTS):
        assert not declared & set(other)
    assert '#include "outerspace_spgemm.h"' in hdr
    # the model's pass count is the sort's: 8-bit digits, and the row-mask path ends at 64 rows
    src = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_transpose.h")).read()
    assert int(re.search(r"kTrMaskRows\s*=\s*(\d+)", src).group(1)) == 64
    assert [model.passes(n) for n in (0, 1, 2, 256, 257, 65536, 65537, (1 << 24) + 3)] == [1, 1, 1, 1, 2, 2, 3, 4]


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_transpose_t", _lib.Transpose), ("osp_transpose_stats_t", _lib.TransposeStats)])
def test_transpose_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_transpose.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_transpose_stats_dict():
    assert set(_lib.TransposeStats().as_dict()) == {"nnz", "path", "passes", "launches", "ms_total"}


def test_transpose_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: a null `in`, alone and with the other pointers null
    (tests/test_gpu_transpose.py passes the other bad arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.TransposeStats()
    stats.nnz = 77
    tp = _lib.Transpose()
    fake = ctypes.c_void_p(0)
    calls = [lambda: L.osp_csr_transpose(None, ctypes.byref(tp), ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_transpose(fake, None, ctypes.byref(out), ctypes.byref(stats)),
             lambda: L.osp_csr_transpose(None, None, None, ctypes.byref(stats)),
             lambda: L.osp_csr_transpose(None, ctypes.byref(tp), ctypes.byref(out), None)]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz == 77


def test_python_entries_exist():
    assert callable(S.CsrResult.transpose) and callable(S.CsrResult.matmul)
    for name in ("strongly_connected", "cocitation", "bibliographic_coupling"):
        assert callable(getattr(graph, name))


def test_directed_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.strongly_connected(r, c), lambda: graph.cocitation(r, c), lambda: graph.bibliographic_coupling(r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_model_is_scipys_transpose_bit_for_bit(dt):
    """4 x 6: row 2 is empty, column 3 is empty; a NaN with a payload, -0.0, both infinities and an explicit +0.0."""
    nan = np.array([0x7fc00123], np.uint32).view(np.float32)[0] if dt == np.float32 else \
        np.array([0x7ff8000000abcdef], np.uint64).view(np.float64)[0]
    rowptr = np.array([0, 3, 5, 5, 9], np.int64)
    col = np.array([0, 2, 5, 1, 2, 0, 1, 4, 5], np.uint32)
    val = np.array([1.5, nan, -0.0, np.inf, -np.inf, 0.0, 2.0, -3.0, 4.0], dt)
    got = model.transpose(rowptr, col, val, 6)
    T = sp.csr_matrix((val, col.astype(np.int64), rowptr), shape=(4, 6)).T.tocsr()
    T.sort_indices()
    assert T.nnz == 9                                         # (scipy kept the explicit zeros)
    assert np.array_equal(got[0], T.indptr) and np.array_equal(got[1], T.indices)
    assert got[2].dtype == dt and np.array_equal(_bits(got[2]), _bits(T.data))
    assert got[0][3] == got[0][4] and got[0].tolist() == [0, 2, 4, 6, 6, 7, 9]
    back = model.transpose(*got, 4)
    assert np.array_equal(back[0], rowptr) and np.array_equal(back[1], col) and np.array_equal(_bits(back[2]), _bits(val))


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_component_model_is_scipys_strong_components(name):
    n, r, c = GRAPHS[name]
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    _, label = connected_components(sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n)), directed=True, connection="strong")
    sources = np.arange(n) if n <= 64 else np.random.default_rng(1).choice(n, 64, replace=False)
    member, info = model.strongly_connected(r, c, n, sources)
    assert member.shape == (len(sources), n)
    assert np.array_equal(member, label[sources][:, None] == label[None, :])
    assert member[np.arange(len(sources)), sources].all()
    assert info["nnz_forward"] >= member.sum() <= info["nnz_backward"]
    # one round reaches the neighbours only
    cut, cinfo = model.strongly_connected(r, c, n, sources, max_iter=1)
    assert cinfo["rounds_forward"] <= 1 and not (cut & ~member).any()
