"""CPU-side checks of the mask filter's boundary (include/outerspace_spgemm_apply_mask.h) and of the traversals built on it:
the symbol is exported and listed, the stats struct has the layout the C compiler gives it, null arguments are argument
errors, without a GPU the Python entries fail loudly, the graph plumbing builds the adjacency scipy builds, and the models
that judge the GPU (tests/bfs_model.py) agree with scipy's shortest paths and networkx's betweenness."""
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
from tests import bfs_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_apply_mask.h")


def test_apply_mask_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    assert declared
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.APPLY_MASK_EXPORTS)
    for other in (_lib.EXPORTS, _lib.MASKED_EXPORTS, _lib.MCL_EXPORTS):
        assert not declared & set(other)


def test_apply_mask_stats_have_the_layout_the_c_compiler_gives(tmp_path):
    fields = [name for name, _ in _lib.ApplyMaskStats._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_apply_mask.h"\n'
                   'int main(void) { printf("%zu", sizeof(osp_apply_mask_stats_t));\n'
                   + "".join(f'    printf(" %zu", offsetof(osp_apply_mask_stats_t, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.ApplyMaskStats)] + [getattr(_lib.ApplyMaskStats, f).offset for f in fields]
    assert set(_lib.ApplyMaskStats().as_dict()) == {"nnz_in", "nnz_mask", "nnz_out", "ms_total", "launches"}


def test_apply_mask_null_arguments_are_argument_errors():
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.ApplyMaskStats()
    stats.nnz_in = 77
    rowptr = np.zeros(5, np.int64)
    rp = ctypes.c_void_p(rowptr.ctypes.data)
    # without a device there is no result to pass as `in`: a null `in`, alone and with a null out (tests/test_gpu_apply_mask.py
    # passes a null out and a null mask with a real result)
    for args in ((None, 4, 4, rp, None, _lib.OSP_HOST, 0, 0, ctypes.byref(out), ctypes.byref(stats)),
                 (None, 4, 4, rp, None, _lib.OSP_HOST, 1, 1, None, ctypes.byref(stats)),
                 (None, 4, 4, None, None, _lib.OSP_DEVICE, 0, 0, ctypes.byref(out), None)):
        assert L.osp_csr_apply_mask(*args) == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77


def test_traversals_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.bfs_levels(r, c, sources=[0]), lambda: graph.betweenness_centrality(r, c)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


@pytest.mark.parametrize("seed", range(6))
def test_symmetric_adjacency_matches_scipy(seed):
    rng = np.random.default_rng(200 + seed)
    n = int(rng.integers(1, 40))
    m = int(rng.integers(0, 5 * n))
    rows = rng.integers(0, n, m)
    cols = rng.integers(0, n, m)
    if seed == 0 and m:
        cols[: m // 2] = 0          # a hub
    if m > 4:
        rows[-2:], cols[-2:] = rows[:2], cols[:2]      # duplicates in the same direction
        rows[-4:-2], cols[-4:-2] = cols[2:4], rows[2:4]  # and in the other
    nn, rowptr, colidx, vals = graph.symmetric_adjacency(torch.from_numpy(rows), torch.from_numpy(cols), n)
    assert nn == n and rowptr.device.type == "cpu" and vals.dtype == torch.float64
    # scipy's A + A.T with the diagonal removed and the values set to 1, built here and not by the model
    import scipy.sparse as sp
    A = sp.coo_matrix((np.ones(m), (rows, cols)), shape=(n, n)).tocsr()
    D = (A + A.T).toarray()
    np.fill_diagonal(D, 0)
    want = sp.csr_matrix((D != 0).astype(np.float64))
    want.sort_indices()
    assert np.array_equal(rowptr.numpy(), want.indptr)
    assert np.array_equal(colidx.numpy(), want.indices)
    assert np.array_equal(vals.numpy(), want.data)
    mod = model.symmetric_adjacency(rows, cols, n)
    assert np.array_equal(mod.indptr, want.indptr) and np.array_equal(mod.indices, want.indices) and np.array_equal(mod.data, want.data)
    # walk_pattern is the same graph with a loop on every vertex
    _, wp, wc, _ = graph.walk_pattern(torch.from_numpy(rows), torch.from_numpy(cols), n)
    assert np.array_equal(np.diff(wp.numpy()), np.diff(want.indptr) + 1)


def test_symmetric_adjacency_rejects_out_of_range_ids():
    with pytest.raises(ValueError):
        graph.symmetric_adjacency(torch.tensor([0, 5]), torch.tensor([1, 2]), n=4)


def _graphs():
    n, r, c = model.grid_edges(16, 16)
    yield "grid16", n, r, c
    n, r, c, _ = gen.rmat_coo(10, abcd="g500")
    yield "rmat10", n, r, c


@pytest.mark.parametrize("name,n,rows,cols", list(_graphs()), ids=lambda x: x if isinstance(x, str) else "")
def test_models_agree_with_scipy_and_networkx(name, n, rows, cols):
    import networkx as nx
    from scipy.sparse.csgraph import shortest_path
    adj = model.symmetric_adjacency(rows, cols, n)
    level, sigma, info = model.bfs_levels(adj, np.arange(n))
    dist = shortest_path(adj, unweighted=True)
    dist[np.isinf(dist)] = -1
    assert np.array_equal(level, dist.astype(np.int32))
    assert info["levels"] == int(dist.max()) and len(info["nnz_product"]) >= info["levels"]
    assert np.array_equal(sigma > 0, level >= 0)
    bc = model.brandes(adj)
    ref = nx.betweenness_centrality(nx.from_scipy_sparse_array(adj), normalized=False)
    want = 2.0 * np.array([ref[v] for v in range(n)])
    assert np.array_equal(bc == 0, want == 0)
    nz = want != 0
    assert nz.any()
    assert np.max(np.abs(bc[nz] - want[nz]) / want[nz]) <= 1e-12


def test_model_apply_mask_rules():
    rowptr = np.array([0, 3, 3, 5])
    col = np.array([1, 4, 7, 0, 9], np.uint32)
    val = np.array([1.0, -0.0, np.nan, 0.0, 5.0])
    m_rowptr = np.array([0, 2, 3, 5])
    m_col = np.array([0, 4, 2, 8, 9], np.uint32)
    rp, c, v = model.apply_mask(rowptr, col, val, m_rowptr, m_col, 10)
    assert rp.tolist() == [0, 1, 1, 2] and c.tolist() == [4, 9] and np.signbit(v[0]) and v[1] == 5.0
    rp, c, v = model.apply_mask(rowptr, col, val, m_rowptr, m_col, 10, complement=True)
    assert rp.tolist() == [0, 2, 2, 3] and c.tolist() == [1, 7, 0] and np.isnan(v[1])
