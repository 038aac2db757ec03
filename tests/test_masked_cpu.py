"""CPU-side checks of the masked product's boundary (include/outerspace_spgemm_masked.h): its symbols are exported and
listed, a null handle is an argument error, without a GPU the Python entry fails loudly, and the graph plumbing of
triangle_count builds the L that scipy builds."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masked_header_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "outerspace_spgemm_masked.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.MASKED_EXPORTS)
    assert not declared & set(_lib.EXPORTS)


def test_masked_version_is_7():
    hdr = open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read()
    assert re.search(r"#define OSP_VERSION 7\b", hdr)


def test_masked_null_context_is_an_argument_error():
    L = _lib.lib()
    colptr = np.zeros(3, np.int64)
    out = ctypes.c_void_p()
    cfg = _lib.Config()
    L.osp_config_default(ctypes.byref(cfg))
    p = ctypes.c_void_p(colptr.ctypes.data)
    st = L.osp_spgemm_masked(None, _lib.OSP_F64, 2, 2, 2, p, None, None, p, None, None, p, None, _lib.OSP_HOST, ctypes.byref(cfg),
                             ctypes.byref(out))
    assert st == _lib.ERR_ARG
    assert L.osp_last_error_string()
    assert out.value is None


def test_masked_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    A = sp.random(4, 5, density=0.5, random_state=0, format="csr")
    with pytest.raises(S.OspError) as ei:
        S.spgemm_masked(A, A, sp.eye(4, format="csr"))
    assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)
    with pytest.raises(S.OspError):
        graph.triangle_count(np.array([0, 1, 2]), np.array([1, 2, 0]))


def _scipy_oriented(rows, cols, n):
    """The same L in scipy and numpy: symmetric pattern without loops, rank by (degree, id), keep rank u < rank v."""
    A = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    A = A + A.T
    A.setdiag(0)
    A.eliminate_zeros()
    A = (A != 0).astype(np.int64).tocoo()
    deg = np.bincount(A.row, minlength=n)
    order = np.lexsort((np.arange(n), deg))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    ru, rv = rank[A.row], rank[A.col]
    keep = ru < rv
    return sp.csr_matrix((np.ones(int(keep.sum())), (ru[keep], rv[keep])), shape=(n, n))


@pytest.mark.parametrize("seed", range(6))
def test_oriented_adjacency_matches_scipy(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    m = int(rng.integers(0, 4 * n))
    rows = rng.integers(0, n, m)
    cols = rng.integers(0, n, m)
    if seed == 0 and m:
        cols[: m // 2] = 0          # a hub
    rows_t, cols_t = torch.from_numpy(rows), torch.from_numpy(cols)
    nn, rowptr, colidx, colptr, rowidx = graph.oriented_adjacency(rows_t, cols_t, n)
    assert nn == n and rowptr.device.type == "cpu"
    want = _scipy_oriented(rows, cols, n)
    want.sort_indices()
    assert np.array_equal(rowptr.numpy(), want.indptr)
    assert np.array_equal(colidx.numpy(), want.indices)
    wc = want.tocsc()
    wc.sort_indices()
    assert np.array_equal(colptr.numpy(), wc.indptr)
    assert np.array_equal(rowidx.numpy(), wc.indices)
    # every row has at most sqrt(2m) entries, m the undirected edge count
    deg = np.diff(rowptr.numpy())
    assert deg.max(initial=0) <= np.sqrt(2 * want.nnz) + 1e-9
    # oriented: no edge in both directions, no loop, and L + L^T is the simple graph's pattern
    D = (want + want.T).toarray()
    assert np.all(np.diag(D) == 0) and D.max(initial=0) <= 1


def test_oriented_adjacency_rejects_out_of_range_ids():
    with pytest.raises(ValueError):
        graph.oriented_adjacency(torch.tensor([0, 5]), torch.tensor([1, 2]), n=4)
