"""CPU-side checks of the Markov-clustering step's boundary (include/outerspace_spgemm_mcl.h): its symbol is exported and
listed, its structs have the sizes the C compiler gives them, null arguments are argument errors, without a GPU the Python
entry fails loudly, the graph plumbing builds the A + I that scipy builds, and the numpy model that judges the GPU
(tests/mcl_model.py) recovers planted partitions."""
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
from tests import mcl_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_mcl.h")


def test_mcl_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    assert declared
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.MCL_EXPORTS)
    assert not declared & set(_lib.EXPORTS)
    assert not declared & set(_lib.MASKED_EXPORTS)


def test_mcl_structs_have_the_sizes_the_c_compiler_gives(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_mcl.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(osp_mcl_step_t), sizeof(osp_mcl_stats_t),\n'
                   '    offsetof(osp_mcl_step_t, max_per_row), offsetof(osp_mcl_stats_t, chaos), offsetof(osp_mcl_stats_t, launches)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.MclStep), ctypes.sizeof(_lib.MclStats), _lib.MclStep.max_per_row.offset, _lib.MclStats.chaos.offset,
                   _lib.MclStats.launches.offset]


def test_mcl_null_arguments_are_argument_errors():
    L = _lib.lib()
    step = _lib.MclStep()
    step.power = 2.0
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    # without a device there is no result to pass as `in`: a null `in`, alone and with a null step / out (tests/test_gpu_mcl.py
    # passes a null step and a null out with a real result)
    for args in ((None, ctypes.byref(step), 0, ctypes.byref(out), None),
                 (None, None, 0, ctypes.byref(out), None),
                 (None, ctypes.byref(step), 0, None, None)):
        assert L.osp_csr_inflate_prune(*args) == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel


def test_mcl_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(S.OspError) as ei:
        graph.markov_cluster(np.array([0, 1, 2]), np.array([1, 2, 0]))
    assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("seed", range(5))
def test_walk_pattern_matches_scipy(seed, weighted):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 40))
    m = int(rng.integers(0, 5 * n))
    rows = rng.integers(0, n, m)
    cols = rng.integers(0, n, m)
    if seed == 0 and m:
        cols[: m // 2] = 0          # a hub
    if m > 4:
        rows[-2:], cols[-2:] = rows[:2], cols[:2]      # duplicates in the same direction
        rows[-4:-2], cols[-4:-2] = cols[2:4], rows[2:4]  # and in the other
    w = rng.random(m) + 0.1 if weighted else None
    nn, rowptr, colidx, vals = graph.walk_pattern(torch.from_numpy(rows), torch.from_numpy(cols), n, None if w is None else torch.from_numpy(w))
    assert nn == n and rowptr.device.type == "cpu" and vals.dtype == torch.float64
    want = model.walk_pattern(rows, cols, n, w)
    assert np.array_equal(rowptr.numpy(), want.indptr)
    assert np.array_equal(colidx.numpy(), want.indices)
    assert np.array_equal(vals.numpy(), want.data)
    # an independent scipy construction of the same thing
    D = np.zeros((n, n))
    for i, j, x in zip(rows, cols, np.ones(m) if w is None else w):
        if i != j:
            D[i, j] = max(D[i, j], x)
            D[j, i] = max(D[j, i], x)
    for i in range(n):
        D[i, i] = D[i].max() if (weighted and D[i].max() > 0) else 1.0
    assert np.array_equal(want.toarray(), D)
    assert np.all(np.diff(rowptr.numpy()) >= 1)          # every vertex has its loop


def test_walk_pattern_rejects_out_of_range_ids():
    with pytest.raises(ValueError):
        graph.walk_pattern(torch.tensor([0, 5]), torch.tensor([1, 2]), n=4)


def test_model_ordered_sum_is_the_defined_order():
    rng = np.random.default_rng(1)
    for m in (0, 1, 63, 64, 65, 200):
        e = rng.random(m).astype(np.float32)
        p = [np.float32(0)] * 64
        for i, x in enumerate(e):
            p[i % 64] = np.float32(p[i % 64] + x)
        d = 32
        while d:
            for l in range(d):
                p[l] = np.float32(p[l] + p[l + d])
            d //= 2
        assert model.ordered_sum(e) == p[0]


def test_model_step_rules():
    # row 0: cap 2 of [.3 .3 .3 .1]: the two lowest columns among the ties; row 1: nothing reaches the threshold: the largest,
    # lowest column first; row 2: empty; row 3: a value equal to the threshold stays, the next below it goes
    below = np.nextafter(0.25, 0)
    rowptr = np.array([0, 4, 7, 7, 9])
    col = np.array([1, 3, 5, 7, 0, 2, 4, 6, 8], np.uint32)
    val = np.array([.3, .3, .3, .1, .01, .02, .02, 0.25, below])
    rp, c, v, st = model.inflate_prune(rowptr, col, val, 1.0, 0.25, 2)
    assert rp.tolist() == [0, 2, 3, 3, 4]
    assert c.tolist() == [1, 3, 2, 6]
    assert v.tolist() == [0.5, 0.5, 1.0, 1.0]
    assert (st["rows_capped"], st["rows_rescued"], st["nnz_out"]) == (1, 1, 4)
    assert st["chaos"] == 0.0


@pytest.mark.parametrize("seed", range(4))
def test_model_recovers_planted_partition(seed):
    n, rows, cols, truth = model.planted_partition(seed)
    labels, info, (rp, ci, va) = model.markov_cluster(rows, cols, n)
    assert info["converged"] and info["iterations"] < 100
    assert np.array_equal(labels, truth)
    # converged: every row sums to 1 and holds equal weights on its attractors
    T = sp.csr_matrix((va, ci.astype(np.int64), rp), shape=(n, n))
    assert np.allclose(np.asarray(T.sum(1)).ravel(), 1.0, atol=1e-12)
