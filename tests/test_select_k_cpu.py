"""CPU-side checks of the row-wise k-select (include/outerspace_spgemm_select_k.h) and of what is built on it: the symbol is
exported and listed, both structs have the layout the C compiler gives them, null arguments are argument errors that leave
the outputs alone, the Python entries validate before they touch a handle and fail loudly without a GPU, and the models that
judge the GPU (tests/select_k_model.py) equal constructions that share nothing with them: a dense ``np.sort``, the
negation symmetry, the nesting property, chi-square statistics of the hash over 4000 fixed seeds, and ``np.argpartition``."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.stats
import torch

from outerspace_amd import _lib
from outerspace_amd import graph
from outerspace_amd import spgemm as S
from tests import select_k_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_select_k.h")
KERNELS = os.path.join(ROOT, "outerspace_amd", "csrc", "osp_select_k.h")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_select_k_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert declared == set(_lib.SELECT_K_EXPORTS) == {"osp_csr_select_k"}
    others = [name for name in dir(_lib) if name.endswith("EXPORTS") and name != "SELECT_K_EXPORTS"]
    assert len(others) >= 18
    for name in others:
        assert not declared & set(getattr(_lib, name)), name
    values = {name.lower(): int(v) for name, v in re.findall(r"OSP_SELECT_K_([A-Z]+) = (\d+)", hdr)}
    assert values == _lib.SELECT_K_ORDERS and tuple(values) == model.ORDERS
    # the class boundary: the kernels' header, the binding and the model agree
    src = open(KERNELS).read()
    assert int(re.search(r"kSelectKLongMin\s*=\s*(\d+)", src).group(1)) == _lib.SELECT_K_LONG_MIN == model.LONG_MIN
    assert int(re.search(r"kSelectKLongThreads\s*=\s*(\d+)", src).group(1)) == 256
    assert "OSP_SELECT_K" not in open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_settings.h")).read()   # no new setting


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_select_k_t", _lib.SelectK), ("osp_select_k_stats_t", _lib.SelectKStats)])
def test_select_k_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_select_k.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    if struct is _lib.SelectKStats:
        assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "rows_capped", "rows_long", "ms_total", "launches", "readbacks"}


def test_select_k_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in` (whatever else is wrong with it), and a fake
    operand with a null sk or out (the null checks come before an operand is touched; tests/test_gpu_select_k.py passes the
    other bad arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.SelectKStats()
    stats.nnz_in = 77
    ok = _lib.SelectK()
    ok.k = 3
    zero_k = _lib.SelectK()
    bad_order = _lib.SelectK()
    bad_order.order, bad_order.k = 3, 1
    bad_word = _lib.SelectK()
    bad_word.k, bad_word.reserved[7] = 1, 1
    fake = ctypes.c_void_p(0x1000)
    refs = (ctypes.byref(out), ctypes.byref(stats))
    calls = [lambda: L.osp_csr_select_k(None, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_select_k(None, ctypes.byref(zero_k), *refs),
             lambda: L.osp_csr_select_k(None, ctypes.byref(bad_order), *refs),
             lambda: L.osp_csr_select_k(None, ctypes.byref(bad_word), *refs),
             lambda: L.osp_csr_select_k(None, None, None, None),
             lambda: L.osp_csr_select_k(fake, None, *refs),
             lambda: L.osp_csr_select_k(fake, ctypes.byref(ok), None, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _fake(shape=(3, 3)):
    res = object.__new__(S.CsrResult)   # (no handle: the arguments are checked before anything is touched)
    res._h, res._ctx, res.shape, res.dtype, res.nnz = None, None, shape, np.float64, 0
    return res


def test_python_entries_exist_and_validate_before_touching_a_handle():
    assert callable(S.CsrResult.select_k)
    for name in ("sample_neighbors", "knn_graph", "random_walks"):
        assert callable(getattr(graph, name))
    a = _fake()
    for bad in (0, -1, 1 << 32, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            a.select_k(bad)
    for bad in ("median", None, 0, "LARGEST"):
        with pytest.raises(ValueError):
            a.select_k(1, bad)
    for bad in (-1, 1 << 64, 0.5, "1", None):
        with pytest.raises(ValueError):
            a.select_k(1, "random", seed=bad)
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.sample_neighbors(r, c, 3, [0], [0]), lambda: graph.sample_neighbors(r, c, 3, [0], [2], seed=-1),
                 lambda: graph.knn_graph(r, c, 3, np.ones(3), 0), lambda: graph.knn_graph(r, c, 3, np.ones(3), 1, symmetric="both"),
                 lambda: graph.knn_graph(r, c, 3, None, 1), lambda: graph.random_walks(r, c, 3, [0], -1),
                 lambda: graph.random_walks(r, c, 3, [0], 2, seed=1 << 64)):
        with pytest.raises(ValueError):
            call()


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        return   # (with a GPU they run: tests/test_gpu_sampling.py)
    r, c = np.array([0, 1, 2]), np.array([1, 2, 0])
    for call in (lambda: graph.sample_neighbors(r, c, 3, [0], [2]), lambda: graph.knn_graph(r, c, 3, np.ones(3), 1),
                 lambda: graph.random_walks(r, c, 3, [0], 2)):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model, value orders ---------------------------------------------------------------------------------------------------
def _random_csr(rng, m, n, density, dt=np.float64, values=None):
    lists = [np.flatnonzero(rng.random(n) < density) for _ in range(m)]
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.concatenate(lists + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = (rng.standard_normal(len(col)) if values is None else rng.choice(values, len(col))).astype(dt)
    return rowptr, col, val


def _pattern(csr, n):
    rowptr, col, _ = csr
    d = np.zeros((len(rowptr) - 1, n), bool)
    d[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), col] = True
    return d


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", ["largest", "smallest"])
def test_the_model_equals_a_dense_sort(order, dt):
    """On NaN-free input with ties: the kept set of a row is every entry strictly better than the k-th best value, and of
    the entries equal to it the leftmost ones; read off a dense ``np.sort`` of the row."""
    rng = np.random.default_rng(1)
    n = 40
    csr = _random_csr(rng, 30, n, 0.5, dt, values=[-2.0, -0.0, 0.0, 1.5, 3.0, np.inf, -np.inf, 1e-40])
    rowptr, col, val = csr
    for k in (1, 2, 5, 19, 40):
        (op, oc, ov), st = model.select_k(csr, n, k, order)
        want = np.zeros((30, n), bool)
        for i in range(30):
            c, v = col[rowptr[i]:rowptr[i + 1]].astype(np.int64), val[rowptr[i]:rowptr[i + 1]].astype(np.float64)
            if len(c) <= k:
                want[i, c] = True
                continue
            kth = np.sort(v)[::-1][k - 1] if order == "largest" else np.sort(v)[k - 1]
            better = v > kth if order == "largest" else v < kth
            want[i, c[better]] = True
            want[i, c[v == kth][:k - better.sum()]] = True
        assert np.array_equal(_pattern((op, oc, ov), n), want)
        assert np.array_equal(np.diff(op), np.minimum(np.diff(rowptr), k)) and st["nnz_out"] == len(oc)
        # values travel with their columns, bit for bit
        dense = np.zeros((30, n), dt)
        dense[np.repeat(np.arange(30), np.diff(rowptr)), col] = val
        got = dense[np.repeat(np.arange(30), np.diff(op)), oc]
        assert np.array_equal(got.view(np.uint32 if dt == np.float32 else np.uint64), ov.view(np.uint32 if dt == np.float32 else np.uint64))


def test_largest_of_x_is_smallest_of_minus_x_and_selects_nest():
    rng = np.random.default_rng(2)
    n = 50
    rowptr, col, val = _random_csr(rng, 25, n, 0.6, values=[-3.0, -1.0, 0.0, -0.0, 2.0, 2.5, np.nan])
    for k in (1, 3, 10, 33):
        a, _ = model.select_k((rowptr, col, val), n, k, "largest")
        b, _ = model.select_k((rowptr, col, -val), n, k, "smallest")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for order in model.ORDERS:
        for k, k2 in ((10, 3), (33, 10), (3, 3), (7, 1)):
            once, _ = model.select_k((rowptr, col, val), n, k2, order, seed=9)
            twice, _ = model.select_k(model.select_k((rowptr, col, val), n, k, order, seed=9)[0], n, k2, order, seed=9)
            for x, y in zip(once, twice):
                assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)


def test_nans_are_chosen_only_when_numbers_run_out():
    rng = np.random.default_rng(3)
    for order in ("largest", "smallest"):
        for numbers in (0, 1, 4, 9):
            v = np.full(12, np.nan)
            v[rng.choice(12, numbers, replace=False)] = rng.standard_normal(numbers) * np.array([np.inf, 1.0])[rng.integers(0, 2, numbers)]
            csr = (np.array([0, 12], np.int64), np.arange(12, dtype=np.uint32) * 3, v)
            for k in range(1, 12):
                (_, oc, ov), _ = model.select_k(csr, 40, k, order)
                assert np.isnan(ov).sum() == max(0, k - numbers)
                # the NaNs taken are the leftmost ones
                assert np.array_equal(oc[np.isnan(ov)], csr[1][np.isnan(v)][:max(0, k - numbers)])


# ---- the model, RANDOM ------------------------------------------------------------------------------------------------------------
def test_the_hash_is_the_header_s():
    """mix() on Python integers, and no two entries of a row share a key."""
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
        return z ^ (z >> 31)
    for seed, row, cols in ((0, 0, [0, 1, 2]), ((1 << 64) - 1, (1 << 32) - 2, [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 2]), (12345, 7, [5])):
        s = mix((seed + 0x9E3779B97F4A7C15) & ((1 << 64) - 1))
        want = [mix(s ^ ((row << 32) | j)) for j in cols]
        assert model.random_keys(seed, row, cols).tolist() == want
    for row in (0, 12345, (1 << 32) - 2):
        keys = model.random_keys(3, row, np.arange(1 << 16))
        assert len(np.unique(keys)) == 1 << 16


def _inclusion_statistic(row, cols, k, seeds):
    """X = sum (c - e)^2 / (e (1 - p)) (m - 1) / m over the columns' inclusion counts: chi-square with m - 1 degrees of freedom
    for uniform k-subsets.  ``seeds`` and ``row`` broadcast: one of them is an array of the trials."""
    cols = np.asarray(cols, np.uint64)
    m = len(cols)
    trials = max(np.size(seeds), np.size(row))
    counts = np.zeros(m)
    for t in range(trials):
        sd = seeds[t] if np.size(seeds) > 1 else seeds
        rw = row[t] if np.size(row) > 1 else row
        counts[np.argsort(model.random_keys(sd, rw, cols), kind="stable")[:k]] += 1
    p = k / m
    e = trials * p
    return float(((counts - e) ** 2).sum() / (e * (1 - p)) * (m - 1) / m)


SEEDS = np.arange(4000)


@pytest.mark.parametrize("row,cols,k,regression", [
    (0, np.arange(40), 10, 47.2),
    (12345, 64 * np.arange(40), 10, 43.8),
    (7, np.arange(40), 1, 40.9),
    (3, (1 << 31) + np.arange(257), 64, 259.1),
])
def test_inclusion_is_uniform_over_4000_seeds(row, cols, k, regression):
    x = _inclusion_statistic(row, cols, k, SEEDS)
    bound = scipy.stats.chi2.ppf(0.999, len(cols) - 1)
    print(f"X = {x:.1f}, bound {bound:.2f}")
    assert x < bound
    if len(cols) == 40:
        assert abs(bound - 72.06) < 0.01
    assert abs(x - regression) < 0.06   # the statistic is deterministic


def test_inclusion_is_uniform_across_rows():
    x = _inclusion_statistic(np.arange(4000), np.arange(40), 10, 1)
    print(f"X = {x:.1f}")
    assert x < scipy.stats.chi2.ppf(0.999, 39)
    assert abs(x - 35.4) < 0.06


def test_joint_inclusion_of_two_entries():
    m, k, n = 40, 10, len(SEEDS)
    expected = n * k * (k - 1) / (m * (m - 1))
    q = k * (k - 1) / (m * (m - 1))
    sd = (n * q * (1 - q)) ** 0.5
    assert abs(expected - 230.8) < 0.05 and abs(sd - 15) < 0.5
    cols = np.arange(m)
    for a, b in ((0, 1), (5, 30)):
        both = 0
        for s in SEEDS:
            top = np.argsort(model.random_keys(s, 0, cols), kind="stable")[:k]
            both += (a in top) and (b in top)
        print(f"entries {a} and {b} together: {both}")
        assert abs(both - expected) < 4 * sd


def test_random_ignores_values_and_other_rows():
    rng = np.random.default_rng(4)
    n = 60
    rowptr, col, val = _random_csr(rng, 20, n, 0.5)
    a, _ = model.select_k((rowptr, col, val), n, 6, "random", seed=5)
    b, _ = model.select_k((rowptr, col, np.full(len(col), np.nan)), n, 6, "random", seed=5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # row 7 alone, kept at its number
    lone = np.zeros(21, np.int64)
    lone[8:] = rowptr[8] - rowptr[7]
    c, _ = model.select_k((lone, col[rowptr[7]:rowptr[8]], val[rowptr[7]:rowptr[8]]), n, 6, "random", seed=5)
    assert np.array_equal(c[1], a[1][a[0][7]:a[0][8]])
    d, _ = model.select_k((rowptr, col, val), n, 6, "random", seed=6)
    assert not np.array_equal(a[1], d[1])


def test_the_model_counts_kernels_by_the_header_s_cost_paragraph():
    csr = (np.array([0, 3, 3, 5], np.int64), np.array([0, 1, 2, 1, 2], np.uint32), np.ones(5))
    assert model.select_k(csr, 3, 3, "largest")[1] == {"nnz_in": 5, "nnz_out": 5, "rows_capped": 0, "rows_long": 0, "launches": 0, "readbacks": 0}
    assert model.select_k(csr, 9, 3, "largest")[1]["launches"] == 1 and model.select_k(csr, 9, 3, "largest")[1]["readbacks"] == 1
    st = model.select_k(csr, 9, 2, "random")[1]
    assert st == {"nnz_in": 5, "nnz_out": 4, "rows_capped": 1, "rows_long": 0, "launches": 1 + 1 + 1 + 1 + 2, "readbacks": 2}
    big = (np.array([0, 5000, 5003], np.int64), np.concatenate([np.arange(5000), [1, 2, 3]]).astype(np.uint32), np.ones(5003))
    st = model.select_k(big, 6000, 2, "smallest")[1]
    assert (st["rows_capped"], st["rows_long"], st["launches"]) == (2, 1, 1 + 2 + 1 + 1 + 2)
    empty = (np.zeros(5, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    assert model.select_k(empty, 4, 1, "largest")[1]["launches"] == 0


# ---- the graph models ---------------------------------------------------------------------------------------------------------------
def _graph(seed, n=200, m=1500):
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n - 5, m), rng.integers(0, n - 5, m)   # (the last five vertices are isolated)
    return r, c, n


def test_sampled_blocks_are_sub_patterns_of_the_extracted_rows():
    r, c, n = _graph(1)
    A = model.adjacency(r, c, n)
    deg = np.diff(A[0])
    seeds = np.array([3, 17, 3, n - 1, 40])
    fanouts = (5, 3)
    blocks, frontiers, info = model.sample_neighbors(r, c, n, seeds, fanouts, seed=11)
    assert len(blocks) == 2 and len(frontiers) == 3 and np.array_equal(frontiers[0], seeds)
    for h, (bp, bc) in enumerate(blocks):
        f = frontiers[h]
        assert len(bp) == len(f) + 1
        assert np.array_equal(np.diff(bp), np.minimum(deg[f], fanouts[h]))
        for i, v in enumerate(f):
            mine = bc[bp[i]:bp[i + 1]]
            assert np.all(np.diff(mine.astype(np.int64)) > 0) and np.isin(mine, A[1][A[0][v]:A[0][v + 1]]).all()
        new = frontiers[h + 1][len(f):]
        assert np.array_equal(frontiers[h + 1][:len(f)], f) and np.all(np.diff(new) > 0)
        assert set(new) == set(bc.tolist()) - set(f.tolist())
        assert info["nnz"][h] == len(bc)
    # the repeated seed draws twice, independently (the key takes the frontier-local row)
    (bp, bc) = blocks[0]
    assert deg[3] > 10 and not np.array_equal(bc[bp[0]:bp[1]], bc[bp[2]:bp[3]])
    assert bp[4] == bp[3]   # the isolated seed


def test_knn_model_equals_argpartition_on_tie_free_weights():
    r, c, n = _graph(2)
    keep = r != c
    r, c = r[keep], c[keep]
    key = np.unique(np.minimum(r, c) * n + np.maximum(r, c))     # a simple graph: one weight per edge
    r, c = key // n, key % n
    w = np.random.default_rng(5).permutation(len(r)).astype(np.float64) + 0.5
    dense = np.full((n, n), np.nan)
    dense[r, c] = w
    dense[c, r] = w
    for largest in (True, False):
        for k in (1, 4, 9):
            listed = np.zeros((n, n), bool)
            for i in range(n):
                nb = np.flatnonzero(~np.isnan(dense[i]))
                if len(nb) > k:
                    score = -dense[i, nb] if largest else dense[i, nb]
                    nb = nb[np.argpartition(score, k - 1)[:k]]
                listed[i, nb] = True
            for symmetric, want in (("union", listed | listed.T), ("mutual", listed & listed.T), (None, listed)):
                (rowptr, col, val), st = model.knn_graph(r, c, n, w, k, largest, symmetric)
                assert np.array_equal(_pattern((rowptr, col, val), n), want), (largest, k, symmetric)
                rows = np.repeat(np.arange(n), np.diff(rowptr))
                assert np.array_equal(val, dense[rows, col])
                assert st["rows_capped"] == int((np.diff(model.adjacency(r, c, n)[0]) > k).sum())


def test_walks_only_step_along_edges():
    r, c, n = _graph(3)
    for directed in (False, True):
        rowptr, col, _ = model.adjacency(r, c, n, directed)
        edge = set(zip(np.repeat(np.arange(n), np.diff(rowptr)).tolist(), col.tolist()))
        dead_end = int(np.flatnonzero(np.diff(rowptr) == 0)[0])
        starts = np.array([0, 1, 1, dead_end, 50, 1])
        walks = model.random_walks(r, c, n, starts, 12, seed=21, directed=directed)
        assert walks.shape == (6, 13) and np.array_equal(walks[:, 0], starts)
        for wk in walks:
            for a, b in zip(wk[:-1], wk[1:]):
                assert (b == -1 and (a == -1 or rowptr[a + 1] == rowptr[a])) or (int(a), int(b)) in edge
        assert (walks[3, 1:] == -1).all()
        assert not np.array_equal(walks[1], walks[2])   # two walkers on one vertex move independently
        assert np.array_equal(walks, model.random_walks(r, c, n, starts, 12, seed=21, directed=directed))
