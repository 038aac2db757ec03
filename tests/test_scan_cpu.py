"""CPU-side checks of the row-wise scan and the weighted draws (include/outerspace_spgemm_scan.h) and of what is built on them:
the symbols are exported and listed, the four structs have the layout the C compiler gives them, null arguments are argument
errors that leave the outputs alone, the Python entries validate before they touch a handle and fail loudly without a GPU,
and the models that judge the GPU (tests/scan_model.py) equal constructions that share nothing with them: a pure-Python loop of
the header's definition, ``np.cumsum``, the monotonicity the order was chosen for, the hash on Python integers, chi-square
statistics of the draw counts, and the injected edge cases of the pick."""
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
from tests import scan_cases as sc
from tests import scan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "outerspace_spgemm_scan.h")
KERNELS = os.path.join(ROOT, "outerspace_amd", "csrc", "osp_scan.h")
DTS = [np.float32, np.float64]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_scan_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(osp_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert declared == set(_lib.SCAN_EXPORTS) == {"osp_csr_scan", "osp_csr_draw"}
    others = [name for name in dir(_lib) if name.endswith("EXPORTS") and name != "SCAN_EXPORTS"]
    assert len(others) >= 19
    for name in others:
        assert not declared & set(getattr(_lib, name)), name
    # the ops are reduce's first three, COUNT is not one of them
    assert _lib.SCAN_OPS == {k: v for k, v in _lib.REDUCE_OPS.items() if k != "count"} and tuple(_lib.SCAN_OPS) == model.OPS
    # the block, the chain's boundary and the local pass's tile: the header, the kernels, the binding and the model agree
    src = open(KERNELS).read()
    assert int(re.search(r"#define OSP_SCAN_BLOCK (\d+)", hdr).group(1)) == _lib.SCAN_BLOCK == model.BLOCK == 32
    assert int(re.search(r"kScanBlock\s*=\s*(\d+)", src).group(1)) == 32
    assert int(re.search(r"kScanChainLane\s*=\s*(\d+)", src).group(1)) == _lib.SCAN_CHAIN_LANE == model.CHAIN_LANE
    assert int(re.search(r"kScanLocalThreads\s*=\s*(\d+)", src).group(1)) == _lib.SCAN_LOCAL_TILE == model.LOCAL_TILE
    assert "OSP_SCAN" not in open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_settings.h")).read()   # no new setting
    assert "contract(off)" in src and "rocprim" not in src.lower()


def test_osp_version_is_still_7():
    assert re.search(r"#define OSP_VERSION 7\b", open(os.path.join(ROOT, "include", "outerspace_spgemm.h")).read())


@pytest.mark.parametrize("cname,struct", [("osp_scan_t", _lib.Scan), ("osp_scan_stats_t", _lib.ScanStats), ("osp_draw_t", _lib.Draw),
                                          ("osp_draw_stats_t", _lib.DrawStats)])
def test_scan_structs_have_the_layout_the_c_compiler_gives(tmp_path, cname, struct):
    fields = [name for name, _ in struct._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm_scan.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'    printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    if struct is _lib.ScanStats:
        assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "blocks", "ms_total", "launches", "readbacks"}
    if struct is _lib.DrawStats:
        assert set(struct().as_dict()) == {"nnz_in", "nnz_out", "rows_without", "ms_total", "launches", "readbacks"}


def test_scan_null_arguments_are_argument_errors():
    """Without a device there is no result to pass: every call with a null `in` (whatever else is wrong with it), and a fake
    operand with a null sc or out (the null checks come before an operand is touched; tests/test_gpu_scan.py passes the other
    bad arguments with real results)."""
    L = _lib.lib()
    sentinel = 0x1234
    out = ctypes.c_void_p(sentinel)
    stats = _lib.ScanStats()
    stats.nnz_in = 77
    ok = _lib.Scan()
    count = _lib.Scan()
    count.op = 3
    bad_word = _lib.Scan()
    bad_word.reserved[7] = 1
    fake = ctypes.c_void_p(0x1000)
    refs = (ctypes.byref(out), ctypes.byref(stats))
    calls = [lambda: L.osp_csr_scan(None, ctypes.byref(ok), *refs),
             lambda: L.osp_csr_scan(None, ctypes.byref(count), *refs),
             lambda: L.osp_csr_scan(None, ctypes.byref(bad_word), *refs),
             lambda: L.osp_csr_scan(None, None, None, None),
             lambda: L.osp_csr_scan(fake, None, *refs),
             lambda: L.osp_csr_scan(fake, ctypes.byref(ok), None, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert out.value == sentinel and stats.nnz_in == 77


def test_draw_null_arguments_are_argument_errors():
    L = _lib.lib()
    cols = np.full(4, 55, np.int64)
    pos = np.full(4, 66, np.int64)
    stats = _lib.DrawStats()
    stats.nnz_in = 77
    ok = _lib.Draw()
    ok.draws = 2
    zero = _lib.Draw()
    fake = ctypes.c_void_p(0x1000)
    cp, pp = ctypes.c_void_p(cols.ctypes.data), ctypes.c_void_p(pos.ctypes.data)
    calls = [lambda: L.osp_csr_draw(None, ctypes.byref(ok), cp, pp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_draw(None, ctypes.byref(zero), cp, pp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_draw(None, None, None, None, _lib.OSP_HOST, None),
             lambda: L.osp_csr_draw(fake, None, cp, pp, _lib.OSP_HOST, ctypes.byref(stats)),
             lambda: L.osp_csr_draw(fake, ctypes.byref(ok), None, pp, _lib.OSP_HOST, ctypes.byref(stats))]
    for call in calls:
        assert call() == _lib.ERR_ARG
        assert L.osp_last_error_string()
        assert (cols == 55).all() and (pos == 66).all() and stats.nnz_in == 77


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _fake(shape=(3, 3)):
    res = object.__new__(S.CsrResult)   # (no handle: the arguments are checked before anything is touched)
    res._h, res._ctx, res.shape, res.dtype, res.nnz = None, None, shape, np.float64, 0
    return res


def test_python_entries_exist_and_validate_before_touching_a_handle():
    assert callable(S.CsrResult.scan) and callable(S.CsrResult.draw)
    for name in ("weighted_random_walks", "weighted_sample_neighbors", "random_walks", "sample_neighbors"):
        assert callable(getattr(graph, name))
    a = _fake()
    for bad in ("count", "sum", None, 0, "PLUS"):
        with pytest.raises(ValueError):
            a.scan(bad)
    for bad in (0, -1, 1 << 32, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            a.draw(bad)
    for bad in (-1, 1 << 64, 0.5, "1", None):
        with pytest.raises(ValueError):
            a.draw(1, seed=bad)
    with pytest.raises(ValueError):
        a.draw(1, space="gpu")
    with pytest.raises(S.OspError) as ei:
        _fake(((1 << 20), 3)).draw((1 << 20) + 1, space="host")
    assert ei.value.status == _lib.ERR_ARG
    with pytest.raises(S.OspError):
        a.draw(2, out=np.zeros((3, 3), np.int64), space="host")       # the wrong shape
    with pytest.raises(S.OspError):
        a.draw(2, out=np.zeros((3, 2), np.float64), space="host")     # the wrong dtype
    with pytest.raises(S.OspError):
        a.draw(2, out_pos=np.zeros(6, np.int64), space="host")
    r, c, w = np.array([0, 1, 2]), np.array([1, 2, 0]), np.ones(3)
    for call in (lambda: graph.weighted_random_walks(r, c, 3, w, [0], -1), lambda: graph.weighted_random_walks(r, c, 3, w, [0], 2, seed=1 << 64),
                 lambda: graph.weighted_random_walks(r, c, 3, None, [0], 2), lambda: graph.weighted_sample_neighbors(r, c, 3, w, [0], [0]),
                 lambda: graph.weighted_sample_neighbors(r, c, 3, w, [0], [2], seed=-1),
                 lambda: graph.weighted_sample_neighbors(r, c, 3, None, [0], [2])):
        with pytest.raises(ValueError):
            call()


def test_graph_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        return   # (with a GPU they run: tests/test_gpu_weighted_walks.py)
    r, c, w = np.array([0, 1, 2]), np.array([1, 2, 0]), np.ones(3)
    for call in (lambda: graph.weighted_random_walks(r, c, 3, w, [0], 2), lambda: graph.weighted_sample_neighbors(r, c, 3, w, [0], [2])):
        with pytest.raises(S.OspError) as ei:
            call()
        assert ei.value.status == _lib.ERR_HIP and "no CPU path" in str(ei.value)


# ---- the model of the scan -----------------------------------------------------------------------------------------------------------
def _definition(v, op):
    """The header's definition as a loop over Python scalars of the dtype."""
    dt = v.dtype.type
    ident = model.identity(op, dt)

    def comb(a, b):
        if op == "plus":
            with np.errstate(all="ignore"):
                return dt(a + b)
        if op == "min":
            return b if b < a else a
        return b if b > a else a
    L, T = [], []
    for q, e in enumerate(v):
        L.append(comb(ident if q % 32 == 0 else L[-1], e))
        if q % 32 == 31 or q == len(v) - 1:
            T.append(L[-1])
    C = [ident]
    for t in T:
        C.append(comb(C[-1], t))
    return np.array([comb(C[q // 32], L[q]) for q in range(len(v))], v.dtype)


def _adversarial(rng, m, dt):
    """Non-negative entries with magnitudes from 2^-60 to 2^60, a fifth of them zero."""
    v = np.ldexp(rng.random(m) + 0.5, rng.integers(-60, 61, m)).astype(dt)
    v[rng.random(m) < 0.2] = 0
    return v


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", model.OPS)
def test_the_model_equals_a_loop_of_the_definition(op, dt):
    rng = np.random.default_rng(1)
    sp = sc.kc.special(dt)
    for m in (1, 2, 31, 32, 33, 63, 64, 65, 100, 257, 400):
        v = rng.standard_normal(m).astype(dt)
        v[::7] = np.resize(sp, len(v[::7]))
        assert model.same(model.scan_row(v, op), _definition(v, op)), m
        if op != "plus":   # (no NaN comes out: the bits themselves)
            assert np.array_equal(_bits(model.scan_row(v, op)), _bits(_definition(v, op))), m
        w = _adversarial(rng, m, dt)
        assert np.array_equal(_bits(model.scan_row(w, op)), _bits(_definition(w, op))), m
    assert len(model.scan_row(np.zeros(0, dt), op)) == 0


@pytest.mark.parametrize("dt", DTS)
def test_rows_of_at_most_32_entries_are_cumsum(dt):
    rng = np.random.default_rng(2)
    for m in range(1, 33):
        v = rng.standard_normal(m).astype(dt)
        assert np.array_equal(_bits(model.scan_row(v, "plus")), _bits(np.cumsum(v, dtype=dt)))
    # except that a leading -0.0 reads +0.0, as in reduce
    v = np.array([-0.0, -0.0, 1.0], dt)
    assert np.array_equal(_bits(model.scan_row(v, "plus")), _bits(np.array([0.0, 0.0, 1.0], dt)))
    assert np.signbit(np.cumsum(v, dtype=dt)[0])
    # in block 0 S has L's bits; beyond it S = C (+) L
    v = rng.standard_normal(70).astype(dt)
    S_ = model.scan_row(v, "plus")
    assert np.array_equal(_bits(S_[:32]), _bits(np.cumsum(v[:32], dtype=dt)))
    assert S_[40] == dt(S_[31] + np.cumsum(v[32:41], dtype=dt)[-1])


@pytest.mark.parametrize("dt", DTS)
def test_plus_is_monotone_on_non_negative_input_and_a_zero_repeats_the_value_before_it(dt):
    rng = np.random.default_rng(3)
    rows = 0
    for trial in range(300):
        m = int(rng.integers(1, 5000)) if trial % 10 == 0 else int(rng.integers(1, 400))
        v = _adversarial(rng, m, dt)
        S_ = model.scan_row(v, "plus")
        assert np.all(S_[1:] >= S_[:-1]), (trial, m)
        zero = np.flatnonzero(v[1:] == 0) + 1
        assert np.array_equal(_bits(S_[zero]), _bits(S_[zero - 1])), (trial, m)
        rows += 1
    assert rows == 300
    # a scan by doubling is not monotone: the property is the order's, not addition's
    v = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 0.0], np.float32)
    pair = np.float32(v[1] + v[2])
    assert np.float32(v[0] + pair) > np.float32(np.float32(v[0] + v[1]) + v[2])


@pytest.mark.parametrize("dt", DTS)
def test_min_and_max_never_return_a_nan_and_plus_propagates_one(dt):
    rng = np.random.default_rng(4)
    for m in (5, 32, 33, 100):
        v = rng.standard_normal(m).astype(dt)
        v[rng.random(m) < 0.4] = np.nan
        v[0] = np.nan                       # a leading NaN: the identity until a number arrives
        first = int(np.flatnonzero(~np.isnan(v))[0])
        for op, ident, ref in (("min", np.inf, np.fmin), ("max", -np.inf, np.fmax)):
            S_ = model.scan_row(v, op)
            assert not np.isnan(S_).any()
            assert (S_[:first] == ident).all()
            assert np.array_equal(S_[first:], ref.accumulate(v)[first:])
        at = m // 2
        w = np.abs(rng.standard_normal(m)).astype(dt)
        w[at] = np.nan
        S_ = model.scan_row(w, "plus")
        assert not np.isnan(S_[:at]).any() and np.isnan(S_[at:]).all()
    allnan = np.full(40, np.nan, dt)
    assert (model.scan_row(allnan, "min") == np.inf).all() and (model.scan_row(allnan, "max") == -np.inf).all()
    assert np.isnan(model.scan_row(np.array([np.inf, -np.inf, 1.0], dt), "plus")[1:]).all()


def test_a_row_s_scan_depends_on_the_row_alone_and_the_stats_follow_the_header():
    csr, ncol = sc.family(np.float64)["edges"]
    full = model.scan(csr, "plus")
    for i in (3, 9, len(csr[0]) - 2):
        b, e = csr[0][i], csr[0][i + 1]
        assert model.same(full[2][b:e], model.scan_row(csr[2][b:e], "plus"))
    assert model.scan_stats(csr, ncol) == {"nnz_in": len(csr[1]), "nnz_out": len(csr[1]), "blocks": len(csr[1]) // 32 + len(csr[0]) - 1,
                                           "launches": 1 + 1 + 2, "readbacks": 0}
    small = (np.array([0, 3, 3, 5], np.int64), np.array([0, 1, 2, 1, 2], np.uint32), np.ones(5))
    assert model.scan_stats(small, 40)["launches"] == 2 and model.scan_stats(small, 40)["blocks"] == 3
    empty = (np.zeros(5, np.int64), np.zeros(0, np.uint32), np.zeros(0))
    assert model.scan_stats(empty, 4)["launches"] == 0 and model.draw_stats(empty, 4, 3) == {"nnz_in": 0, "nnz_out": 12, "launches": 0, "readbacks": 0}
    assert model.draw_stats(small, 40, 2) == {"nnz_in": 5, "nnz_out": 6, "launches": 5, "readbacks": 1}


# ---- the model of the draw -----------------------------------------------------------------------------------------------------------
def test_the_hash_is_the_header_s():
    """mix() on Python integers with the header's constants, and both uniforms are exact fractions below 1."""
    hdr = open(HEADER).read()
    assert "0x9E3779B97F4A7C15" in hdr and model.GOLDEN == 0x9E3779B97F4A7C15
    sk = open(os.path.join(ROOT, "include", "outerspace_spgemm_select_k.h")).read()
    assert "0xBF58476D1CE4E5B9" in sk and "0x94D049BB133111EB" in sk

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
        return z ^ (z >> 31)
    for seed, row, draws in ((0, 0, 3), ((1 << 64) - 1, (1 << 32) - 2, 4), (12345, 7, 1)):
        s0 = mix((seed + 0x9E3779B97F4A7C15) & ((1 << 64) - 1))
        want = [mix(s0 ^ ((row << 32) | d)) for d in range(draws)]
        got = model.mix_array(np.uint64(model.mix(seed + model.GOLDEN)) ^ ((np.uint64(row) << np.uint64(32)) | np.arange(draws, dtype=np.uint64)))
        assert got.tolist() == want
        u64, u32 = model.uniform(got, np.float64), model.uniform(got, np.float32)
        assert u64.dtype == np.float64 and u32.dtype == np.float32
        assert [float(x) for x in u64] == [(h >> 11) / 2 ** 53 for h in want]
        assert [float(x) for x in u32] == [(h >> 40) / 2 ** 24 for h in want]
    top = np.array([(1 << 64) - 1], np.uint64)
    assert model.uniform(top, np.float64)[0] < 1 and model.uniform(top, np.float32)[0] < 1


@pytest.mark.parametrize("dt", DTS)
def test_the_pick_with_t_at_both_ends_injected(dt):
    """t == total and t == 0 cannot be produced through the hash: the fallback clause is reachable only here."""
    v = np.array([0, 0, 3, 0, 5, 0, 0], dt)
    S_ = model.scan_row(model.weights(v), "plus")
    assert S_.tolist() == [0, 0, 3, 3, 8, 8, 8]
    assert model.pick(S_, dt(0)) == 2           # the first entry of positive weight, not the leading zeros
    assert model.pick(S_, dt(2.999)) == 2 and model.pick(S_, dt(3)) == 4 and model.pick(S_, dt(7.5)) == 4
    assert model.pick(S_, dt(8)) == 4           # t == total: S_q == total picks the entry that reached it, not a trailing zero
    assert model.pick(S_, np.nextafter(dt(8), dt(0))) == 4
    one = model.scan_row(np.array([2.5], dt), "plus")
    assert model.pick(one, dt(0)) == 0 and model.pick(one, dt(2.5)) == 0
    # the vectorised form in model.draw is the same predicate
    rng = np.random.default_rng(5)
    w = rng.random(200).astype(dt)
    w[rng.random(200) < 0.3] = 0
    S_ = model.scan_row(w, "plus")
    for t in list(S_[::9]) + [dt(0), S_[-1]] + list((rng.random(50) * S_[-1]).astype(dt)):
        q = min(np.searchsorted(S_, t, side="right"), np.searchsorted(S_, S_[-1], side="left"))
        assert q == model.pick(S_, t) and w[q] > 0


def _one_row(vals, cols=None):
    vals = np.asarray(vals)
    cols = np.arange(len(vals)) if cols is None else np.asarray(cols)
    return np.array([0, len(vals)], np.int64), cols.astype(np.uint32), vals


@pytest.mark.parametrize("dt", DTS)
def test_every_draw_lands_on_a_positive_finite_weight_and_rows_without_one_give_minus_one(dt):
    big = np.finfo(dt).max
    rows = [[1.0, 0.0, np.nan, -2.0, np.inf, 3.0, -np.inf, 0.5, -0.0],
            [0.0, 0.0, -0.0],
            [np.nan, np.nan],
            [-1.0, -5.0],
            [0.75 * big, 0.75 * big],     # the sum overflows
            [],
            [np.inf, -np.inf, np.nan],
            [0.0] * 40 + [7.0] + [0.0] * 40]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    val = np.array([x for r in rows for x in r], dt)
    col = np.concatenate([np.arange(len(r)) * 2 + 1 for r in rows]).astype(np.uint32)
    for seed in range(5):
        cols, pos, without = model.draw((rowptr, col, val), 200, seed)
        assert without == 6
        assert (cols[1:7] == -1).all() and (pos[1:7] == -1).all()
        assert set(val[pos[0]].tolist()) == {1.0, 3.0, 0.5} and np.array_equal(cols[0], col[pos[0]])
        assert (pos[7] == rowptr[7] + 40).all() and (cols[7] == 81).all()
        assert (pos[0] >= 0).all() and (pos[0] < rowptr[1]).all()


def _counts(w, draws, seed, dt, row=0):
    """Draw counts per entry of one row placed at number ``row``."""
    rowptr = np.zeros(row + 2, np.int64)
    rowptr[row + 1] = len(w)
    _, pos, _ = model.draw((rowptr, np.arange(len(w), dtype=np.uint32), np.asarray(w, dt)), draws, seed)
    return np.bincount(pos[row], minlength=len(w))


CHI = {  # (m, draws, dtype name) -> the five statistics of seeds 0..4, pinned as regressions
    (8, 4000, "float32"): [7.0, 6.1, 5.5, 10.2, 6.3],
    (8, 4000, "float64"): [7.0, 6.1, 5.5, 10.2, 6.3],
    (100, 40000, "float32"): [87.7, 101.7, 86.3, 110.4, 117.6],
    (100, 40000, "float64"): [87.7, 101.7, 86.8, 110.4, 117.6],
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("m,draws", [(8, 4000), (100, 40000)])
def test_draw_counts_follow_the_weights(m, draws, dt):
    w = np.arange(1, m + 1, dtype=np.float64)
    expected = draws * w / w.sum()
    assert expected.min() >= 5
    bound = scipy.stats.chi2.ppf(0.999, m - 1)
    assert abs(bound - (24.32 if m == 8 else 148.23)) < 0.01
    got = []
    for seed in range(5):
        c = _counts(w, draws, seed, dt)
        assert c.sum() == draws
        x = float(((c - expected) ** 2 / expected).sum())
        print(f"m={m} draws={draws} {np.dtype(dt).name} seed={seed}: X = {x:.1f}, bound {bound:.2f}")
        assert x < bound
        got.append(round(x, 1))
    assert np.allclose(got, CHI[(m, draws, np.dtype(dt).name)], atol=0.06), got   # the statistic is deterministic


def test_draws_of_two_rows_and_of_two_draw_numbers_are_uncorrelated():
    """2 x 2 tables of 'the draw fell in the heavier half': rows 0 and 1 at the same draw number over 4000 draw numbers, and
    draw numbers d and d + 1 of one row over 2000 pairs; chi-square with one degree of freedom at the same quantile."""
    w = np.array([1.0, 2.0, 3.0, 6.0])          # the last entry holds half of the weight
    bound = scipy.stats.chi2.ppf(0.999, 1)
    rowptr = np.array([0, 4, 8], np.int64)
    csr = (rowptr, np.tile(np.arange(4, dtype=np.uint32), 2), np.tile(w, 2))

    def statistic(a, b):
        table = np.array([[np.sum(a & b), np.sum(a & ~b)], [np.sum(~a & b), np.sum(~a & ~b)]], float)
        e = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
        return float(((table - e) ** 2 / e).sum())
    for seed in (0, 1):
        cols, _, _ = model.draw(csr, 4000, seed)
        heavy = cols == 3
        x_rows = statistic(heavy[0], heavy[1])
        x_draws = statistic(heavy[0][0::2], heavy[0][1::2])
        print(f"seed {seed}: rows X = {x_rows:.2f}, draw numbers X = {x_draws:.2f}, bound {bound:.2f}")
        assert x_rows < bound and x_draws < bound
        assert abs(heavy[0].mean() - 0.5) < 0.04 and not np.array_equal(cols[0], cols[1])


def test_a_row_s_draws_depend_on_its_number_and_values_alone():
    rng = np.random.default_rng(6)
    csr, ncol = sc.family(np.float64)["ragged positive"]
    a = model.draw(csr, 7, 5)
    changed = csr[2].copy()
    changed[csr[0][9]:csr[0][10]] = rng.random(csr[0][10] - csr[0][9])
    b = model.draw((csr[0], csr[1], changed), 7, 5)
    keep = np.arange(len(csr[0]) - 1) != 9
    assert np.array_equal(a[0][keep], b[0][keep]) and np.array_equal(a[1][keep], b[1][keep]) and not np.array_equal(a[1][9], b[1][9])
    assert not np.array_equal(a[0], model.draw(csr, 7, 6)[0])
    # the same values at another row number draw differently; the first draws of s = 7 are the draws of s = 2
    assert np.array_equal(a[0][:, :2], model.draw(csr, 2, 5)[0])
    assert not np.array_equal(_counts(np.arange(1, 9), 50, 3, np.float64, row=0), _counts(np.arange(1, 9), 50, 3, np.float64, row=1))


# ---- the graph models ---------------------------------------------------------------------------------------------------------------
def _graph(seed, n=200, m=1500):
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n - 5, m), rng.integers(0, n - 5, m)   # (the last five vertices are isolated)
    w = rng.integers(0, 4, m).astype(np.float64)                  # a quarter of the edges weigh 0; parallel edges add exactly
    return r, c, n, w


def test_walks_only_step_along_edges_of_positive_weight():
    r, c, n, w = _graph(3)
    for directed in (False, True):
        rowptr, col, val = model.adjacency(r, c, n, w, directed, np.float64)
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        edge = set(zip(rows[val > 0].tolist(), col[val > 0].tolist()))
        assert (val == 0).any()
        stuck = np.array([not (val[rowptr[v]:rowptr[v + 1]] > 0).any() for v in range(n)])
        dead_end = int(np.flatnonzero(stuck)[0])
        starts = np.array([0, 1, 1, dead_end, 50, 1])
        walks = model.weighted_random_walks(r, c, n, w, starts, 12, seed=21, directed=directed)
        assert walks.shape == (6, 13) and np.array_equal(walks[:, 0], starts)
        for wk in walks:
            for a, b in zip(wk[:-1], wk[1:]):
                assert (b == -1 and (a == -1 or stuck[a])) or (int(a), int(b)) in edge
        assert (walks[3, 1:] == -1).all()
        assert not np.array_equal(walks[1], walks[2])   # two walkers on one vertex move independently
        assert np.array_equal(walks, model.weighted_random_walks(r, c, n, w, starts, 12, seed=21, directed=directed))


def test_sampled_multiplicities_sum_to_the_fanout():
    r, c, n, w = _graph(1)
    A = model.adjacency(r, c, n, w, False, np.float64)
    drawable = np.array([(A[2][A[0][v]:A[0][v + 1]] > 0).any() for v in range(n)])
    seeds = np.array([3, 17, 3, n - 1, 40])
    fanouts = (5, 3)
    blocks, frontiers = model.weighted_sample_neighbors(r, c, n, w, seeds, fanouts, seed=11)
    assert len(blocks) == 2 and len(frontiers) == 3 and np.array_equal(frontiers[0], seeds)
    for h, (bp, bc, bv) in enumerate(blocks):
        f = frontiers[h]
        sums = np.add.reduceat(np.concatenate([bv, [0]]), bp[:-1])[:len(f)] * (np.diff(bp) > 0)
        assert np.array_equal(sums, np.where(drawable[f], fanouts[h], 0))
        for i, v in enumerate(f):
            mine = bc[bp[i]:bp[i + 1]]
            lo, hi = A[0][v], A[0][v + 1]
            assert np.all(np.diff(mine.astype(np.int64)) > 0) and np.isin(mine, A[1][lo:hi][A[2][lo:hi] > 0]).all()
        new = frontiers[h + 1][len(f):]
        assert np.array_equal(frontiers[h + 1][:len(f)], f) and np.all(np.diff(new) > 0)
        assert set(new) == set(bc.tolist()) - set(f.tolist())
    assert not drawable[n - 1] and blocks[0][0][4] == blocks[0][0][3]   # the isolated seed
