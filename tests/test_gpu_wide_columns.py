"""Every operation of the library on column spaces of 2^24 to 2^32 - 1 columns (tests/wide_columns.py: WIDTHS and the three
relabelings), bit for bit: row pointers and columns equal, values equal as bits, a NaN that came out of arithmetic only has to
be a NaN.  No tolerance anywhere.

The reference is never the code under test.  It is the oracle or a numpy model run on the wide operands, or -- every operation
but the positional predicates of ``select`` sees a column only through comparisons with other columns -- the oracle's or the
model's NARROW answer with the relabeling applied to its columns (tests/test_wide_columns_cpu.py holds the models to that
equivalence at every width).  The products at the largest width are checked against the oracle on the wide operands too.

The product: B's columns are relabeled, A stays.  The cases are narrow ones the suite already has (the skewed random operands
of test_gpu_fuzz.py, the long row / pile / dense-segment product of test_gpu_parity.py, a stretch row of
test_gpu_split_from_b.py, the small-planner and four-wave-planner rows of test_gpu_plan_small.py, gathered and written), each
whole, through ``partial_capacity`` panels, as row shards and with a k range, plus ``spgemm_coo``, ``spgemm_masked`` and a
hand-built tile of the most rows a width allows whose first row holds column 0 and whose last row holds column N - 1.
``test_the_wide_products_reached_the_hard_paths`` (the last test of the module) asserts from ``res.info`` that long rows,
sorted segments, direct rows, gathered rows and several panels each occurred at every width and under every map, and states
the one path the planner cannot take at these widths: dense segments.  ``spgemm_masked`` has an O(N) footprint (a column view
of B) and runs with the operations of that kind; from N = 2^32 - 256 on it refuses, and so does ``transpose``.

The result operations run on results of wide N uploaded with ``merge_csr_parts`` (a merge at that width): the built pair of
test_gpu_mxm.py with the right operand's columns relabeled, and operands A and P of result_chain.starting_operands.
A row permutation runs at every width as ``extract(rows=a permutation)``; ``permute`` itself needs a square result and is an
extract by columns as well, so it runs with the O(N) operations.

The operations whose footprint is O(N) -- transpose, reduce over columns, extract / select_vertices by columns, apply_vectors
with a column vector, mxv, mxd and sddmm with real operands, permute -- run once each at N = 2^25 + 1 with columns 0, 2^24, 2^24 + 1
and N - 1 occupied, and at no other width.  The largest single allocation of this file is there: the 2^25 + 2 int64 row pointers
of a result of that many rows (256 MiB, on the device and on the host).  No allocation is larger; the test that holds most at
once is permute's, with five such results (1.3 GiB)."""
import collections
import functools

import numpy as np
import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import spgemm as S
from tests import bfs_model, build_model, ewise_model, extract_model, mcl_model, mxd_model, mxm_masked_model, mxv_arg_model
from tests import mxv_model, result_chain, sddmm_model, semiring_model, transpose_model, truss_model, vector_model
from tests import test_gpu_apply_mask as am        # _upload, _dev, _bits, _mask_for only
from tests import test_gpu_fuzz as fuzz            # skewed_coo only
from tests import test_gpu_masked as gmasked       # _filtered only
from tests import test_gpu_mxm as gm               # the built pair, SEMIRINGS, _check_stats only
from tests import test_gpu_plan_small as plan_small   # Operands only
from tests import test_gpu_split_from_b as sfb     # Operands, FORCE only
from tests import wide_columns as W
from tests.ieee_model import assert_same_bits

pytestmark = pytest.mark.gpu

DEV = am.DEV
_bits, _upload, _dev = am._bits, am._upload, am._dev
DTYPES = [np.float32, np.float64]
PATHS = ("heavy_rows", "sorted_segments", "dense_segments", "direct_rows", "gathered_rows", "panels")
SEEN = collections.defaultdict(collections.Counter)      # (N, map) -> how many wide products took each path
TOTALS = collections.Counter()                            # res.info summed over the module's wide products


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    _ctx_shared.algorithm = "outer"
    yield _ctx_shared
    _ctx_shared.trim()
    torch.cuda.empty_cache()


def _tally(N, name, info):
    for p in PATHS:
        SEEN[N, name][p] += info[p] > (1 if p == "panels" else 0)
        TOTALS[p] += info[p]
    TOTALS["products"] += 1
    TOTALS["partials"] += info["partials"]


def _same(res, want, computed=False, what=""):
    """A CsrResult against (rowptr, col, val): exact, values as bits; where ``computed`` (True, or a mask over the entries) says
    the value came out of arithmetic, a NaN only has to be a NaN."""
    rowptr, col, val = want[:3]
    assert res.nnz == len(col) == res.info["nnz_c"], what
    assert np.array_equal(res.rowptr, rowptr), what
    assert res.colidx.dtype == np.uint32 and np.array_equal(res.colidx, col), what
    _same_values(res.vals, val, computed, what)


def _same_values(got, val, computed=False, what=""):
    got, val = np.asarray(got), np.asarray(val)
    assert got.dtype == val.dtype and got.shape == val.shape, what
    loose = np.isnan(val) & np.broadcast_to(np.asarray(computed, bool), val.shape)
    assert np.isnan(got[loose]).all(), what
    assert np.array_equal(_bits(got[~loose]), _bits(val[~loose])), what


def _rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


# ==== the product =========================================================================================================================
def _csc_csr(M, K, a, b, dt):
    return S.coo_to_csc(K, a[0], a[1], a[2].astype(dt)), S.coo_to_csr(K, b[0], b[1], b[2].astype(dt))


def _skewed(seed, alpha, M, K, n, nnz_a, nnz_b, dt):
    rng = np.random.default_rng(seed)
    return M, K, n, fuzz.skewed_coo(rng, M, K, nnz_a, alpha, dt), fuzz.skewed_coo(rng, K, n, nnz_b, alpha, dt)


def _long_rows():
    """test_gpu_parity.test_long_rows_split_and_fallback's operands: column 5 of output row 0 collects 6000 products."""
    rng = np.random.default_rng(3)
    M, K, n = 8, 6000, 64
    a_rows = np.concatenate([np.zeros(K, np.uint32), rng.integers(1, M, 400).astype(np.uint32)])
    a_cols = np.concatenate([np.arange(K, dtype=np.uint32), rng.choice(K, 400, replace=False).astype(np.uint32)])
    key = np.unique(a_rows.astype(np.int64) * K + a_cols)
    a = ((key // K).astype(np.uint32), (key % K).astype(np.uint32), rng.uniform(0.5, 1.5, len(key)))
    b_cols = np.stack([np.full(K, 5), rng.integers(6, 35, K), rng.integers(35, n, K)], 1).reshape(-1).astype(np.uint32)
    return M, K, n, a, (np.repeat(np.arange(K, dtype=np.uint32), 3), b_cols, rng.uniform(0.5, 1.5, 3 * K))


def _stretch():
    """test_gpu_split_from_b.test_one_job: a stretch row of 7000 products beside two short rows (n = 2^20)."""
    ops = sfb.Operands(1)
    ops.a_row([40, 3])
    ops.a_row([100] * 70)
    ops.a_row([9])
    M, K, a, b = ops.coo()
    return M, K, sfb.N, a, b


def _planned():
    """test_gpu_plan_small.test_long_and_short_chunks: two rows of the one-wave planner and one of the four-wave planner
    (n = 2^18)."""
    ops = plan_small.Operands(4)
    ops.a_row([177] * 28)
    ops.a_row([7] * 300)
    ops.a_row([9] * 60 + [plan_small.TILE_CAP[np.dtype(np.float64)]])
    M, K, a, b = ops.coo()
    return M, K, plan_small.N, a, b


NO_HUB = dict(sfb.FORCE, OSP_HUB="0")
# name -> (builder, dtype, environment)
PRODUCTS = {
    "skew_uniform": (lambda: _skewed(11, 0.0, 1200, 1500, 2500, 20000, 20000, np.float64), np.float64, {}),
    "skew_1": (lambda: _skewed(12, 1.0, 700, 1100, 2300, 30000, 30000, np.float32), np.float32, {}),
    "skew_3": (lambda: _skewed(13, 3.0, 300, 500, 1900, 8000, 8000, np.float64), np.float64, {}),
    "skew_3_sorted": (lambda: _skewed(13, 3.0, 300, 500, 1900, 8000, 8000, np.float32), np.float32, {"OSP_DENSE_SEG": "0", "OSP_BIGTILE_CAP": "0"}),
    "long_rows_dense": (_long_rows, np.float64, {"OSP_DENSE_SEG": "1"}),
    "long_rows_pile": (_long_rows, np.float32, {"OSP_DENSE_SEG": "0", "OSP_BIGTILE_CAP": "0"}),
    "stretch": (_stretch, np.float64, NO_HUB),
    "planned_gathered": (_planned, np.float64, {}),
    "planned_written": (_planned, np.float64, {"OSP_GATHER": "0"}),
}
_ORACLE = {}


@functools.lru_cache(maxsize=None)
def _product_case(case):
    build, dt, env = PRODUCTS[case]
    M, K, n, a, b = build()
    acsc, bcsr = _csc_csr(M, K, a, b, dt)
    rowlen = int(np.bincount(a[0], weights=np.diff(bcsr[0])[a[1]], minlength=M).max())
    return M, K, n, acsc, bcsr, rowlen


def _oracle(port, case, k_range=None):
    """The oracle's NARROW answer, once per case and k range."""
    if (case, k_range) not in _ORACLE:
        M, K, n, acsc, bcsr, _ = _product_case(case)
        _ORACLE[case, k_range] = port.spgemm(M, K, n, *acsc, *bcsr, *(k_range or ()))
    return _ORACLE[case, k_range]


def _same_product(got, want, table, lo=0, hi=None):
    hi = len(want["rowptr"]) - 1 if hi is None else hi
    o0, o1 = want["rowptr"][lo], want["rowptr"][hi]
    assert np.array_equal(got.rowptr, want["rowptr"][lo:hi + 1] - o0)
    assert got.colidx.dtype == np.uint32 and np.array_equal(got.colidx, W.relabel(want["colidx"][o0:o1], table))
    assert_same_bits(got.vals, want["vals"][o0:o1])


@pytest.mark.parametrize("case", sorted(PRODUCTS))
@pytest.mark.parametrize("name", W.MAPS)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_products_equal_the_oracle(mctx, port, monkeypatch, N, name, case):
    M, K, n, acsc, bcsr, rowlen = _product_case(case)
    for k, v in PRODUCTS[case][2].items():
        monkeypatch.setenv(k, v)
    table = W.phi(name, n, N)
    bw = W.relabel_csr(bcsr, table)
    want = _oracle(port, case)
    P = want["partials"]
    res = mctx.spgemm_csc_csr(M, K, N, *acsc, *bw)
    assert res.info["partials"] == P and res.shape == (M, N) and res.info["N"] == N
    _same_product(res, want, table)
    _tally(N, name, res.info)
    TOTALS["oracle_cases"] += 1
    if N == W.WIDTHS[-1]:                            # the oracle on the wide operands themselves
        wide = port.spgemm(M, K, N, *acsc, *bw)
        assert wide["partials"] == P and np.array_equal(wide["rowptr"], want["rowptr"])
        assert np.array_equal(wide["colidx"], W.relabel(want["colidx"], table))
        assert_same_bits(wide["vals"], want["vals"])
    res.close()
    cap = max(P // 3, rowlen, 1)                     # panels: the capacity must hold the longest row
    res = mctx.spgemm_csc_csr(M, K, N, *acsc, *bw, partial_capacity=cap)
    _same_product(res, want, table)
    _tally(N, name, res.info)
    res.close()
    end = 0
    for i in range(3):                               # row shards
        r = mctx.spgemm_csc_csr(M, K, N, *acsc, *bw, partial_capacity=cap, row_shard=(i, 3))
        assert r.info["row_begin"] == end
        end = r.info["row_end"]
        _same_product(r, want, table, r.info["row_begin"], end)
        _tally(N, name, r.info)
        r.close()
    assert end == M
    kr = (K // 4, K - K // 4)                        # a k range
    rk = mctx.spgemm_csc_csr(M, K, N, *acsc, *bw, k_range=kr)
    _same_product(rk, _oracle(port, case, kr), table)
    _tally(N, name, rk.info)
    rk.close()


def test_the_narrow_cases_reach_the_paths_they_are_there_for(mctx, port, monkeypatch):
    """The planner side, at the cases' own narrow width: which case is there for which path."""
    reach = {"skew_3": ("heavy_rows",), "long_rows_dense": ("heavy_rows", "dense_segments"), "long_rows_pile": ("heavy_rows", "sorted_segments"),
             "stretch": ("heavy_rows",), "planned_gathered": ("direct_rows", "gathered_rows"), "planned_written": ("direct_rows",)}
    for case, paths in reach.items():
        M, K, n, acsc, bcsr, _ = _product_case(case)
        with monkeypatch.context() as mp:
            for k, v in PRODUCTS[case][2].items():
                mp.setenv(k, v)
            res = mctx.spgemm_csc_csr(M, K, n, *acsc, *bcsr)
        _same_product(res, _oracle(port, case), np.arange(n, dtype=np.uint32))
        assert all(res.info[p] > 0 for p in paths), (case, res.info)
        if case == "planned_written":
            assert res.info["gathered_rows"] == 0
        res.close()


def _tile_case(N, dt):
    """3 R + 1 output rows of six products each (R = the most rows a tile may hold at this width; 255 * 6 products fit a
    tile): EVERY row holds column 0 and column N - 1, each fed by two products, so whichever rows a tile begins and ends
    with, its first row holds column 0 and its last row column N - 1 -- at N = 2^31 the packed key of that entry (local row
    1, column 2^31 - 1) is all ones.  The middle columns sit on both sides of bit 31."""
    R = W.TILE_ROWS[N]
    M, K = 3 * R + 1, 8
    rng = np.random.default_rng(N % 1000)
    mids = np.array([1, N // 2 - 1, N // 2, N - 2], np.int64)
    while len(mids) < K:
        mids = np.unique(np.concatenate([mids, rng.integers(2, N - 2, K - len(mids))]))
    mids = mids.astype(np.uint32)
    b_rows = np.repeat(np.arange(K, dtype=np.uint32), 3)
    b_cols = np.stack([np.zeros(K, np.uint32), np.sort(mids), np.full(K, N - 1, np.uint32)], 1).reshape(-1)
    i = np.arange(M, dtype=np.uint32)
    a_rows = np.repeat(i, 2)
    a_cols = np.stack([i % K, (3 * i + 1) % K], 1)
    a_cols[a_cols[:, 0] == a_cols[:, 1], 1] += 1
    a_cols %= K
    a = (a_rows, a_cols.reshape(-1).astype(np.uint32), rng.uniform(-1.5, 1.5, 2 * M))
    b = (b_rows, b_cols, rng.uniform(-1.5, 1.5, 3 * K))
    return M, K, R, _csc_csr(M, K, a, b, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_a_tile_of_the_most_rows_with_column_0_and_column_N_minus_1(ctx, port, N, dt):
    M, K, R, (acsc, bcsr) = _tile_case(N, dt)
    want = port.spgemm(M, K, N, *acsc, *bcsr)          # the oracle on the wide operands
    first, last = want["rowptr"][:-1], want["rowptr"][1:] - 1
    assert np.all(want["colidx"][first] == 0) and np.all(want["colidx"][last] == N - 1) and want["partials"] == 6 * M
    if N == 1 << 31:
        assert (1 << W.bits_for(N)) | int(want["colidx"][last[1]]) == 0xffffffff
    res = ctx.spgemm_csc_csr(M, K, N, *acsc, *bcsr)
    assert res.info["partials"] == 6 * M and res.info["heavy_rows"] == 0
    assert np.array_equal(res.rowptr, want["rowptr"]) and np.array_equal(res.colidx, want["colidx"])
    assert_same_bits(res.vals, want["vals"])
    # a tile holds at most R rows, and the greedy packing fills it: 6 R products are within a tile's capacity
    assert res.info["light_tiles"] == -(-M // R) == 4, res.info
    res.close()
    res = ctx.spgemm_csc_csr(M, K, N, *acsc, *bcsr, partial_capacity=6 * (R + 1))
    assert res.info["panels"] > 1
    assert np.array_equal(res.rowptr, want["rowptr"]) and np.array_equal(res.colidx, want["colidx"])
    assert_same_bits(res.vals, want["vals"])
    res.close()


@pytest.mark.parametrize("name", W.MAPS)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_coo_products(ctx, port, N, name):
    M, K, n, acsc, bcsr, _ = _product_case("skew_1")
    table = W.phi(name, n, N)
    bw = W.relabel_csr(bcsr, table)
    want = port.spgemm(M, K, N, *acsc, *bw)            # the oracle on the wide operands
    rng = np.random.default_rng(5)
    a = (acsc[1], _rows_of(acsc[0]).astype(np.uint32), acsc[2])          # COO in any order
    b = (_rows_of(bw[0]).astype(np.uint32), bw[1], bw[2])
    pa, pb = rng.permutation(len(a[0])), rng.permutation(len(b[0]))
    res = ctx.spgemm_coo(M, K, N, tuple(x[pa] for x in a), tuple(x[pb] for x in b))
    assert res.info["partials"] == want["partials"]
    assert np.array_equal(res.rowptr, want["rowptr"]) and np.array_equal(res.colidx, want["colidx"])
    assert_same_bits(res.vals, want["vals"])
    _tally(N, name, res.info)
    res.close()


# osp_spgemm_masked makes a column view of B: N + 1 int64 offsets on the device, whatever the operands hold (its header says
# so).  That is 128 MiB at 2^24 and 256 MiB at 2^25 + 1, and 2 GiB and more at every other width of W.WIDTHS: beyond what a
# test of this file may hold, so the masked product belongs with the O(N) operations and runs at these two widths.
MASKED_WIDTHS = [1 << 24, W.LINEAR_WIDTH]


@pytest.mark.parametrize("name", W.MAPS)
@pytest.mark.parametrize("N", MASKED_WIDTHS)
def test_masked_products(ctx, port, N, name):
    M, K, n, acsc, bcsr, _ = _product_case("skew_1")
    table = W.phi(name, n, N)
    bw = W.relabel_csr(bcsr, table)
    want = port.spgemm(M, K, N, *acsc, *bw)            # the oracle on the wide operands
    rng = np.random.default_rng(5)
    # the mask: half of the product's pattern, as many coordinates beside it, and column 0 and N - 1 of every row
    rows = _rows_of(want["rowptr"])
    keep = rng.random(len(rows)) < 0.5
    other_r, other_c = rng.integers(0, M, len(rows) // 2), W.relabel(rng.integers(0, n, len(rows) // 2), table).astype(np.int64)
    r = np.concatenate([rows[keep], other_r, np.arange(M), np.arange(M)])
    c = np.concatenate([want["colidx"][keep].astype(np.int64), other_c, np.zeros(M, np.int64), np.full(M, N - 1, np.int64)])
    order = np.lexsort((c, r))
    first = np.ones(len(order), bool)
    first[1:] = (r[order][1:] != r[order][:-1]) | (c[order][1:] != c[order][:-1])
    mr, mc = r[order][first], c[order][first].astype(np.uint32)
    m_rowptr = np.concatenate([[0], np.cumsum(np.bincount(mr, minlength=M))]).astype(np.int64)
    res = ctx.spgemm_masked(M, K, N, *acsc, *bw, m_rowptr, mc)
    rp, ci, va = gmasked._filtered(want, M, N, m_rowptr, mc)
    assert 0 < len(ci) < len(want["colidx"])
    assert np.array_equal(res.rowptr, rp) and np.array_equal(res.colidx, ci)
    assert_same_bits(res.vals, va)
    prow, pcol = mxm_masked_model.product_columns(_csr_of_csc(acsc, M), bw)
    assert res.info["partials"] == int(np.isin(prow * N + pcol, mr * N + mc.astype(np.int64)).sum())
    res.close()


# a kernel that takes one thread each in blocks of 256 can be launched for at most (2^24 - 1) * 256 items (kThreadEachMax)
THREAD_EACH_MAX = (1 << 32) - 256
FIRST_REFUSED = THREAD_EACH_MAX            # the first N whose N + 1 offsets are beyond that


def test_the_bound_of_the_refusals_is_the_launch_bound():
    """Whole blocks of 256 threads for n items, fewer than 2^32 threads a launch: n = N + 1 <= 2^32 - 256."""
    threads = lambda n: -(-n // 256) * 256   # noqa: E731
    assert threads(FIRST_REFUSED) == (1 << 32) - 256 < 1 << 32                 # N = FIRST_REFUSED - 1: N + 1 items
    assert all(threads(N + 1) >= 1 << 32 for N in (FIRST_REFUSED, FIRST_REFUSED + 1, W.WIDTHS[-1]))
    assert W.WIDTHS[-1] >= FIRST_REFUSED > W.WIDTHS[-2]


@pytest.mark.parametrize("N", [FIRST_REFUSED, FIRST_REFUSED + 1, W.WIDTHS[-1]])
def test_the_masked_product_refuses_what_its_views_cannot_be_launched_for(mctx, N):
    """The column view of B takes N + 1 offsets, one thread each in blocks of 256 (the row view of A M + 1, the validation
    K + 1): from N = 2^32 - 256 on that is 2^32 threads, more than a launch takes.  The call is refused with OSP_ERR_ARG before
    anything is launched or allocated, and the caller's handle is left alone (the header says so).  The last N it takes,
    2^32 - 257, cannot be run here: its view alone is 32 GiB (test_the_bound_of_the_refusals_is_the_launch_bound holds the
    bound to the launch's arithmetic instead)."""
    import ctypes
    a = (np.array([0, 1, 2], np.int64), np.array([0, 1], np.uint32), np.array([1.0, 2.0]))            # 2 x 2, CSC
    b = (np.array([0, 2, 3], np.int64), np.array([0, N - 1, 5], np.uint32), np.array([3.0, 4.0, 5.0]))
    mask = (np.array([0, 1, 2], np.int64), np.array([N - 1, 5], np.uint32))
    with pytest.raises(S.OspError) as ei:
        mctx.spgemm_masked(2, 2, N, *a, *b, *mask)
    assert ei.value.status == _lib.ERR_ARG and "2^32 - 256" in str(ei.value)
    sentinel = 0x1234
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for M_, K_, N_ in ((2, 2, N), (N, 2, 5), (2, N, 5)):    # (the dimension check comes before any array is read)
        out = ctypes.c_void_p(sentinel)
        st = _lib.lib().osp_spgemm_masked(mctx._h, _lib.OSP_F64, M_, K_, N_, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(b[0]), ptr(b[1]), ptr(b[2]),
                                          ptr(mask[0]), ptr(mask[1]), _lib.OSP_HOST, None, ctypes.byref(out))
        assert st == _lib.ERR_ARG and out.value == sentinel, (M_, K_, N_)
    res = mctx.spgemm_csc_csr(2, 2, N, *a, *b)          # the unmasked product takes the width
    assert res.colidx.tolist() == [0, N - 1, 5] and res.vals.tolist() == [3.0, 4.0, 10.0]
    # ... and so does a result of that width, but its transpose has N + 1 row pointers written one thread each: refused too
    sent = ctypes.c_void_p(sentinel)
    stats = _lib.TransposeStats()
    stats.nnz = 77
    st = _lib.lib().osp_csr_transpose(res._h, None, ctypes.byref(sent), ctypes.byref(stats))
    assert st == _lib.ERR_ARG and sent.value == sentinel and stats.nnz == 77
    with pytest.raises(S.OspError) as ei:
        res.transpose()
    assert ei.value.status == _lib.ERR_ARG
    res.close()


def _csr_of_csc(csc, M):
    """(rowptr, col) of the pattern of a CSC operand with M rows."""
    colptr, rowidx = csc[0], csc[1].astype(np.int64)
    col = _rows_of(colptr)
    order = np.lexsort((col, rowidx))
    return np.concatenate([[0], np.cumsum(np.bincount(rowidx, minlength=M))]).astype(np.int64), col[order].astype(np.uint32)


# ==== the result operations ===============================================================================================================
@functools.lru_cache(maxsize=None)
def _unary(dt):
    """Operands A (special values, an all-NaN row) and P (small positive values) of result_chain.starting_operands."""
    ops = {name: (ncol, tuple(csr)) for name, ncol, csr in result_chain.starting_operands(0, dt)}
    (n, A), (n2, P) = ops["A"], ops["P"]
    assert n == n2 and len(A[0]) == len(P[0]) == n + 1
    mask = am._mask_for(A[0], A[1], n, seed=4)
    return n, A, P, mask


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_mxm_every_semiring_masked_and_matmul(mctx, N, dt):
    a, b = gm._pair(dt)
    ra = _upload(mctx, gm.K, a)
    try:
        for name in W.MAPS:
            table = W.phi(name, gm.N, N)
            bw = W.relabel_csr(b, table)
            rb = _upload(mctx, N, bw)
            try:
                for add, mul in gm.SEMIRINGS:
                    want, wst = gm._want(dt, add, mul)
                    res, st = ra.mxm(rb, add, mul)
                    try:
                        assert res.shape == (len(gm.A_ROWS), N) and res.dtype == dt
                        _same(res, W.relabel_csr(want, table), True, (name, add, mul))
                        gm._check_stats(st, res, wst, a, bw)
                    finally:
                        res.close()
                want, wst = semiring_model.mxm(a, bw, N, "min", "plus")            # the model on the wide operands
                res, st = ra.mxm(rb, "min", "plus")
                _same(res, want, True, name)
                res.close()
                # the pile at column 7 moved with the map: row 10's entry there is fed by 5000 products
                full = gm._want(dt, "plus", "times")[0]
                assert table[7] in W.relabel(full[1][full[0][10]:full[0][11]], table)
                # the masked product, both senses: the mask is half the product's pattern and columns 0 and N - 1 of every row
                rng = np.random.default_rng(6)
                M = len(gm.A_ROWS)
                rows = _rows_of(full[0])
                keep = rng.random(len(rows)) < 0.5
                mkey = np.unique(np.concatenate([rows[keep] * gm.N + full[1][keep], np.arange(M) * gm.N, np.arange(M) * gm.N + gm.N - 1]))
                mask = (np.concatenate([[0], np.cumsum(np.bincount(mkey // gm.N, minlength=M))]).astype(np.int64), (mkey % gm.N).astype(np.uint32))
                mask_w = (mask[0], W.relabel(mask[1], table), np.ones(len(mask[1]), np.float32))
                rm = _upload(mctx, N, mask_w)
                try:
                    for add, mul in (("plus", "times"), ("min", "second")):
                        wfull, wst = gm._want(dt, add, mul)
                        for complement in (False, True):
                            want, mst = mxm_masked_model.filter_product(wfull, wst, a, b, mask, gm.N, complement)
                            res, st = ra.mxm(rb, add, mul, mask=rm, complement=complement)
                            try:
                                _same(res, W.relabel_csr(want, table), True, (name, add, mul, complement))
                                assert {k: st[k] for k in mst} == mst, (st, mst)
                                assert 0 < mst["products_kept"] < mst["products"]
                            finally:
                                res.close()
                finally:
                    rm.close()
                # the pipeline product with the wide operand on the right: mxm(plus, times) bit for bit
                res = ra.matmul(rb)
                try:
                    assert res.shape == (M, N) and res.info["partials"] == gm._want(dt, "plus", "times")[1]["products"]
                    _same(res, W.relabel_csr(full, table), False, name)
                    _tally(N, name, res.info)
                finally:
                    res.close()
            finally:
                rb.close()
    finally:
        ra.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_apply_mask_with_host_device_and_result_masks(mctx, N, dt):
    n, A, _, mask = _unary(dt)
    for name in W.MAPS:
        table = W.phi(name, n, N)
        Aw, mw = W.relabel_csr(A, table), (mask[0], W.relabel(mask[1], table))
        src = _upload(mctx, N, Aw)
        msk = _upload(mctx, N, (mw[0], mw[1], np.ones(len(mw[1]), dt)))
        dmask = [_dev(mw[0]), _dev(mw[1])]
        torch.cuda.synchronize(DEV)
        try:
            for complement in (False, True):
                want = W.relabel_csr(bfs_model.apply_mask(*A, *mask, n, complement), table)
                wide = bfs_model.apply_mask(*Aw, *mw, N, complement)               # the model on the wide operands
                assert np.array_equal(wide[1], want[1]) and 0 < len(want[1]) < len(A[1])
                for how in ("host", "device", "result"):
                    if how == "result":
                        res, st = src.apply_mask(msk, complement=complement, validate=True)
                    else:
                        m = mw if how == "host" else (dmask[0].data_ptr(), dmask[1].data_ptr())
                        res, st = src.apply_mask(m, complement=complement, space=how)
                    try:
                        assert res.shape == (n, N)
                        _same(res, want, False, (name, complement, how))
                        assert (st["nnz_in"], st["nnz_mask"], st["nnz_out"]) == (len(A[1]), len(mask[1]), len(want[1]))
                    finally:
                        res.close()
        finally:
            src.close()
            msk.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_select_every_value_and_positional_op(mctx, N, dt):
    n, A, _, _ = _unary(dt)
    for name in W.MAPS:
        table = W.phi(name, n, N)
        Aw = W.relabel_csr(A, table)
        src = _upload(mctx, N, Aw)
        try:
            for op in truss_model.VALUE_OPS:
                for fill in (None, 2.5):
                    want = W.relabel_csr(truss_model.select(*A, op, 0.5, fill=fill), table)
                    res, st = src.select(op, 0.5, fill=fill)
                    try:
                        _same(res, want, False, (name, op, fill))
                        assert (st["nnz_in"], st["nnz_out"]) == (len(A[1]), len(want[1]))
                    finally:
                        res.close()
            kept = collections.Counter()
            for op in truss_model.POSITION_OPS:
                for diag in (0, 1, -1, N - 2, -(N - 2), 1 << 33):
                    want = truss_model.select(*Aw, op, diag=diag)                  # the model on the wide operand: Python integers
                    res, st = src.select(op, diag=diag)
                    try:
                        _same(res, want, False, (name, op, diag))
                        assert (st["nnz_in"], st["nnz_out"]) == (len(A[1]), len(want[1]))
                        kept[op, diag] = len(want[1])
                    finally:
                        res.close()
            # a diagonal beyond the matrix: everything is below it
            assert kept["tril", 1 << 33] == len(A[1]) and kept["triu", 1 << 33] == 0
            if name == "straddle":   # the lower half of the columns is where it was: the small diagonals cut through it
                for op in ("tril", "triu", "offdiag"):
                    assert all(0 < kept[op, d] < len(A[1]) for d in (0, 1, -1)), (op, kept)
                assert 0 < kept["diag", 0] < len(A[1])
        finally:
            src.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_ewise_union_intersect_and_self(mctx, N, dt):
    n, A, P, _ = _unary(dt)
    plan = ewise_model.Plan(A, P, n)
    assert 0 < plan.nnz_both < min(len(A[1]), len(P[1]))
    for name in W.MAPS:
        table = W.phi(name, n, N)
        ra, rp = _upload(mctx, N, W.relabel_csr(A, table)), _upload(mctx, N, W.relabel_csr(P, table))
        try:
            for mode in ewise_model.MODES:
                for op in (ewise_model.UNION_OPS if mode == "union" else ewise_model.OPS):
                    rowptr, col, val, computed = plan.result(mode, op)
                    res, st = ra.ewise(rp, mode, op)
                    try:
                        _same(res, (rowptr, W.relabel(col, table), val), computed & (op not in ewise_model.COPY_OPS), (name, mode, op))
                        assert (st["nnz_a"], st["nnz_b"], st["nnz_both"], st["nnz_out"]) == (len(A[1]), len(P[1]), plan.nnz_both, len(col))
                    finally:
                        res.close()
            for mode, op in (("union", "plus"), ("intersect", "times"), ("intersect", "minus")):
                rowptr, col, val = ewise_model.ewise(A, A, n, mode, op)
                res, st = ra.ewise(ra, mode, op)
                try:
                    _same(res, (rowptr, W.relabel(col, table), val), True, (name, mode, op, "self"))
                    assert st["nnz_both"] == st["nnz_out"] == len(A[1])
                finally:
                    res.close()
        finally:
            ra.close()
            rp.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_inflate_prune(mctx, N, dt):
    n, _, P, _ = _unary(dt)
    for name in W.MAPS:
        table = W.phi(name, n, N)
        src = _upload(mctx, N, W.relabel_csr(P, table))
        try:
            for power, thr, cap in ((2.0, 0.0, 0), (2.0, 0.4, 5), (1.0, 2.0, 3)):
                rowptr, col, val, want = mcl_model.inflate_prune(*P, power, thr, cap)
                res, st = src.inflate_prune(power, thr, cap)
                try:
                    _same(res, (rowptr, W.relabel(col, table), val), False, (name, power, thr, cap))
                    assert {k: st[k] for k in want} == want
                finally:
                    res.close()
        finally:
            src.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_build_with_every_dup_op(mctx, N, dt):
    n, A, _, _ = _unary(dt)
    M = n
    rng = np.random.default_rng(9)
    rows, cols, vals = _rows_of(A[0]), A[1].astype(np.int64), A[2]
    extra = rng.integers(0, len(rows), 3000)                                     # repeats of random coordinates ...
    rows = np.concatenate([rows, rows[extra], np.full(7, M - 1), [0]])           # ... of (M - 1, N - 1), and (0, 0) once
    cols = np.concatenate([cols, cols[extra], np.full(7, n - 1), [0]])
    vals = np.concatenate([vals, rng.standard_normal(3000).astype(dt), rng.standard_normal(8).astype(dt)])
    order = rng.permutation(len(rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    for name in W.MAPS:
        table = W.phi(name, n, N)
        wide = W.relabel(cols, table)
        assert int(wide.max()) == N - 1
        for dup in build_model.DUP_OPS:
            if dup == "error":
                with pytest.raises(S.OspError) as ei:
                    mctx.build(M, N, rows, wide, vals, dup=dup, dtype=dt)
                assert ei.value.status == _lib.ERR_DUPLICATE
                u = np.unique(rows * n + cols, return_index=True)[1]            # a list without repeats passes
                want, wst, _ = build_model.build(M, N, rows[u], wide[u], vals[u], dup, dt)
                res, st = mctx.build(M, N, rows[u], wide[u], vals[u], dup=dup, dtype=dt)
            else:
                want, wst, _ = build_model.build(M, N, rows, wide, vals, dup, dt)  # the model on the wide list
                narrow = build_model.build(M, n, rows, cols, vals, dup, dt)[0]
                assert np.array_equal(want[1], W.relabel(narrow[1], table)) and np.array_equal(_bits(want[2]), _bits(narrow[2]))
                res, st = mctx.build(M, N, rows, wide, vals, dup=dup, dtype=dt)
            try:
                assert res.shape == (M, N)
                _same(res, want, dup == "plus", (name, dup))
                assert res.colidx[-1] == N - 1 and res.rowptr[-1] - res.rowptr[-2] >= 1
                assert {k: st[k] for k in wst} == wst, (name, dup, st, wst)
            finally:
                res.close()
        with pytest.raises(S.OspError) as ei:                                      # column N is outside, N - 1 is not
            mctx.build(M, N, [0, 1], [N - 1, N], None, dtype=dt)
        assert ei.value.status == _lib.ERR_RANGE


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_the_row_side_operations(mctx, N, dt):
    """extract and a permutation by rows, select_vertices with keep_rows, apply_vectors with a row vector, reduce over rows."""
    n, A, _, _ = _unary(dt)
    M = n
    rng = np.random.default_rng(10)
    lists = {"repeats": np.concatenate([rng.integers(0, M, 500), [M - 1, 0, M - 1]]), "permutation": rng.permutation(M)}
    keep_rows = (rng.random(M) < 0.5).astype(np.uint8)
    vec = rng.standard_normal(M).astype(dt)
    for name in W.MAPS:
        table = W.phi(name, n, N)
        Aw = W.relabel_csr(A, table)
        src = _upload(mctx, N, Aw)
        try:
            for what, rows in lists.items():
                want, wst = extract_model.extract(*Aw, N, rows=rows)              # the model on the wide operand
                res, st = src.extract(rows=rows, space="host")
                try:
                    assert res.shape == (len(rows), N)
                    _same(res, want, False, (name, what))
                    assert {k: st[k] for k in wst} == wst and not st["composed"]
                finally:
                    res.close()
            want = vector_model.select_vertices(*Aw, keep_rows=keep_rows)
            res, st = src.select_vertices(keep_rows=keep_rows, space="host")
            try:
                _same(res, want, False, name)
                assert (st["nnz_in"], st["nnz_out"]) == (len(A[1]), len(want[1])) and 0 < len(want[1]) < len(A[1])
            finally:
                res.close()
            for op in ("times", "plus", "second", "min"):
                val, computed = vector_model.apply_vectors(*Aw, rows=vec, row_op=op)
                res, st = src.apply_vectors(rows=vec, row_op=op, space="host")
                try:
                    _same(res, (Aw[0], Aw[1], val), computed, (name, op))
                finally:
                    res.close()
            for op in vector_model.REDUCE_OPS:
                want, nlong = vector_model.reduce(*Aw, N, "rows", op)
                got, st = src.reduce("rows", op)
                _same_values(got, want, op == "plus", (name, op))
                assert (st["nnz_in"], st["nnz_out"], st["long_segments"]) == (len(A[1]), M, nlong)
        finally:
            src.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", W.WIDTHS)
def test_the_forms_that_read_no_length_N_operand(mctx, N, dt):
    """mul = "first" and no operand: mxv, mxv_arg (min and max, values on and off: the int64 positions are the UNSIGNED
    columns), mxd, sddmm."""
    n, A, _, _ = _unary(dt)
    M = n
    rng = np.random.default_rng(11)
    X = rng.standard_normal((M, 3)).astype(dt)
    for name in W.MAPS:
        table = W.phi(name, n, N)
        Aw = W.relabel_csr(A, table)
        src = _upload(mctx, N, Aw)
        try:
            for add in mxv_model.ADD_OPS:
                want, nlong = mxv_model.mxv(*Aw, None, add, "first")
                got, st = src.mxv(None, add, "first", space="host")
                _same_values(got, want, add == "plus", (name, add))
                assert (st["nnz_in"], st["nnz_out"], st["long_segments"]) == (len(A[1]), M, nlong)
                wantd, _ = mxd_model.mxd(*Aw, None, add, "first", k=3)
                gotd, st = src.mxd(None, add, "first", space="host", k=3)
                _same_values(gotd, wantd, add == "plus", (name, add, "mxd"))
                for accum in ("second", "plus"):
                    wants, computed = sddmm_model.sddmm(*Aw, X, None, add, "first", accum)
                    res, st = src.sddmm(X, None, add, "first", accum, space="host")
                    try:
                        _same(res, (Aw[0], Aw[1], wants), computed, (name, add, accum))
                    finally:
                        res.close()
            for add in mxv_arg_model.ADD_OPS:
                y, arg, nlong, without = mxv_arg_model.mxv_arg(*Aw, None, add, "first")
                assert arg.dtype == np.int64 and arg.min() == -1 and arg.max() < N
                assert arg.max() >= 1 << 31 or N < W.WIDTHS[-1] or name == "spread"       # (winners with bit 31 set, where many columns have it)
                for values in (True, False):
                    got, garg, st = src.mxv_arg(None, add, "first", space="host", values=values)
                    assert garg.dtype == np.int64 and np.array_equal(garg, arg), (name, add, values)
                    assert (got is None) == (not values)
                    if values:
                        _same_values(got, y, False, (name, add))
                    assert (st["rows_without"], st["long_segments"]) == (without, nlong)
        finally:
            src.close()
    # the edge columns as winners, whatever the operand above holds: rows {0}, {N - 1}, {0, N - 1}, {}, {N - 2, N - 1}
    edge = (np.array([0, 1, 2, 4, 4, 6], np.int64), np.array([0, N - 1, 0, N - 1, N - 2, N - 1], np.uint32), np.array([1, 2, 3, 4, 6, 5], dt))
    src = _upload(mctx, N, edge)
    try:
        for add, winners in (("max", [0, N - 1, N - 1, -1, N - 2]), ("min", [0, N - 1, 0, -1, N - 1])):
            y, arg, _, without = mxv_arg_model.mxv_arg(*edge, None, add, "first")
            assert arg.tolist() == winners and without == 1
            got, garg, st = src.mxv_arg(None, add, "first", space="host")
            assert garg.tolist() == winners and st["rows_without"] == 1, (add, garg)
            _same_values(got, y)
            dev_y, dev_arg, _ = src.mxv_arg(None, add, "first", values=False)      # positions only, on the device
            assert dev_y is None and dev_arg.dtype == torch.int64 and dev_arg.cpu().tolist() == winners
    finally:
        src.close()


# ==== a short chain at the full width ====================================================================================================
@pytest.mark.parametrize("dt", DTYPES)
def test_a_chain_at_the_full_width(mctx, dt):
    """mxm, select, ewise with itself, apply_mask, extract by rows, masked mxm, reduce over rows on N = 2^32 - 1, each step
    against its model on the previous step's model answer; results are closed in between, so pool buffers recycle."""
    N = W.WIDTHS[-1]
    a, b = gm._pair(dt)
    table = W.phi("straddle", gm.N, N)
    bw = W.relabel_csr(b, table)
    M = len(gm.A_ROWS)
    ra, rb = _upload(mctx, gm.K, a), _upload(mctx, N, bw)
    step = {}
    try:
        w1, _ = semiring_model.mxm(a, bw, N, "plus", "times")
        step[1], _ = ra.mxm(rb)
        _same(step[1], w1, True, "mxm")
        rb.close()
        w2 = truss_model.select(*w1, "gt", 0.0)
        step[2], _ = step[1].select("gt", 0.0)
        _same(step[2], w2, False, "select")
        wm = truss_model.select(*w1, "lt", 1.0)                                   # the mask of the later steps
        step["mask"], _ = step[1].select("lt", 1.0)
        _same(step["mask"], wm, False, "select lt")
        wt = truss_model.select(*w1, "triu", diag=1 << 31)                        # columns at or beyond row + 2^31: the upper half
        tri, _ = step[1].select("triu", diag=1 << 31)
        try:
            _same(tri, wt, False, "triu")
        finally:
            tri.close()
        assert 0 < len(wt[1]) < len(w1[1]) and wt[1].min() >= 1 << 31
        step.pop(1).close()
        w3 = ewise_model.ewise(w2, w2, N, "union", "plus")
        step[3], _ = step[2].ewise(step[2], "union", "plus")
        _same(step[3], w3, True, "ewise")
        step.pop(2).close()
        w4 = bfs_model.apply_mask(*w3, wm[0], wm[1], N)
        step[4], _ = step[3].apply_mask(step["mask"])
        _same(step[4], w4, False, "apply_mask")
        assert 0 < len(w4[1]) < len(w3[1]) and w4[1].min() < 1 << 31 <= w4[1].max()
        step.pop(3).close()
        rows = [10, 9, 9, 17, 0, 12, 5, 19]
        w5, _ = extract_model.extract(*w4, N, rows=rows)
        step[5], _ = step[4].extract(rows=rows, space="host")
        _same(step[5], w5, False, "extract")
        step.pop(4).close()
        # a left operand of M x 8 over the extracted rows; the mask's complement
        rng = np.random.default_rng(12)
        has = rng.random((M, len(rows))) < 0.5
        left = (np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int64), np.nonzero(has)[1].astype(np.uint32),
                rng.standard_normal(int(has.sum())).astype(dt))
        step["left"] = _upload(mctx, len(rows), left)
        w6, _ = mxm_masked_model.mxm_masked(left, w5, wm, N, True, "min", "plus")
        step[6], _ = step["left"].mxm(step[5], "min", "plus", mask=step["mask"], complement=True)
        _same(step[6], w6, True, "masked mxm")
        assert 0 < len(w6[1]) and w6[1].min() < 1 << 31 <= w6[1].max()
        step.pop(5).close()
        w7, _ = vector_model.reduce(*w6, N, "rows", "max")
        got, _ = step[6].reduce("rows", "max")
        _same_values(got, w7, False, "reduce")
    finally:
        for r in list(step.values()) + [ra]:
            r.close()


# ==== the operations with an O(N) footprint: once each, at N = 2^25 + 1 =================================================================
LN = W.LINEAR_WIDTH
MUST = [0, 1 << 24, (1 << 24) + 1, LN - 1]


@functools.lru_cache(maxsize=None)
def _linear_case():
    """70 rows (beyond the transpose's row-mask path) over 200 occupied columns of [0, 2^25 + 1), float32: columns 0, 2^24,
    2^24 + 1 and N - 1 among them, each in a row of its own and in a full row."""
    rng = np.random.default_rng(13)
    n, M, dt = 200, 70, np.float32
    table = W.table_through(n, LN, MUST, seed=14)
    has = rng.random((M, n)) < 0.2
    has[7] = True
    has[40] = False
    rows, cols = np.nonzero(has)
    csr = (np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int64), table[cols], rng.standard_normal(len(cols)).astype(dt))
    assert set(MUST) <= set(csr[1].tolist())
    return M, table, csr


@pytest.fixture
def linear(mctx):
    M, table, csr = _linear_case()
    src = _upload(mctx, LN, csr)
    yield M, table, csr, src
    src.close()
    mctx.trim()
    torch.cuda.empty_cache()


def test_transpose_at_2_to_25_plus_1(linear):
    M, table, csr, src = linear
    want = transpose_model.transpose(*csr, LN)
    res, st = src.transpose()
    try:
        assert res.shape == (LN, M) and st["path"] == 2 and st["passes"] == transpose_model.passes(LN) == 4
        _same(res, want)
        for c in MUST:
            assert res.rowptr[c + 1] - res.rowptr[c] >= 1
        back, _ = res.transpose()                       # 2^25 + 1 rows, 70 columns: twice gives the three arrays back
        _same(back, csr)
        back.close()
    finally:
        res.close()


def test_reduce_over_columns_at_2_to_25_plus_1(linear):
    M, table, csr, src = linear
    for op in ("plus", "count", "max"):
        want, nlong = vector_model.reduce(*csr, LN, "cols", op)
        got, st = src.reduce("cols", op)
        _same_values(got, want, False, op)
        assert st["nnz_out"] == LN and st["long_segments"] == nlong
        if op == "count":
            assert all(want[c] >= 1 for c in MUST) and want[1] == 0


def test_extract_and_select_vertices_by_columns_at_2_to_25_plus_1(linear):
    M, table, csr, src = linear
    cols = np.unique(np.concatenate([MUST, table[::3], [1, (1 << 24) - 1, LN - 2]]))      # ascending; some name no entry
    want, wst = extract_model.extract(*csr, LN, rows=[3, 7, 7, 69], cols=cols)
    res, st = src.extract(rows=[3, 7, 7, 69], cols=cols, space="host")
    try:
        assert res.shape == (4, len(cols)) and not st["composed"]
        _same(res, want)
        assert {k: st[k] for k in wst} == wst and 0 < wst["nnz_out"] < wst["nnz_gathered"]
    finally:
        res.close()
    keep = np.zeros(LN, np.uint8)
    keep[cols] = 1
    want = vector_model.select_vertices(*csr, keep_cols=keep)
    res, st = src.select_vertices(keep_cols=keep, space="host")
    try:
        _same(res, want)
        assert set(MUST) <= set(res.colidx.tolist()) and 0 < res.nnz < len(csr[1])
    finally:
        res.close()


def _column_vector(seed):
    """2^25 + 1 distinct-looking float32 values in [0.5, 1.5): a neighbour's value in place of a column's shows."""
    return np.random.default_rng(seed).random(LN, np.float32) + np.float32(0.5)


def test_apply_vectors_with_a_column_vector_and_mxv_at_2_to_25_plus_1(linear):
    M, table, csr, src = linear
    x = _column_vector(15)
    val, computed = vector_model.apply_vectors(*csr, cols=x, col_op="times")
    res, st = src.apply_vectors(cols=x, col_op="times", space="host")
    try:
        _same(res, (csr[0], csr[1], val), computed)
    finally:
        res.close()
    for add, mul in (("plus", "times"), ("min", "second")):
        want, nlong = mxv_model.mxv(*csr, x, add, mul)
        got, st = src.mxv(x, add, mul, space="host")
        _same_values(got, want, add == "plus", (add, mul))
    y, arg, nlong, without = mxv_arg_model.mxv_arg(*csr, x, "max", "second")
    got, garg, st = src.mxv_arg(x, "max", "second", space="host")
    assert np.array_equal(garg, arg) and st["rows_without"] == without == 1
    _same_values(got, y)


def test_mxd_and_sddmm_with_real_operands_at_2_to_25_plus_1(linear):
    M, table, csr, src = linear
    rng = np.random.default_rng(16)
    Y = (rng.random((LN, 2), np.float32) - np.float32(0.5))                      # N x 2 float32: 256 MiB
    want, _ = mxd_model.mxd(*csr, Y, "plus", "times")
    got, st = src.mxd(Y, "plus", "times", space="host")
    _same_values(got, want, True, "mxd")
    X = rng.standard_normal((M, 2)).astype(np.float32)
    wants, computed = sddmm_model.sddmm(*csr, X, Y, "plus", "times", "second")
    res, st = src.sddmm(X, Y, "plus", "times", "second", space="host")
    try:
        _same(res, (csr[0], csr[1], wants), computed, "sddmm")
    finally:
        res.close()


def test_permute_at_2_to_25_plus_1(mctx):
    """``permute`` is ``extract(perm, perm)`` on a SQUARE result: 2^25 + 1 rows and columns, 300 entries with (0, 0),
    (N - 1, N - 1), (2^24, 2^24 + 1) and (N - 1, 0) among them, built with ``build``.  A permutation is not ascending, so the
    call goes through transpose, row gather, transpose, row gather; the five results it holds at the end have 2^25 + 2 row
    pointers each (the most this file holds at once: 1.3 GiB in arrays of 256 MiB)."""
    rng = np.random.default_rng(17)
    key = np.unique(np.concatenate([[0, LN * LN - 1, (1 << 24) * LN + (1 << 24) + 1, (LN - 1) * LN],
                                    rng.integers(0, LN, 296) * LN + rng.integers(0, LN, 296)]))
    rows, cols = key // LN, key % LN
    vals = rng.standard_normal(len(key)).astype(np.float32)
    perm = rng.permutation(LN).astype(np.uint32)
    perm[[0, int(np.flatnonzero(perm == LN - 1)[0])]] = perm[[int(np.flatnonzero(perm == LN - 1)[0]), 0]]   # vertex N - 1 becomes vertex 0
    assert perm[0] == LN - 1
    want = W.permuted((rows, cols, vals), perm, LN)
    src, _ = mctx.build(LN, LN, rows, cols, vals, dup="error", dtype=np.float32)
    try:
        assert src.shape == (LN, LN) and src.nnz == len(key)
        res, st = src.permute(perm, space="host")
        try:
            assert res.shape == (LN, LN) and st["composed"] and st["nnz_out"] == len(key)
            _same(res, want)
            assert res.rowptr[1] >= 1 and res.colidx[0] == 0            # in[N - 1, N - 1] is out[0, 0]
        finally:
            res.close()
    finally:
        src.close()
        mctx.trim()
        torch.cuda.empty_cache()
    wide = mctx.merge_csr_parts(2, LN, [(np.array([0, 1, 2], np.int64), np.array([0, LN - 1], np.uint32), np.ones(2, np.float32))])
    with pytest.raises(S.OspError) as ei:                               # not square: refused, whatever the width
        wide.permute([1, 0], space="host")
    assert ei.value.status == _lib.ERR_DIM
    wide.close()


# ==== coverage ============================================================================================================================
def test_the_wide_products_reached_the_hard_paths():
    """(runs after the products above) Each of long rows, sorted segments, direct rows, gathered rows and several panels was
    taken at least once at every width -- not only at and above 2^31, where colbits leaves 32-bit keys no row bits -- under every map: above 2^13 columns
    split_params_kernel's limits (osp_split.h) no longer depend on colbits, and panels follow the capacity alone.

    Dense segments are beyond the planner at EVERY width of this file, under every map, whatever the case: an over-long
    segment is accumulated densely when the column range it was cut for, [vcol0, vcol1), spans at most 2^kDenseBits = 2048
    columns (SegDenseFlag), and that range is a whole bin of the split, never the span of the columns that occur: 2^(colbits -
    b) columns with b <= kSplitMaxBits = 12 split bits (split and stretch rows, split_vrows_kernel; hub rows the same), or a
    group of such bins with b <= kDirectFineBits = 9 (direct rows).  From colbits = 24 on a bin is 4096 columns and more --
    only the last bin of colbits 32 is clamped, to 2^20 - 1 -- so even the pile at ONE column of the long-row case, which is
    a dense segment at its own 64 columns (test_the_narrow_cases_reach_the_paths_they_are_there_for), goes to the big
    in-place tile here, or with OSP_BIGTILE_CAP=0 to the sort.  Clustering (``top``, ``straddle``) does not help: the bins are
    not placed by the data.  The dense-segment cases run all the same, with OSP_DENSE_SEG on and off, and must equal the
    oracle; that the counter stays 0 is asserted, so that a planner which learns to place its ranges shows up here."""
    if TOTALS["oracle_cases"] < len(W.WIDTHS) * len(W.MAPS) * len(PRODUCTS):   # (every case of test_products_equal_the_oracle)
        pytest.skip("not the whole module ran")
    print("wide products:", dict(TOTALS))
    for N in W.WIDTHS:
        for name in W.MAPS:
            print(N, name, dict(SEEN[N, name]))
    missing = [(N, name, p) for N in W.WIDTHS for name in W.MAPS for p in PATHS if p != "dense_segments" and SEEN[N, name][p] == 0]
    assert not missing, missing
    assert TOTALS["dense_segments"] == 0
