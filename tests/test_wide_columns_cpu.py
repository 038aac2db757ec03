"""tests/wide_columns.py and the numpy models on column spaces of 2^24 to 2^32 - 1 columns (no GPU).

The GPU file (tests/test_gpu_wide_columns.py) judges the library at these widths by the models run on the wide operands, or
by a model's narrow answer with the relabeling applied to its columns.  Both are only as good as the models' own arithmetic
on wide columns (an int32 key, a signed cast, an O(N) array would spoil them), so every model the GPU file relies on is held
here to ``model(phi(case)) == phi(model(case))`` with identical value bits, at every width and under every map.  The
positional predicates of ``select`` compare a column with a row and are not equivariant: they are checked against a literal
loop in Python integers instead."""
import numpy as np
import pytest

from tests import bfs_model, build_model, ewise_model, extract_model, mcl_model, mxm_masked_model, mxv_arg_model, mxv_model
from tests import semiring_model, truss_model, vector_model
from tests import wide_columns as W

NARROW = 41          # columns of the narrow case (odd: "straddle" splits it 20 / 21)
DTYPES = [np.float32, np.float64]
COMBOS = [(N, m) for N in W.WIDTHS + [W.LINEAR_WIDTH] for m in W.MAPS]


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _same(got, want):
    """(rowptr, col, val) equal: pointers and columns as integers, values as bits."""
    assert np.array_equal(got[0], want[0])
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1])
    assert got[2].dtype == want[2].dtype and np.array_equal(_bits(got[2]), _bits(want[2]))


def _random_csr(rng, M, ncol, dt, fill=0.3, full_row=None):
    """A CSR with ascending columns; row ``full_row`` holds every column (so column 0 and column ncol - 1 occur)."""
    has = rng.random((M, ncol)) < fill
    has[M // 2] = False                       # an empty row
    if full_row is not None:
        has[full_row] = True
    rows, cols = np.nonzero(has)
    rowptr = np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int64)
    val = (rng.standard_normal(len(cols)) * 10.0 ** rng.integers(-2, 3, len(cols))).astype(dt)
    val[rng.choice(len(val), 4, replace=False)] = [np.nan, -0.0, np.inf, -np.inf]
    return rowptr, cols.astype(np.uint32), val


def _case(dt, seed=5):
    rng = np.random.default_rng(seed)
    a = _random_csr(rng, 9, 13, dt, 0.4)                       # 9 x 13
    b = _random_csr(rng, 13, NARROW, dt, 0.3, full_row=3)      # 13 x NARROW: the operand whose columns are relabeled
    c = _random_csr(rng, 13, NARROW, dt, 0.3, full_row=7)      # a second one of b's shape
    return a, b, c


# ---- the maps ---------------------------------------------------------------------------------------------------------------------
def test_the_widths_are_the_ones_the_forks_need():
    assert W.WIDTHS == [1 << 24, (1 << 28) + 5, 1 << 31, (1 << 31) + 1, 0xffffffff]
    assert [W.bits_for(N) for N in W.WIDTHS] == [24, 29, 31, 32, 32]
    # a tile's rows: min(255, 2^(32 - colbits)), one row at colbits 32 (osp_pipeline.h, pl.max_rows)
    assert [W.TILE_ROWS[N] for N in W.WIDTHS] == [min(255, 1 << (32 - W.bits_for(N))) if W.bits_for(N) < 32 else 1 for N in W.WIDTHS]
    assert W.TILE_ROWS[1 << 24] == 255 and 24 + 8 == 32             # the first 32-bit key
    assert (1 << 31 | ((1 << 31) - 1)) == 0xffffffff                 # N = 2^31: local row 1, column N - 1 is the all-ones key
    assert W.bits_for(W.LINEAR_WIDTH) == 26


@pytest.mark.parametrize("N,name", COMBOS)
@pytest.mark.parametrize("n", [1, 2, 3, NARROW, 3000, 1 << 16])
def test_maps_are_strictly_increasing_and_hit_their_endpoints(N, name, n):
    t = W.phi(name, n, N)
    assert t.dtype == np.uint32 and t.shape == (n,)
    wide = t.astype(np.int64)
    assert np.all(np.diff(wide) > 0) and wide[0] >= 0 and wide[-1] == N - 1     # column n - 1 becomes N - 1
    if name == "top":
        assert np.array_equal(wide, np.arange(n) + (N - n))
    if name == "spread" and n > 1:
        assert wide[0] == 0 and np.all(np.diff(wide)[:-1] == N // n) and wide[-1] - wide[-2] >= N // n
    if name == "straddle" and n > 1:
        h = n // 2
        assert np.array_equal(wide[:h], np.arange(h)) and np.array_equal(wide[h:], np.arange(h, n) + (N - n))
        if N > 1 << 31:
            assert wide[0] < 1 << 31 <= wide[-1]                                  # both sides of bit 31
    assert np.array_equal(W.relabel(np.array([0, n - 1], np.uint32), t), t[[0, -1]])


def test_a_map_that_is_not_increasing_is_refused():
    with pytest.raises(AssertionError):
        W._checked(np.array([1, 1], np.uint32), 2, 10)
    with pytest.raises(AssertionError):
        W._checked(np.array([1, 10], np.uint32), 2, 10)
    with pytest.raises(AssertionError):
        W.phi("top", 5, 1 << 32)
    t = W.table_through(50, W.LINEAR_WIDTH, [0, 1 << 24, (1 << 24) + 1, W.LINEAR_WIDTH - 1])
    assert {0, 1 << 24, (1 << 24) + 1, W.LINEAR_WIDTH - 1} <= set(t.tolist()) and len(t) == 50


# ---- the models are relabel-equivariant, and right, on wide columns -----------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,name", COMBOS)
def test_mxm_and_its_masked_form(N, name, dt):
    a, b, _ = _case(dt)
    t = W.phi(name, NARROW, N)
    bw = W.relabel_csr(b, t)
    for add, mul in (("plus", "times"), ("min", "plus"), ("first", "second")):
        narrow, st_n = semiring_model.mxm(a, b, NARROW, add, mul)
        wide, st_w = semiring_model.mxm(a, bw, N, add, mul)
        _same(wide, W.relabel_csr(narrow, t))
        assert st_w == st_n
        rng = np.random.default_rng(3)
        keep = rng.random(len(narrow[1])) < 0.5                                   # a mask: half the product's pattern and row 0 whole
        rows = np.repeat(np.arange(9), np.diff(narrow[0]))
        mkey = np.union1d(rows[keep] * NARROW + narrow[1][keep].astype(np.int64), np.arange(NARROW))
        mask = (np.concatenate([[0], np.cumsum(np.bincount(mkey // NARROW, minlength=9))]).astype(np.int64), (mkey % NARROW).astype(np.uint32))
        mask_w = (mask[0], W.relabel(mask[1], t))
        for complement in (False, True):
            got_n, s_n = mxm_masked_model.filter_product(narrow, st_n, a, b, mask, NARROW, complement)
            got_w, s_w = mxm_masked_model.filter_product(wide, st_w, a, bw, mask_w, N, complement)
            _same(got_w, W.relabel_csr(got_n, t))
            assert s_w == s_n and 0 < s_w["nnz_out"] < st_w["nnz_out"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,name", COMBOS)
def test_ewise_and_apply_mask(N, name, dt):
    _, b, c = _case(dt)
    t = W.phi(name, NARROW, N)
    bw, cw = W.relabel_csr(b, t), W.relabel_csr(c, t)
    pn, pw = ewise_model.Plan(b, c, NARROW), ewise_model.Plan(bw, cw, N)
    assert pn.nnz_both == pw.nnz_both > 0
    for mode, op in (("union", "plus"), ("union", "second"), ("intersect", "minus"), ("intersect", "div"), ("union", "min")):
        _same(pw.result(mode, op)[:3], W.relabel_csr(pn.result(mode, op)[:3], t))
    _same(ewise_model.ewise(bw, bw, N, "union", "plus"), W.relabel_csr(ewise_model.ewise(b, b, NARROW, "union", "plus"), t))
    for complement in (False, True):
        got = bfs_model.apply_mask(*bw, cw[0], cw[1], N, complement)
        want = bfs_model.apply_mask(*b, c[0], c[1], NARROW, complement)
        _same(got, W.relabel_csr(want, t))
        assert 0 < len(got[1]) < len(b[1])


def _select_loop(csr, op, threshold, diag):
    """select, entry by entry, in Python integers and floats."""
    rowptr, col, val = csr
    cmp = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b, "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b,
           "eq": lambda a, b: a == b, "ne": lambda a, b: a != b, "tril": lambda a, b: a <= b, "triu": lambda a, b: a >= b,
           "diag": lambda a, b: a == b, "offdiag": lambda a, b: a != b}[op]
    keep = np.zeros(len(col), bool)
    for r in range(len(rowptr) - 1):
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            keep[e] = cmp(float(val[e]), float(threshold)) if op in truss_model.VALUE_OPS else cmp(int(col[e]), r + int(diag))
    out = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))[keep], minlength=len(rowptr) - 1))])
    return out.astype(np.int64), col[keep], val[keep]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,name", COMBOS)
def test_select(N, name, dt):
    _, b, _ = _case(dt)
    t = W.phi(name, NARROW, N)
    bw = W.relabel_csr(b, t)
    for op in truss_model.VALUE_OPS:
        got = truss_model.select(*bw, op, 0.25)
        _same(got, W.relabel_csr(truss_model.select(*b, op, 0.25), t))
        _same(got, _select_loop(bw, op, 0.25, 0))
    kept = set()
    for op in truss_model.POSITION_OPS:
        for diag in (0, 1, -1, N - 2, -(N - 2), 1 << 33, N - 4, -(1 << 33)):
            got = truss_model.select(*bw, op, diag=diag)
            _same(got, _select_loop(bw, op, 0.0, diag))
            kept.add(len(got[1]))
    assert len(kept) > 2                                                          # the diagonals cut at different places
    # row 3 holds column N - 1 = 3 + (N - 4): the diagonal N - 4 is not empty
    assert len(truss_model.select(*bw, "diag", diag=N - 4)[1]) >= 1


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,name", COMBOS)
def test_build(N, name, dt):
    rng = np.random.default_rng(8)
    M, nnz = 7, 300
    rows, cols = rng.integers(0, M, nnz), rng.integers(0, NARROW, nnz)
    rows[-5:], cols[-5:] = M - 1, NARROW - 1                                      # repeats of the last coordinate
    rows[0], cols[0] = 0, 0
    vals = rng.standard_normal(nnz).astype(dt)
    t = W.phi(name, NARROW, N)
    wide = W.relabel(cols, t)
    for dup in ("plus", "min", "max", "first", "last", "count"):
        (got, st_w, _), (want, st_n, _) = build_model.build(M, N, rows, wide, vals, dup, dt), build_model.build(M, NARROW, rows, cols, vals, dup, dt)
        _same(got, W.relabel_csr(want, t))
        assert got[1][-1] == N - 1 and got[1][0] == t[0]
        assert {k: v for k, v in st_w.items() if k != "launches"} == {k: v for k, v in st_n.items() if k != "launches"}
        assert st_w["launches"] > st_n["launches"]                                # more sort passes over the wider key
    with pytest.raises(build_model.BuildError) as ei:
        build_model.build(M, N, rows, wide, vals, "error", dt)
    assert ei.value.status == build_model.ERR_DUPLICATE
    with pytest.raises(build_model.BuildError) as ei:
        build_model.build(M, N, [0], [N], [1.0], "plus", dt)
    assert ei.value.status == build_model.ERR_RANGE


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,name", COMBOS)
def test_extract_by_rows_reduce_over_rows_and_inflate_prune(N, name, dt):
    _, b, _ = _case(dt)
    t = W.phi(name, NARROW, N)
    bw = W.relabel_csr(b, t)
    rows = [12, 0, 3, 3, 6, 12]
    got, st_w = extract_model.extract(*bw, N, rows=rows)
    want, st_n = extract_model.extract(*b, NARROW, rows=rows)
    _same(got, W.relabel_csr(want, t))
    assert st_w == st_n
    for op in vector_model.REDUCE_OPS:
        gw, gn = vector_model.reduce(*bw, N, "rows", op), vector_model.reduce(*b, NARROW, "rows", op)
        nan = np.isnan(gn[0])
        assert np.array_equal(nan, np.isnan(gw[0])) and np.array_equal(_bits(gw[0][~nan]), _bits(gn[0][~nan])) and gw[1] == gn[1]
    rng = np.random.default_rng(2)
    p = (b[0], b[1], (rng.random(len(b[1])) * 0.95 + 0.05).astype(dt))
    p[2][b[0][3]:b[0][3] + 6] = dt(0.5)                                           # ties: the lower column wins, whatever its label
    pw = W.relabel_csr(p, t)
    for cap in (0, 4):
        got, want = mcl_model.inflate_prune(*pw, 2.0, 0.3, cap), mcl_model.inflate_prune(*p, 2.0, 0.3, cap)
        _same(got[:3], W.relabel_csr(want[:3], t))
        assert got[3] == want[3]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,name", COMBOS)
def test_the_forms_that_read_no_length_N_operand(N, name, dt):
    """mxv, mxv_arg with mul = "first" and x = None: the models index no vector, and the positions are unsigned columns."""
    _, b, _ = _case(dt)
    t = W.phi(name, NARROW, N)
    bw = W.relabel_csr(b, t)
    for add in ("min", "max"):
        y_w, arg_w, _, without_w = mxv_arg_model.mxv_arg(*bw, None, add, "first")
        y_n, arg_n, _, without_n = mxv_arg_model.mxv_arg(*b, None, add, "first")
        assert arg_w.dtype == np.int64 and without_w == without_n
        assert np.array_equal(arg_w, np.where(arg_n < 0, -1, t.astype(np.int64)[np.maximum(arg_n, 0)]))
        assert arg_w.max() >= 0 and arg_w.min() >= -1                             # never a sign-extended column
        nan = np.isnan(y_n)
        assert np.array_equal(_bits(y_w[~nan]), _bits(y_n[~nan]))
    assert np.array_equal(_bits(mxv_model.mxv(*bw, None, "plus", "first")[0]), _bits(mxv_model.mxv(*b, None, "plus", "first")[0]))


def test_permute_by_its_definition_is_the_composed_extract():
    """tests/test_gpu_wide_columns.py judges ``permute`` at 2^25 + 1 by out[i, k] = in[perm[i], perm[k]] written out; here that
    is held to extract_model.extract_any, the model of the composed path, on a small square case."""
    rng = np.random.default_rng(21)
    n = 37
    csr = _random_csr(rng, n, n, np.float32, 0.2, full_row=5)
    rows = np.repeat(np.arange(n), np.diff(csr[0]))
    for perm in (rng.permutation(n), np.arange(n), np.arange(n)[::-1].copy()):
        want = extract_model.extract_any(*csr, n, rows=perm, cols=perm)
        _same(W.permuted((rows, csr[1].astype(np.int64), csr[2]), perm, n), want)
