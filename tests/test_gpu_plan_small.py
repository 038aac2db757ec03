"""The one-wave planner of small direct rows (osp_split.h, direct_plan_small_kernel).

A long row of at most 64 chunks whose (chunk, range) cells fit the small planner's LDS is planned by one wave instead of
a workgroup of four; the plan must be word for word the four-wave planner's.  Every case here is one product of a few
thousand to a few tens of thousands of partial products, built by hand so that output rows sit at the small planner's
edges, and computed three ways: with the small planner (the default), with OSP_PLAN_SMALL=0 (every row to
direct_plan_kernel), and by the CPU oracle.  rowptr, colidx and vals must be bit-identical across the three, the
counters that describe the plan equal between the two settings, and the number of rows the small planner took -- the
OSP_VERBOSE line of plan_panel -- what the eligibility rule of split_params_kernel predicts.

Operands: N = 2^18 columns.  (With N near 4096 every long row is a "capped" row -- its bins are as narrow as the dense
accumulators -- and capped rows are not eligible.)

The walk branch of the (chunk, range) counts -- chunks shorter than 8 entries per range boundary -- cannot occur in a
small row (at most 64 chunks; the proof is at the kernel): the case below puts such a row beside a row of long chunks
and checks that the short-chunk row stays with the four-wave planner.
"""
import re

import numpy as np
import pytest

from tests.test_gpu_parity import assert_same, run_both

pytestmark = pytest.mark.gpu

N = 1 << 18
COLBITS = 18
TILE_CAP = {np.dtype(np.float64): 1536, np.dtype(np.float32): 1792}   # TileCap<T>
SMALL_CHUNKS, SMALL_CELLS, SMALL_BITS = 64, 512, 8                    # kSmallChunks, kSmallCells, kSmallFineBits
PLAN_COUNTERS = ("panels", "light_tiles", "heavy_rows", "heavy_partials", "direct_rows", "direct_partials", "gathered_rows",
                 "gathered_partials", "gathered_runs", "gathered_short_partials", "sorted_segments", "sorted_partials",
                 "dense_segments", "merge_launches", "direct_plan_launches", "nnz_c", "partials")


def eligible(U, nc, cap):
    """split_params_kernel's rule for a row of U partial products in nc chunks (N = 2^18, default limits)."""
    if U <= cap:
        return False                                        # a short row: no plan
    want = -(-U // 256)
    b = 1
    while b < 12 and (1 << b) < want:
        b += 1
    b = min(b, COLBITS, COLBITS - 11)
    if (1 << b) < want:
        return False                                        # capped
    nranges = min(2 * U // cap + 2, (1 << b) + 1)
    hbits = min(b + 2, COLBITS, 9)
    return hbits <= SMALL_BITS and 1 <= nc <= SMALL_CHUNKS and nc * nranges <= SMALL_CELLS


class Operands:
    """B rows are appended as needed; a row of A is the list of B rows it multiplies."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b_cols, self.a_rows = [], []

    def b_row(self, length, cols=None):
        if cols is None:
            cols = np.sort(self.rng.choice(N, length, replace=False))
        self.b_cols.append(np.asarray(cols, np.uint32))
        return len(self.b_cols) - 1

    def a_row(self, lengths):
        """An output row whose chunks have these lengths, in ascending k.  Returns (U, nc)."""
        ks = [self.b_row(n) for n in lengths]
        self.a_rows.append(ks)
        return sum(lengths), len(lengths)

    def coo(self):
        K = len(self.b_cols)
        b_rows = np.concatenate([np.full(len(c), k, np.uint32) for k, c in enumerate(self.b_cols)])
        b_cols = np.concatenate(self.b_cols)
        a_rows = np.concatenate([np.full(len(ks), i, np.uint32) for i, ks in enumerate(self.a_rows)])
        a_cols = np.concatenate([np.asarray(ks, np.uint32) for ks in self.a_rows])
        a = (a_rows, a_cols, self.rng.uniform(0.5, 1.5, len(a_rows)))
        b = (b_rows, b_cols, self.rng.uniform(0.5, 1.5, len(b_rows)))
        return len(self.a_rows), K, a, b


def small_rows(err):
    """Rows the small planner took, summed over the panels, from the OSP_VERBOSE lines of one product."""
    found = re.findall(r"small planner: (\d+) of (\d+) direct rows", err)
    assert found, err
    return sum(int(a) for a, _ in found), sum(int(t) for _, t in found)


def three_ways(ctx, port, monkeypatch, capfd, ops, dt, want_small, want_direct):
    ctx.algorithm = "outer"
    M, K, a, b = ops.coo()
    monkeypatch.setenv("OSP_VERBOSE", "1")
    monkeypatch.delenv("OSP_PLAN_SMALL", raising=False)
    capfd.readouterr()
    on, want = run_both(ctx, port, M, K, N, a, b, dt)
    n_on, d_on = small_rows(capfd.readouterr().err)
    monkeypatch.setenv("OSP_PLAN_SMALL", "0")
    off, _ = run_both(ctx, port, M, K, N, a, b, dt)
    n_off, d_off = small_rows(capfd.readouterr().err)
    print(f"small planner: {n_on} of {d_on} direct rows (OSP_PLAN_SMALL=0: {n_off} of {d_off})")
    assert_same(on, want)
    assert_same(off, want)
    for name in ("rowptr", "colidx", "vals"):
        assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), name
    assert {k: on.info[k] for k in PLAN_COUNTERS} == {k: off.info[k] for k in PLAN_COUNTERS}
    assert on.info["gathered_rows"] == on.info["direct_rows"] == want_direct, on.info
    assert n_off == 0 and d_on == d_off == want_direct
    assert n_on == want_small, (n_on, want_small)          # a case meant for the small planner must reach it
    on.close()
    off.close()


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
def test_smallest_long_row(_ctx_shared, port, monkeypatch, capfd, dt):
    """U = TileCap + 1: two ranges."""
    cap = TILE_CAP[np.dtype(dt)]
    ops = Operands(1)
    ops.a_row([100])                                        # a short row before it
    U, nc = ops.a_row([64] * (cap // 64) + [1])
    assert U == cap + 1 and eligible(U, nc, cap)
    ops.a_row([7, 9])
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, 1)


def _limit_rows(cap):
    """(name, chunk lengths, eligible): the last eligible row and the first that is not, at every limit."""
    per32, per33 = (340, 330) if cap == 1536 else (400, 390)   # 16 segments either way: 2 U / cap = 14
    return [("64 chunks", [32] * 64, True), ("65 chunks", [32] * 65, False),
            ("512 cells", [per32] * 32, True), ("528 cells", [per33] * 33, False),
            ("256 bins", [1024] * 16, True), ("512 bins", [1024] * 16 + [1], False)]


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("dt", DTYPES)
def test_eligibility_limits(_ctx_shared, port, monkeypatch, capfd, dt, which):
    cap = TILE_CAP[np.dtype(dt)]
    name, lengths, want = _limit_rows(cap)[which]
    ops = Operands(10 + which)
    U, nc = ops.a_row(lengths)
    assert eligible(U, nc, cap) == want, (name, U, nc)
    if name.endswith("cells"):
        assert 2 * U // cap + 2 == 16 and nc * 16 == int(name.split()[0])
    ops.a_row([5])
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, int(want), 1)


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_tiny_and_dominant_chunks(_ctx_shared, port, monkeypatch, capfd, dt):
    """Empty B rows, chunks of one entry, and one chunk longer than all the others together."""
    cap = TILE_CAP[np.dtype(dt)]
    ops = Operands(3)
    for lengths in ([0, 1, 1, 0, 2400, 1, 50, 0, 0, 50, 1, 1, 1, 50, 1, 0], [1, 0, 1] * 5 + [cap] + [0, 1]):
        U, nc = ops.a_row(lengths)
        assert eligible(U, nc, cap), (U, nc)
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 2, 2)


@pytest.mark.parametrize("dt", DTYPES)
def test_long_and_short_chunks(_ctx_shared, port, monkeypatch, capfd, dt):
    """Chunks far longer than 8 entries per range boundary (lower bounds: the small planner's only branch) beside a row
    of chunks shorter than that, which has more than 64 chunks by necessity and walks in the four-wave planner."""
    cap = TILE_CAP[np.dtype(dt)]
    ops = Operands(4)
    U, nc = ops.a_row([177] * 28)
    assert eligible(U, nc, cap)
    U, nc = ops.a_row([7] * 300)
    assert U > cap and not eligible(U, nc, cap)
    U, nc = ops.a_row([9] * 60 + [cap])                     # short chunks and a long one: 61 chunks, lower bounds
    assert eligible(U, nc, cap)
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 2, 3)


@pytest.mark.parametrize("dt", DTYPES)
def test_over_long_range(_ctx_shared, port, monkeypatch, capfd, dt):
    """64 chunks that each hold the same 30 consecutive columns: one fine bin above the tile capacity."""
    cap = TILE_CAP[np.dtype(dt)]
    ops = Operands(5)
    cols = 3 * 8192 + 100 + np.arange(30)
    ops.a_rows.append([ops.b_row(30, cols) for _ in range(64)])
    assert eligible(64 * 30, 64, cap)
    ops.a_row([11, 3])
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, 1)


@pytest.mark.parametrize("dt", DTYPES)
def test_interleaved_rows(_ctx_shared, port, monkeypatch, capfd, dt):
    """Eligible and non-eligible long rows and short rows interleaved in one panel."""
    cap = TILE_CAP[np.dtype(dt)]
    ops = Operands(6)
    rng = np.random.default_rng(66)
    small = direct = 0
    for r in range(36):
        kind = r % 4
        if kind == 0:      # a few ranges, a dozen or two chunks
            lengths = rng.integers(40, 400, rng.integers(8, 30)).tolist()
        elif kind == 1:    # too many chunks
            lengths = rng.integers(10, 60, rng.integers(70, 120)).tolist()
        elif kind == 2:    # a short row
            lengths = rng.integers(1, 40, rng.integers(1, 9)).tolist()
        else:              # long chunks: few chunks, many ranges, some beyond the cells or the bins
            lengths = rng.integers(300, 1500, rng.integers(4, 34)).tolist()
        U, nc = ops.a_row(lengths)
        direct += U > cap
        small += eligible(U, nc, cap)
    assert 8 <= small < direct - 8, (small, direct)
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, small, direct)
