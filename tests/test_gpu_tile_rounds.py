"""Merge tiles of every round count (osp_kernels.h, OSP_TILE_ROUNDS).

The tile kernel runs a tile of n entries through a body of Q >= ceil(n / 256) rounds; a gathered tile gives each wave a
span of 64 * Q positions and every thread a block of Q sorted entries.  These products make tiles of every
ceil(n / 256) from 1 to the capacity's (6 for f64, 7 for f32): as short-row tiles of an exact size (a row of n partial
products followed by a row that fills a tile by itself, so the first is alone in its tile), as the ranges and tail
ranges of long rows, and -- in the formulations that write their rows -- as staged tiles.  Every formulation must give
the oracle's bits.
"""
import os

import numpy as np
import pytest

from tests.test_gpu_parity import assert_same, run_both

pytestmark = pytest.mark.gpu

THREADS = 256                                                        # kMergeThreads
TILE_CAP = {np.dtype(np.float64): 1536, np.dtype(np.float32): 1792}  # TileCap<T>
RUN_SHORT = 16                                                       # kRunShort

# B's rows by family: (first row, rows, entries per row, column window)
N = 1 << 18
WIDE, ONE, BAND, HUB = (0, 3000, 16, N), (3000, 64, 1, N), (3064, 400, 16, 512), (3464, 64, 16, N)
K = 3528


def _operand_b(rng):
    rows, cols = [], []
    for first, count, per, window in (WIDE, ONE, BAND, HUB):
        for k in range(first, first + count):
            c = np.sort(rng.choice(window - 1, per, replace=False)) + 1
            if first == HUB[0]:
                c[0] = 0                                             # every row of the family hits column 0: one long run
            rows.append(np.full(per, k, np.uint32))
            cols.append(c.astype(np.uint32))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return rows, cols, rng.uniform(0.5, 1.5, len(rows))


def _pick(rng, family, count):
    first, rows, _, _ = family
    return np.sort(rng.choice(np.arange(first, first + rows), count, replace=False))


def _row_of(rng, n, family=WIDE):
    """B rows (= columns of A) whose chunks hold n partial products together."""
    per = family[2]
    ks = [_pick(rng, family, n // per)] if n >= per else []
    if n % per:
        ks.append(_pick(rng, ONE, n % per))
    return np.sort(np.concatenate(ks))


def _operand_a(rng, cap):
    """Rows of A as lists of k; returns (rows, their partial-product counts, sizes of the tiles made on purpose)."""
    lpt = cap // THREADS
    a_rows, tiles = [], []
    full = lambda: _row_of(rng, cap)                                 # a row that fills a tile: closes the one before it

    def alone(ks_list):                                              # these rows share one tile, nothing else is in it
        a_rows.extend(ks_list)
        a_rows.append(full())

    # one entry; the edges 256 Q and 256 Q + 1 (and 256 Q - 1) of every round count
    sizes = [1, 2, 63, 64, 65]
    for q in range(1, lpt + 1):
        sizes += [s for s in (THREADS * q - 1, THREADS * q, THREADS * q + 1) if s <= cap]
    sizes += [cap - 1]
    for n in sizes:
        alone([_row_of(rng, n)])
        tiles.append(n)
    # several rows per tile (row bits in the key), of every round count
    for q in range(1, lpt + 1):
        nrows = 3 * q
        per_row = (THREADS * q - 40) // nrows
        alone([_row_of(rng, per_row) for _ in range(nrows)])
        tiles.append(nrows * per_row)
    # many duplicates: runs that cross the blocks of Q sorted entries, in small and in full tiles
    for n in (192, 320, 704, 1120, cap - 16):
        alone([_row_of(rng, n, BAND)])
        tiles.append(n)
    # a run longer than kRunShort in a small tile (it starts the sorted tile and spans many threads' blocks), alone and
    # with a second row behind it
    hub = _pick(rng, HUB, RUN_SHORT + 9)
    alone([hub])
    tiles.append(16 * len(hub))
    alone([_pick(rng, HUB, RUN_SHORT + 1), _row_of(rng, 100, BAND)])
    tiles.append(16 * (RUN_SHORT + 1) + 100)
    # long rows: column ranges of about a tile and a tail each, the tails of every size; the shortest long row too
    for n in [cap + 1, cap + THREADS, 2 * cap] + [int(x) for x in rng.integers(cap + 1, 14 * cap, 160)]:
        a_rows.append(_row_of(rng, n))
    a_rows.append(full())
    rows = np.concatenate([np.full(len(ks), i, np.uint32) for i, ks in enumerate(a_rows)])
    cols = np.concatenate(a_rows).astype(np.uint32)
    return len(a_rows), rows, cols, rng.uniform(0.5, 1.5, len(rows)), tiles


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_tiles_of_every_round_count(ctx, port, dt):
    cap = TILE_CAP[np.dtype(dt)]
    lpt = cap // THREADS
    rng = np.random.default_rng(2406)
    b = _operand_b(rng)
    M, a_rows, a_cols, a_vals, tiles = _operand_a(rng, cap)
    # the tiles made on purpose cover every round count, the edges included
    need = {max(1, -(-n // THREADS)) for n in tiles}
    assert need == set(range(1, lpt + 1)), need
    assert {1, THREADS, THREADS + 1, THREADS * lpt} <= set(tiles)
    got, want = run_both(ctx, port, M, K, N, (a_rows, a_cols, a_vals), b, dt)
    assert_same(got, want)
    i = got.info
    gathers = ctx.algorithm == "outer" and os.environ.get("OSP_GATHER") != "0" and os.environ.get("OSP_DIRECT") != "0"
    if gathers:   # long rows and short rows were formed inside the tile kernel
        assert i["gathered_rows"] > 100 and i["gathered_partials"] > 100 * cap, i
        assert i["gathered_short_partials"] >= sum(tiles), i
    else:         # ... or written by the multiply (or formed row-wise): staged tiles
        assert i["gathered_short_partials"] == 0, i
    got.close()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_uniform_fill_of_every_round_count(ctx, port, dt):
    """Whole products of tiles of ONE size, so that every workgroup meets the same round count tile after tile (the next
    tile's request is placed for the rounds of ITS body while the current one is still being written)."""
    cap = TILE_CAP[np.dtype(dt)]
    rng = np.random.default_rng(77)
    b = _operand_b(rng)
    for q in range(1, cap // THREADS + 1):
        n = THREADS * q - 16 * int(rng.integers(0, 8))              # a few entries short of the round's last slot
        ks = [_row_of(rng, n, BAND if q % 2 else WIDE) if r % 2 == 0 else _row_of(rng, cap) for r in range(60)]
        rows = np.concatenate([np.full(len(k), r, np.uint32) for r, k in enumerate(ks)])
        a = (rows, np.concatenate(ks).astype(np.uint32), rng.uniform(0.5, 1.5, len(rows)))
        got, want = run_both(ctx, port, len(ks), K, N, a, b, dt)
        assert_same(got, want)
        got.close()
