"""Wide column spaces for the tests (a helper module, not a test file): the widths at which the code that forks on
``colbits = bits_for(N)`` takes its wide side, and three strictly increasing relabelings of the columns [0, n) of a narrow case
into [0, N).  Every operation of the library sees a column only through comparisons with other columns of the same space (and,
for the positional predicates of ``select``, with the row), so a strictly increasing relabeling of an operand's columns
relabels the result's columns the same way and leaves every value bit alone: ``model(phi(case)) == phi(model(case))``.
tests/test_wide_columns_cpu.py checks that for every model tests/test_gpu_wide_columns.py relies on."""
import numpy as np

# 2^24:      24 column bits + 8 row bits: the first 32-bit key of a merge tile
# 2^28 + 5:  29 column bits: tiles of at most 8 rows
# 2^31:      colbits 31: tiles of 2 rows, and an all-ones key exists (local row 1, column N - 1)
# 2^31 + 1:  colbits 32: the first N whose largest column has bit 31 set; tiles of 1 row
# 2^32 - 1:  the largest legal N: its largest column, 0xfffffffe, is next to every 0xffffffff sentinel
WIDTHS = [1 << 24, (1 << 28) + 5, 1 << 31, (1 << 31) + 1, (1 << 32) - 1]
# the most rows a merge tile may hold at each width: min(255, 2^(32 - colbits)), 1 at colbits 32
TILE_ROWS = {1 << 24: 255, (1 << 28) + 5: 8, 1 << 31: 2, (1 << 31) + 1: 1, (1 << 32) - 1: 1}
# the one width at which the operations with an O(N) footprint run: the first colbits (26) beyond anything they are tested at
LINEAR_WIDTH = (1 << 25) + 1
MAPS = ["top", "spread", "straddle"]


def bits_for(n):
    """The library's bits_for: the smallest b with n <= 2^b."""
    b = 0
    while n > (1 << b):
        b += 1
    return b


def _checked(out, n, N):
    assert out.dtype == np.uint32 and out.shape == (n,)
    assert n == 0 or int(out[-1]) < N
    assert np.all(out[1:] > out[:-1]), "a relabeling must be strictly increasing"
    return out


def phi(name, n, N):
    """The table of the relabeling ``name`` of [0, n) into [0, N): a uint32 array t of n strictly increasing columns below N.

    ``top``: c + (N - n) -- clustering is kept, every column sits at the top of the space, column n - 1 becomes N - 1.
    ``spread``: c * (N // n), the last column sent to N - 1 -- clustering is destroyed.
    ``straddle``: the lower half of the columns stays, the upper half is shifted to end at N - 1 -- at N > 2^31 a row holds
    columns on both sides of bit 31, and both column 0 and column N - 1 occur."""
    n, N = int(n), int(N)
    assert 0 < n <= N <= 0xffffffff
    c = np.arange(n, dtype=np.int64)
    if name == "top":
        t = c + (N - n)
    elif name == "spread":
        t = c * (N // n)
        t[-1] = N - 1
    elif name == "straddle":
        t = np.where(c < n // 2, c, c + (N - n))
    else:
        raise ValueError(name)
    return _checked(t.astype(np.uint32), n, N)


def relabel(col, table):
    """The columns ``col`` (below len(table)) under the relabeling: uint32."""
    return table[np.asarray(col).astype(np.int64)]


def relabel_csr(csr, table):
    """(rowptr, col, val) with the columns relabeled; rowptr and val are the same arrays."""
    rowptr, col, val = csr
    return rowptr, relabel(col, table), val


def table_through(n, N, must, seed=0):
    """A strictly increasing table of n columns of [0, N) that holds every column of ``must`` and random ones beside them."""
    must = np.unique(np.asarray(must, np.int64))
    assert len(must) <= n and must.max() < N
    rng = np.random.default_rng(seed)
    t = must
    while len(t) < n:
        t = np.unique(np.concatenate([t, rng.integers(0, N, n - len(t))]))
    return _checked(t.astype(np.uint32), n, N)


def permuted(entries, perm, n):
    """``permute`` by its definition, out[i, k] = in[perm[i], perm[k]]: the entry (r, c, v) of in sits at (inv[r], inv[c]) of
    out.  entries = (rows, cols, vals) with distinct coordinates.  Returns (rowptr, col, val); tests/test_wide_columns_cpu.py
    holds it to extract_model.extract_any(rows=perm, cols=perm)."""
    rows, cols, vals = entries
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n, dtype=np.int64)
    r, c = inv[rows], inv[cols]
    order = np.lexsort((c, r))
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr, c[order].astype(np.uint32), np.asarray(vals)[order]
