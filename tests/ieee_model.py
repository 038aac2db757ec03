"""IEEE edge values through the product: a bit comparator, a builder of prescribed sums ("piles") and their plain model.

The bar says the values of every path equal the oracle's BIT FOR BIT.  `np.array_equal` does not check that: it
calls -0.0 and +0.0 equal and can never pass on a NaN.  `assert_same_bits` compares every value as an unsigned integer of
its width; NaNs are compared by position only (x86 yields 0xfff8... for inf - inf where the GPU yields 0x7ff8...).

A pile is the SEQUENCE of products one output entry collects, in ascending k -- the order the merge sums them in, and the
oracle's stable sort too.  `pile_product` builds operands whose output entries collect exactly the prescribed sequences and
returns the value a plain left-to-right chain gives each: the sum STARTS as the first product, then s = T(s + T(a * b)).
`sequences` lists the piles whose result depends on a zero's sign, on gradual underflow, on where a chain overflows, and on
which operands are not finite.  Everything is generated from np.finfo and seeds.
"""
from collections import namedtuple

import numpy as np

LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 80, 81, 300)   # around kRunShort = 16 and the wave-summed chunks of 64 behind it
EVENTS = (0, 1, 15, 16, 17, 79, 80, 81)                 # ... and L - 1: where in a pile the special value sits

# terms: a list of (a, b) factor pairs in ascending k; nan: the pile is DESIGNED to end as a NaN
Pile = namedtuple("Pile", "name terms nan row")
Pile.__new__.__defaults__ = (False, 0)


def _uint(dtype):
    return {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def assert_same_bits(got_vals, want_vals):
    """Same dtype and length, NaNs at the same positions, every other value equal as an unsigned integer of its width."""
    got, want = np.ascontiguousarray(got_vals), np.ascontiguousarray(want_vals)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.dtype in (np.float32, np.float64), got.dtype
    assert got.shape == want.shape and got.ndim == 1, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"NaN positions differ at {np.flatnonzero(gn != wn)[:8].tolist()}"
    u = _uint(got.dtype)
    gb, wb = got.view(u), want.view(u)
    bad = np.flatnonzero((gb != wb) & ~gn)
    assert bad.size == 0, (f"{bad.size} values differ in their bits, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()} "
                           f"({[hex(int(x)) for x in gb[bad[:8]]]}), want {want[bad[:8]].tolist()} ({[hex(int(x)) for x in wb[bad[:8]]]})")


def chain(dtype, terms):
    """The model: the sum starts AS the first product, then s = T(s + T(a * b)) left to right, all in T."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        s = None
        for a, b in terms:
            p = T(T(a) * T(b))
            s = p if s is None else T(s + p)
    return s


def events(L):
    """Positions of the special value in a pile of L terms."""
    return sorted({e for e in EVENTS + (L - 1,) if 0 <= e < L})


def sequences(dtype, L, where=None, seed=0, only=None):
    """The piles of length L (the table of the issue): every sequence (or those whose id is in `only`), those with an event
    once per position in `where` (default: events(L)).  Piles whose NaN comes from the A side sit in output row 1 (in a shared row A's NaN at k would
    reach every column that has a term at k; a row of their own keeps row 0's design readable)."""
    T = np.dtype(dtype).type
    f = np.finfo(dtype)
    tiny, sub, mx = T(f.tiny), T(f.smallest_subnormal), T(f.max)
    h = T(mx / T(4))
    inf, nan, nz, one = T(np.inf), T(np.nan), T(-0.0), T(1)
    plain = lambda bs: [(one, T(b)) for b in bs]   # noqa: E731
    out = []

    def add(name, terms, nan_=False, row=0):
        if only is not None and name.split("/")[0] not in only:
            return
        assert len(terms) == L, (name, len(terms), L)
        out.append(Pile(f"{name}/L{L}", terms, nan_, row))

    # zeros: the sign survives only a sum that starts as its first entry
    add("z1", plain([nz] * L))
    add("z2", plain([nz] + [T(0.0)] * (L - 1)))
    add("z3a", [(nz, T(3))] + plain([nz] * (L - 1)))            # the product's sign rule, A side ...
    add("z3b", [(T(3), nz)] + plain([nz] * (L - 1)))            # ... and B side
    if L >= 2:                                                  # exact cancellation: +0.0, kept as an entry
        rng = np.random.default_rng(seed + 11)
        bs = []
        while len(bs) + 3 < L or len(bs) + 2 == L:
            x = T(rng.integers(1, 1 << 20)) / T(64)
            bs += [x, -x]
        if len(bs) < L:
            x, y = T(rng.integers(1, 1 << 10)) / T(8), T(rng.integers(1, 1 << 10)) / T(4)
            bs += [x, y, -(x + y)]
        add("z4", plain(bs))
    # gradual underflow of the PRODUCT, then sums of subnormals
    add("u1a", [(T(0.5), tiny)] + plain([nz] * (L - 1)))        # a subnormal
    add("u1b", [(tiny, tiny)] + plain([nz] * (L - 1)))          # +0.0
    add("u1c", [(-tiny, tiny)] + plain([nz] * (L - 1)))         # -0.0
    add("u2a", plain([T(3) * sub] * L))                         # exact; flushed if the adds flush
    add("u2b", plain([T(tiny * T(0.75)) + T(3) * sub] * L))     # crosses from subnormal into normal at the second term
    # overflow: WHERE in the chain
    add("o2", plain([h] * min(L, 5) + [-h] * max(L - 5, 0)))    # +inf at the fifth term; in any other order finite
    add("o3", plain([-h] * min(L, 5) + [h] * max(L - 5, 0)))
    # order-sensitive absorption: magnitudes 2^+-(emax - 2), random mantissas and signs; a big term opposes a big sum
    rng = np.random.default_rng(seed + 13)
    big, small = T(2.0) ** T(f.maxexp - 2), T(2.0) ** T(-(f.maxexp - 2))
    bs, s = [], T(0)
    with np.errstate(all="ignore"):
        for i in range(L):
            m = T(1 + rng.random())
            sign = T(-1 if rng.random() < 0.5 else 1)
            if rng.random() < 0.5:
                if abs(s) >= big:
                    sign = T(-np.sign(s))
                bs.append(sign * m * big)
            else:
                bs.append(sign * m * small)
            s = T(s + bs[-1])
    assert np.isfinite(s)
    add("m1", plain(bs))
    # special values at position e
    for e in (events(L) if where is None else [e for e in where if 0 <= e < L]):
        def at(term, rest=one):
            return [term if i == e else (one, rest) for i in range(L)]
        add(f"o1/e{e}", at((mx, T(2))))                         # +inf from one product
        if L >= 2:                                              # +inf at e and -inf later (before, for e = L - 1): NaN
            t = at((one, inf))
            t[(e + L) // 2 if (e + L) // 2 > e else ((L - 1) // 2 if e == L - 1 else e + 1)] = (one, -inf)
            add(f"n1/e{e}", t, True)
        add(f"n2a/e{e}", at((T(0), inf)), True)                 # 0 * inf, both factor orders
        add(f"n2b/e{e}", at((inf, T(0))), True)
        add(f"n3/e{e}", at((one, nan)), True)                   # a NaN value in B
        add(f"n3A/e{e}", at((nan, one)), True, 1)               # ... and in A: a row of its own
        add(f"n4/e{e}", at((one, inf)))                         # +inf, finite elsewhere: +inf
    return out


def nan_count(L):
    """How many piles of sequences(dtype, L) are designed NaN: per event n2a, n2b, n3, n3A, and n1 where L >= 2."""
    return len(events(L)) * (4 + (L >= 2))


def pile_product(dtype, piles, a_vals=None, row_cap=None):
    """Operands of a product whose output entries collect exactly the piles' sequences of products, in ascending k.

    Each output row has k slots of its own; row r of A is dense over them.  The t-th terms of a row's piles share one
    slot per value of a: A's values are 1 but where a pile asks for a factor on the A side (a slot of its own beside the
    t-th plain one), and row k of B holds the columns whose pile has a term at k.  a_vals: A's value of the t-th plain
    slot (default: ones) -- the model takes it as the term's factor.  row_cap:
    open a further output row when the next pile would bring a row's products above it (piles keep their relative
    `row` order; default: the rows the piles name).

    Returns dict(M, K, N, a, b: COO triples, row, col: each pile's output entry, want: the model's values in CSR order,
    nan: the designed NaN flags in CSR order, names in CSR order, row_products: products per output row, first_k: the
    first k slot of (output row, term index t))."""
    T = np.dtype(dtype).type
    u = _uint(dtype)
    bits = lambda x: int(np.asarray(T(x)).view(u))   # noqa: E731
    # output rows: as the piles name them, or opened as the products of a row reach row_cap
    if row_cap is None:
        rows = [p.row for p in piles]
    else:
        rows, cur, used = [], {}, []
        for p in piles:
            r = cur.get(p.row)
            if r is None or used[r] + len(p.terms) > row_cap:
                r = cur[p.row] = len(used)
                used.append(0)
            used[r] += len(p.terms)
            rows.append(r)
    M = max(rows) + 1
    # k slots of output row r: per term index t one slot whose A value is 1 (a_vals[t]) and one per other value asked at t
    groups = [{} for _ in range(M)]                  # t -> {bits of A's value: None}, in order of appearance
    ncol = [0] * M
    cols, want, entries = [], [], []                 # entries: (row, t, bits of a, col, b)
    for p, r in zip(piles, rows):
        cols.append(ncol[r])
        ncol[r] += 1
        terms = []
        for t, (a, b) in enumerate(p.terms):
            if bits(a) == bits(1) and a_vals is not None:
                a = a_vals[t % len(a_vals)]
            groups[r].setdefault(t, {})[bits(a)] = None
            entries.append((r, t, bits(a), cols[-1], T(b)))
            terms.append((T(a), b))
        want.append(chain(dtype, terms))
    slot, a_bits, a_row, first_k = {}, [], [], {}
    for r in range(M):
        for t in sorted(groups[r]):
            first_k[(r, t)] = len(a_bits)
            for ab in groups[r][t]:
                slot[(r, t, ab)] = len(a_bits)
                a_bits.append(ab)
                a_row.append(r)
    K, N = len(a_bits), max(ncol)
    a_rows, a_cols, a_v = np.array(a_row, np.uint32), np.arange(K, dtype=np.uint32), np.array(a_bits, u).view(T)
    e = np.array([(slot[(r, t, ab)], c) for r, t, ab, c, _ in entries], np.int64).reshape(-1, 2)
    b_v = np.array([b for *_, b in entries], T)
    order = np.lexsort((e[:, 1], e[:, 0]))
    b = (e[order, 0].astype(np.uint32), e[order, 1].astype(np.uint32), b_v[order])
    csr = np.lexsort((cols, rows))
    return dict(M=M, K=K, N=N, a=(a_rows, a_cols, a_v), b=b, row=np.array(rows)[csr], col=np.array(cols)[csr],
                want=np.array(want, T)[csr], nan=np.array([p.nan for p in piles])[csr], names=[piles[i].name for i in csr],
                first_k=first_k, row_products=np.bincount(np.array(rows), weights=[len(p.terms) for p in piles], minlength=M).astype(np.int64))
