"""IEEE edge values through every summation path of the product, bit for bit against the oracle.

Every other multiplying test feeds the product tame values; the piles of tests/ieee_model.py (zeros of both signs, products
that underflow gradually or overflow, sums whose result depends on WHERE the chain overflows, infinities, NaNs) go through
the paths here: short rows in tiles of every round class (thread-summed and wave-summed runs), planned long rows (four-wave
and one-wave planner), over-long segments by dense accumulation (atomic and ballot), by the big in-place tile and by the
global sort, both split kernels and the split from B, the row expansion, hub rows, sums across k shards, panels and ranks,
and the bias / ReLU epilogue.  tests/test_ieee_edges_cpu.py pins the oracle to the plain model first, NaN count included;
here each product is compared with the oracle by bits (NaNs by position), each test asserts through `info` that the path
it names was taken, and the piles' entries of the oracle are checked against the model once more where the operands carry
filler beside them.
"""
import functools
import os

import numpy as np
import pytest

from tests import ieee_model as im
from tests.test_gpu_parity import assert_same
from tests.test_gpu_plan_small import eligible
from tests.test_gpu_split_from_b import FORCE, stretch_lines
from tests.test_gpu_tile_rounds import TILE_CAP

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


class Product:
    """Operands (COO), their CSC / CSR forms and -- computed once, shared, never changed -- the oracle's result."""

    def __init__(self, dt, M, K, N, a, b, **notes):
        from outerspace_amd import spgemm as S
        self.dt, self.M, self.K, self.N, self.notes = dt, M, K, N, notes
        self.acsc, self.bcsr = S.coo_to_csc(K, a[0], a[1], a[2].astype(dt)), S.coo_to_csr(K, b[0], b[1], b[2].astype(dt))
        self._want = {}

    def want(self, port, k_range=None):
        if k_range not in self._want:
            w = port.spgemm(self.M, self.K, self.N, *self.acsc, *self.bcsr, *(k_range or ()))
            for x in ("rowptr", "colidx", "vals"):
                w[x].setflags(write=False)
            self._want[k_range] = w
        return self._want[k_range]

    def run(self, ctx, **kw):
        return ctx.spgemm_csc_csr(self.M, self.K, self.N, *self.acsc, *self.bcsr, **kw)

    def check_piles(self, port, pp, rows, cols):
        """The oracle's entries at the piles' places are the model's values (the filler beside them changes nothing)."""
        w = self.want(port)
        at = np.array([w["rowptr"][r] + np.searchsorted(w["colidx"][w["rowptr"][r]:w["rowptr"][r + 1]], c) for r, c in zip(rows, cols)])
        assert np.array_equal(w["colidx"][at], cols)
        im.assert_same_bits(w["vals"][at], pp["want"])


def _select(dt, L, names, where=None, row=0):
    """The piles of sequences(dt, L) whose sequence id is in names, all in output row `row` (+1 for the A-side NaNs)."""
    return [p._replace(row=p.row + row) for p in im.sequences(dt, L, where, only=names)]


def _lay_out(pp, N, seed, filler=None):
    """The piles' columns spread over N (their order kept) and unit-valued filler beside them: filler = {output row: n}
    gives every B row of that output row's k slots whose A value is 1 up to n entries at columns no pile uses.  Returns
    (b as a COO triple, the piles' new columns in pp's CSR order)."""
    rng = np.random.default_rng(seed)
    T = pp["want"].dtype.type
    cmap = np.sort(rng.choice(N, pp["N"], replace=False))
    free = np.setdiff1d(np.arange(N), cmap)
    br, bc, bv = pp["b"]
    br, bc = br.astype(np.int64), cmap[bc]
    ar, ak, av = pp["a"]
    for row, n in (filler or {}).items():
        ks = ak[(av == 1) & (ar == row)].astype(np.int64)
        fk = np.repeat(ks, n)
        fc = free[rng.integers(0, len(free), len(fk))]
        key = np.unique(fk * N + fc)                      # (a column drawn twice for one k: once)
        br, bc, bv = np.concatenate([br, key // N]), np.concatenate([bc, key % N]), np.concatenate([bv, np.ones(len(key), T)])
    order = np.lexsort((bc, br))
    return (br[order].astype(np.uint32), bc[order].astype(np.uint32), bv[order]), cmap[pp["col"]]


# ---- a. short rows in tiles ---------------------------------------------------------------------------------------------
FILL = ("<=512", "<=1024", ">1024")


@functools.lru_cache(maxsize=None)
def _tiles_product(dtname, fill):
    """Every sequence at every length, a few piles per output row; unit filler brings each of these rows to 509, 1021 or
    TileCap - 7 products, and a row that fills a tile by itself follows each, so that each is alone in its tile (the
    recipe of tests/test_gpu_tile_rounds.py): the tile body of every compiled round class sums the piles."""
    dt = np.dtype(dtname).type
    cap = TILE_CAP[np.dtype(dt)]
    piles = [p for L in im.LENGTHS for p in im.sequences(dt, L)]
    pp = im.pile_product(dt, piles, row_cap=480)
    target = {"<=512": 509, "<=1024": 1021, ">1024": cap - 7}[fill]
    assert pp["row_products"].max() <= 480 < target <= cap
    N = 1 << 16
    b, cols = _lay_out(pp, N, 5)
    rng = np.random.default_rng(6)
    M0, K0 = pp["M"], pp["K"]
    free = np.setdiff1d(np.arange(N), cols)
    # B rows K0 .. K0 + M0 - 1: the filler of pile row r; B row K0 + M0: a whole tile
    fill_n = target - pp["row_products"]
    fr = np.concatenate([np.full(n, K0 + r) for r, n in enumerate(fill_n)] + [np.full(cap, K0 + M0)])
    fc = np.concatenate([np.sort(rng.choice(free, n, replace=False)) for n in fill_n] + [np.sort(rng.choice(N, cap, replace=False))])
    b = (np.concatenate([b[0], fr]).astype(np.uint32), np.concatenate([b[1], fc]).astype(np.uint32), np.concatenate([b[2], np.ones(len(fr), dt)]))
    ar, ak, av = pp["a"]
    a = (np.concatenate([2 * ar, 2 * np.arange(M0), 2 * np.arange(M0) + 1]).astype(np.uint32),
         np.concatenate([ak, K0 + np.arange(M0), np.full(M0, K0 + M0)]).astype(np.uint32), np.concatenate([av, np.ones(2 * M0, dt)]))
    order = np.lexsort((a[1], a[0]))
    a = tuple(x[order] for x in a)
    return Product(dt, 2 * M0, K0 + M0 + 1, N, a, b, pp=pp, rows=2 * pp["row"], cols=cols, target=target, pile_rows=M0)


def _gathers(ctx):
    return ctx.algorithm == "outer" and os.environ.get("OSP_GATHER") != "0" and os.environ.get("OSP_DIRECT") != "0"


@pytest.mark.parametrize("fill", FILL)
@pytest.mark.parametrize("dt", DTYPES)
def test_short_rows_in_tiles(ctx, port, dt, fill):
    """Thread-summed runs (up to kRunShort = 16 entries from their head) and wave-summed ones (the rest, 64 at a time), in
    tiles of every round class."""
    p = _tiles_product(np.dtype(dt).name, fill)
    p.check_piles(port, p.notes["pp"], p.notes["rows"], p.notes["cols"])
    got = p.run(ctx)
    print(fill, {k: got.info[k] for k in ("partials", "light_tiles", "heavy_rows", "gathered_short_partials")})
    assert got.info["heavy_rows"] == 0 and got.info["light_tiles"] == p.M, got.info   # every row alone in its tile
    if _gathers(ctx):
        assert got.info["gathered_short_partials"] >= p.notes["pile_rows"] * p.notes["target"], got.info
    assert_same(got, p.want(port))
    got.close()


# ---- b. planned long rows -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_row_product(dtname):
    """Output row 0: every sequence at L = 81 and L = 300, the piles' columns spread over N = 2^18 with unit filler beside
    them (narrow, it would be a row of dense column ranges): some 30 000 products in hundreds of chunks: the four-wave planner."""
    dt = np.dtype(dtname).type
    pp = im.pile_product(dt, im.sequences(dt, 81) + im.sequences(dt, 300))
    N = 1 << 18
    b, cols = _lay_out(pp, N, 7, filler={0: 8})
    return Product(dt, pp["M"], pp["K"], N, pp["a"], b, pp=pp, rows=pp["row"], cols=cols)


@functools.lru_cache(maxsize=None)
def _few_chunks_product(dtname):
    """The transposed shape: rows of at most 64 A entries, each hitting a long B row -- small planned rows (the one-wave
    planner, tests/test_gpu_plan_small.py).  Row 0: every sequence at L = 17 (its k slots: 17 and one per factor asked on
    the A side); row 2: the sequences with no factor on the A side at L = 64, 64 chunks exactly."""
    dt = np.dtype(dtname).type
    cap = TILE_CAP[np.dtype(dt)]
    plain = _select(dt, 64, {"z1", "z2", "z4", "u2a", "u2b", "o2", "o3", "m1", "n1", "n3", "n4"}, row=2)
    pp = im.pile_product(dt, im.sequences(dt, 17) + plain)
    N = 1 << 18
    b, cols = _lay_out(pp, N, 8, filler={0: 100, 2: 10})
    chunk = np.bincount(b[0], minlength=pp["K"])
    small = []
    for r in (0, 2):
        ks = pp["a"][1][pp["a"][0] == r]
        U, nc = int(chunk[ks].sum()), len(ks)
        assert nc <= 64 and U > cap and eligible(U, nc, cap), (r, U, nc)
        small.append((U, nc))
    return Product(dt, pp["M"], pp["K"], N, pp["a"], b, pp=pp, rows=pp["row"], cols=cols, small=small)


@pytest.mark.parametrize("shape", ["hundreds of chunks", "at most 64 chunks"])
@pytest.mark.parametrize("dt", DTYPES)
def test_planned_long_rows(ctx, port, dt, shape):
    """Long rows planned into column ranges: gathered by the merge kernel (outer), written by the multiply (outer-written,
    rowwise) or split after it (outer-split)."""
    p = (_long_row_product if shape.startswith("hundreds") else _few_chunks_product)(np.dtype(dt).name)
    p.check_piles(port, p.notes["pp"], p.notes["rows"], p.notes["cols"])
    got = p.run(ctx)
    i = got.info
    print(shape, {k: i[k] for k in ("partials", "heavy_rows", "direct_rows", "gathered_rows", "dense_segments", "sorted_segments")})
    assert i["heavy_rows"] >= 1
    if os.environ.get("OSP_DIRECT") == "0":
        assert i["direct_rows"] == 0 and i["split_partials"] > 0, i
    else:
        assert i["direct_rows"] >= 1, i
    if _gathers(ctx):
        assert i["gathered_rows"] >= 1, i
    assert_same(got, p.want(port))
    got.close()


# ---- c, d, e. over-long segments ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment_product(dtname, K):
    """The shape of test_long_rows_split_and_fallback (M = 8, N = 64, rows of K dense k): output row r's hot column collects
    K products carrying, row by row, o2 (overflow at the fifth term, then -h), n1 with the +inf at 0, 63, 64, min(4095, K - 2)
    and K - 1, z1 and u2; its neighbours carry z2, z3, m1 (K products as well at K = 6000) and the subnormal-to-normal pile."""
    dt = np.dtype(dtname).type
    hot = [("o2", None), ("n1", 0), ("n1", 63), ("n1", 64), ("n1", min(4095, K - 2)), ("n1", K - 1), ("z1", None), ("u2a", None)]
    piles = []
    for r, (name, e) in enumerate(hot):
        piles += _select(dt, K, {name}, where=[] if e is None else [e], row=r)
        piles += _select(dt, 300, {"z2", "z3a"}, row=r) + _select(dt, 81, {"z3b", "u2b"}, row=r)
        piles += _select(dt, K if K > 4096 else 300, {"m1"}, row=r)
    pp = im.pile_product(dt, piles)
    assert pp["M"] == 8 and pp["N"] == 6
    # the piles at columns 5 .. 10 of 64, as the hot column 5 and its neighbours there
    b = (pp["b"][0], pp["b"][1] + np.uint32(5), pp["b"][2])
    return Product(dt, 8, pp["K"], 64, pp["a"], b, pp=pp, rows=pp["row"], cols=pp["col"] + 5)


@pytest.mark.parametrize("how", ["atomic", "ballot"])
def test_dense_accumulators_both_ways(port, monkeypatch, how):
    """dense_segment_kernel with one LDS floating-point atomic per 64 entries (accumulators start as -0.0) and by ballot
    ranks (a column's sum starts as its first entry)."""
    from outerspace_amd import spgemm as S
    monkeypatch.setenv("OSP_DENSE_ADD", how)
    with S.Context(0) as c:
        for dt in DTYPES:
            p = _segment_product(np.dtype(dt).name, 6000)
            p.check_piles(port, p.notes["pp"], p.notes["rows"], p.notes["cols"])
            got = p.run(c)
            print(how, {k: got.info[k] for k in ("partials", "heavy_rows", "dense_segments", "sorted_segments", "dense_atomic")})
            assert got.info["dense_segments"] >= 1 and got.info["heavy_rows"] >= 8, got.info
            assert_same(got, p.want(port))
            got.close()


@pytest.mark.parametrize("path", ["in-place tile", "global sort", "global sort for all"])
@pytest.mark.parametrize("dt", DTYPES)
def test_segments_through_the_big_tile_and_the_global_sort(ctx, port, monkeypatch, dt, path):
    """OSP_DENSE_SEG=0: a hot column of 3000 products (a segment of at most 4096: the big in-place tile) and one of 6000 (the
    global sort); OSP_BIGTILE_CAP=0 sends the first to the global sort as well."""
    monkeypatch.setenv("OSP_DENSE_SEG", "0")
    if path == "global sort for all":
        monkeypatch.setenv("OSP_BIGTILE_CAP", "0")
    p = _segment_product(np.dtype(dt).name, 6000 if path == "global sort" else 3000)
    p.check_piles(port, p.notes["pp"], p.notes["rows"], p.notes["cols"])
    got = p.run(ctx)
    print(path, {k: got.info[k] for k in ("partials", "heavy_rows", "dense_segments", "sorted_segments", "sorted_partials")})
    assert got.info["heavy_rows"] >= 8 and got.info["dense_segments"] == 0, got.info
    assert (got.info["sorted_segments"] >= 1) == (path != "in-place tile"), got.info
    assert_same(got, p.want(port))
    got.close()


@pytest.mark.parametrize("row_max", ["0", "6000", None])
@pytest.mark.parametrize("dt", DTYPES)
def test_segment_rows_through_both_split_kernels(ctx, port, monkeypatch, dt, row_max):
    """OSP_SPLIT_ROW_MAX moves the rows of the shape above between the stretch split and the one-workgroup split (where the
    formulation splits its long rows after the multiply; the others plan them -- the same bits every way)."""
    if row_max is not None:
        monkeypatch.setenv("OSP_SPLIT_ROW_MAX", row_max)
    p = _segment_product(np.dtype(dt).name, 6000)
    got = p.run(ctx)
    i = got.info
    print(row_max, {k: i[k] for k in ("heavy_rows", "direct_rows", "split_launches", "split_partials", "dense_segments", "hub_rows")})
    assert i["heavy_rows"] >= 8
    if os.environ.get("OSP_DIRECT") == "0":   # every row holds more than 6000 products
        assert (i["split_launches"] >= 1) == (row_max is None) and i["direct_rows"] == 0, i
    assert_same(got, p.want(port))
    got.close()


@functools.lru_cache(maxsize=None)
def _stretch_product(dtname):
    """N = 2^20, as tests/test_gpu_split_from_b.py: row 0 holds every sequence at L = 300 (a stretch row under FORCE: more
    than 6000 products), row 1 its A-side NaN piles (2700 products: split by one workgroup), rows 2 and 3 the same at
    L = 81 with filler (a second stretch row)."""
    dt = np.dtype(dtname).type
    pp = im.pile_product(dt, im.sequences(dt, 300) + [q._replace(row=q.row + 2) for q in im.sequences(dt, 81)])
    N = 1 << 20
    b, cols = _lay_out(pp, N, 9, filler={2: 30})
    U = np.bincount(pp["a"][0], weights=np.bincount(b[0], minlength=pp["K"])[pp["a"][1]], minlength=4).astype(np.int64)
    assert U[0] > 6000 and 2500 < U[1] <= 6000 and U[2] > 6000 and U[3] <= 2500, U
    return Product(dt, pp["M"], pp["K"], N, pp["a"], b, pp=pp, rows=pp["row"], cols=cols, U=U)


@pytest.mark.parametrize("from_b", [None, "2", "0"])
@pytest.mark.parametrize("expand", [None, "0"])
@pytest.mark.parametrize("dt", DTYPES)
def test_rows_beyond_the_planner(_ctx_shared, port, monkeypatch, capfd, dt, expand, from_b):
    """Stretch rows split from B (split_scatter_kernel<.., true> forms the products), after the join, or from staged records;
    the row between the planner's and the stretch split's limits expanded by expand_rows_kernel or staged by the multiply."""
    c = _ctx_shared
    c.algorithm = "outer"
    for k, v in dict(FORCE, OSP_HUB="0", OSP_VERBOSE="1").items():
        monkeypatch.setenv(k, v)
    for name, v in (("OSP_SPLIT_FROM_B", from_b), ("OSP_EXPAND_ROWS", expand)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    p = _stretch_product(np.dtype(dt).name)
    p.check_piles(port, p.notes["pp"], p.notes["rows"], p.notes["cols"])
    capfd.readouterr()
    got = p.run(c)
    lines = stretch_lines(capfd.readouterr().err)
    i, U = got.info, p.notes["U"]
    print(expand, from_b, lines, {k: i[k] for k in ("heavy_rows", "direct_rows", "split_launches", "split_partials", "expand_partials", "hub_rows")})
    assert i["heavy_rows"] == 3 and i["hub_rows"] == 0 and i["direct_rows"] == 0 and i["split_partials"] == U[1], i
    if expand is None:   # the rows are expanded (the stretch rows too, unless they are split from B)
        how = {None: "B", "2": "B, after the join", "0": "staged records"}[from_b]
        assert lines == [(2, int(U[0] + U[2]), how)], lines
        assert i["expand_partials"] == U[1] + (U[0] + U[2] if from_b == "0" else 0), i
    else:                # every long row is staged by the multiply and split from its records
        assert i["expand_partials"] == 0 and i["expand_launches"] == 0, i
    assert_same(got, p.want(port))
    got.close()


# ---- f. hub rows --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hub_product(dtname):
    """One output row beyond OSP_SPLIT_ROW_MAX = 3000: every sequence at L = 300 (u1's factors are on the A side) and hot
    columns of 3000 products carrying z1, o2, m1 and n1 at both ends, spread over N = 2^20 with filler."""
    dt = np.dtype(dtname).type
    piles = im.sequences(dt, 300) + _select(dt, 3000, {"z1", "o2", "m1", "n1"}, where=[0, 2999])
    pp = im.pile_product(dt, piles)
    N = 1 << 20
    b, cols = _lay_out(pp, N, 10, filler={0: 2})
    return Product(dt, pp["M"], pp["K"], N, pp["a"], b, pp=pp, rows=pp["row"], cols=cols)


@pytest.mark.parametrize("dt", DTYPES)
def test_hub_rows(port, monkeypatch, _ctx_shared, dt):
    """The switches of test_hub_rows_written_by_the_multiply: the multiply writes the row through cells into column blocks."""
    for k, v in dict(OSP_HUB="1", OSP_HUB_MIN_SHARE="0", OSP_HUB_MIN_RUN="0", OSP_SPLIT_ROW_MAX="3000", OSP_DIRECT_MAX="3000").items():
        monkeypatch.setenv(k, v)
    c = _ctx_shared
    c.algorithm = "outer"
    p = _hub_product(np.dtype(dt).name)
    p.check_piles(port, p.notes["pp"], p.notes["rows"], p.notes["cols"])
    got = p.run(c)
    print({k: got.info[k] for k in ("partials", "heavy_rows", "hub_rows", "hub_partials", "dense_segments", "sorted_segments")})
    assert got.info["hub_rows"] >= 1 and got.info["hub_partials"] > 30000, got.info
    assert_same(got, p.want(port))
    got.close()


# ---- g. sums across parts -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parts_product(dtname):
    """Every sequence at L = 17 and L = 81 in output rows 0 and 1: the piles share their k slots, so a cut in k falls inside
    all of them at once."""
    dt = np.dtype(dtname).type
    pp = im.pile_product(dt, im.sequences(dt, 17) + im.sequences(dt, 81))
    return Product(dt, pp["M"], pp["K"], pp["N"], pp["a"], pp["b"], pp=pp, rows=pp["row"], cols=pp["col"])


def _cuts(pp):
    """k cuts inside the piles of _parts_product, by term index: before and after o2's overflow (its fifth term), between
    the +inf and the -inf of every n1 (-inf at term (e + L) // 2, or before a +inf at L - 1), and at the row boundary."""
    k = lambda t: pp["first_k"][(0, t)]   # noqa: E731
    return [(k(4),), (k(6),), (k(1), k(9)), (k(16), k(41)), (k(20), k(80)), (k(50), pp["first_k"][(1, 0)])]


def _device(p):
    import torch
    t = [torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).to("cuda:0") for a in (*p.acsc, *p.bcsr)]
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("dt", DTYPES)
def test_k_shards_of_partial_products(ctx, port, dt):
    """The multiply alone per k range, the parts merged once in ascending k (osp_merge_record_parts, the exchange of the
    multi-GPU path): the same chain of additions as the uncut product, so the uncut oracle's bits -- wherever the cut."""
    p = _parts_product(np.dtype(dt).name)
    want = p.want(port)
    t = _device(p)
    ptrs = [x.data_ptr() for x in t]
    for cut in _cuts(p.notes["pp"]):
        edges = [0, *cut, p.K]
        parts = [ctx.spgemm_partials_device(dt, p.M, p.K, p.N, ptrs, k_range=(k0, k1)) for k0, k1 in zip(edges, edges[1:])]
        assert sum(x.nnz for x in parts) == want["partials"] and all(x.nnz > 0 for x in parts)
        got = ctx.merge_record_parts_device(dt, p.M, p.N, [x.partials_ptrs() for x in parts])
        assert np.array_equal(got.rowptr, want["rowptr"]) and np.array_equal(got.colidx, want["colidx"])
        im.assert_same_bits(got.vals, want["vals"])
        for x in parts + [got]:
            x.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_k_shards_of_sums(ctx, port, dt):
    """Each k range as a product of its own equals the oracle's slab by bits; merge_csr_parts then adds the slabs' SUMS in
    part order, which re-associates the chain ((h+h+h) + (h+h-h...) is not h+h+h+h+h-h...): the expected bits are the chain
    over the oracle's slabs, entry by entry -- an overflow on one side of the cut and a NaN from +inf + -inf across it."""
    p = _parts_product(np.dtype(dt).name)
    T = np.dtype(dt).type
    for cut in _cuts(p.notes["pp"]):
        edges = [0, *cut, p.K]
        parts, model = [], {}
        for kr in zip(edges, edges[1:]):
            w = p.want(port, kr)
            got = p.run(ctx, k_range=kr)
            assert_same(got, w)
            parts.append((got.rowptr.copy(), got.colidx.copy(), got.vals.copy()))
            got.close()
            rows = np.repeat(np.arange(p.M), np.diff(w["rowptr"]))
            with np.errstate(all="ignore"):
                for r, c, v in zip(rows, w["colidx"], w["vals"]):
                    model[(r, c)] = T(model[(r, c)] + v) if (r, c) in model else v
        merged = ctx.merge_csr_parts(p.M, p.N, parts)
        keys = sorted(model)
        assert np.array_equal(np.repeat(np.arange(p.M), np.diff(merged.rowptr)), [r for r, _ in keys])
        assert np.array_equal(merged.colidx, [c for _, c in keys])
        im.assert_same_bits(merged.vals, np.array([model[k] for k in keys], T))
        merged.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_panels_and_row_shards(ctx, port, dt):
    """The tiles product of (a) in row panels -- resident and streamed -- and as row shards."""
    import torch
    from outerspace_amd.distributed import _as_tensor
    p = _tiles_product(np.dtype(dt).name, "<=512")
    want = p.want(port)
    P = want["partials"]
    got = p.run(ctx, partial_capacity=P // 6)
    assert got.info["panels"] >= 6
    assert_same(got, want)
    got.close()
    t = _device(p)
    dev = torch.device("cuda:0")
    vt, vs = (torch.float64, "<f8") if dt == np.float64 else (torch.float32, "<f4")
    seen = []

    def on_panel(q):
        lo, hi = want["rowptr"][q["row_begin"]], want["rowptr"][q["row_end"]]
        assert q["nnz"] == hi - lo
        ci = _as_tensor(q["colidx"], q["nnz"], "<i4", dev, torch.int32).cpu().numpy().view(np.uint32)
        cv = _as_tensor(q["vals"], q["nnz"], vs, dev, vt).cpu().numpy()
        seen.append((q["row_begin"], q["row_end"], np.array_equal(ci, want["colidx"][lo:hi]), cv))
    info = ctx.spgemm_csc_csr_panels(dt, p.M, p.K, p.N, [x.data_ptr() for x in t], on_panel, partial_capacity=P // 5 + 1)
    assert info["panels"] == len(seen) >= 5 and seen[0][0] == 0 and seen[-1][1] == p.M and all(s[2] for s in seen)
    im.assert_same_bits(np.concatenate([s[3] for s in seen]), want["vals"])
    end = 0
    for i in range(3):
        r = p.run(ctx, row_shard=(i, 3))
        r0, r1 = r.info["row_begin"], r.info["row_end"]
        assert r0 == end
        lo, hi = want["rowptr"][r0], want["rowptr"][r1]
        assert np.array_equal(r.rowptr, want["rowptr"][r0:r1 + 1] - lo) and np.array_equal(r.colidx, want["colidx"][lo:hi])
        im.assert_same_bits(r.vals, want["vals"][lo:hi])
        end = r1
        r.close()
    assert end == p.M


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("dt", DTYPES)
def test_ranks_of_the_library(port, dt, nranks):
    """The k-sharded product inside the library (logical ranks on one device, as tests/test_gpu_multi.py): slabs of k cut
    inside the piles, partial products sent to their row's owner, merged in rank order."""
    from outerspace_amd import spgemm as S
    from tests.test_gpu_multi import _devices
    for p in (_parts_product(np.dtype(dt).name), _tiles_product(np.dtype(dt).name, "<=512")):
        want = p.want(port)
        with S.MultiGpu(_devices(nranks)) as mg:
            info, (rowptr, colidx, v) = mg.spgemm_csc_csr(p.M, p.K, p.N, *p.acsc, *p.bcsr, validate=True)
            assert info["nranks"] == nranks and info["partials"] == want["partials"]
            ranks = info["ranks"]
            print(p.K, [(r["k_begin"], r["k_end"], r["partials_local"]) for r in ranks])
            assert ranks[0]["k_begin"] == 0 and ranks[-1]["k_end"] == p.K and all(x["k_end"] == y["k_begin"] for x, y in zip(ranks, ranks[1:]))
            if p.M == 2:   # the slabs are balanced by products: every cut falls inside the piles of output row 0
                assert all(0 < r["k_end"] < p.notes["pp"]["first_k"][(1, 0)] for r in ranks[:-1]), ranks
            assert np.array_equal(rowptr, want["rowptr"]) and np.array_equal(colidx, want["colidx"])
            im.assert_same_bits(v, want["vals"])


# ---- h. the epilogue ----------------------------------------------------------------------------------------------------
def _epilogue_model(dt, M, N, entries, bias, relu):
    """osp_epilogue.h's expression in numpy: v = c + bias (an absent entry counts as 0 under a bias, stored entries only
    without one), relu: v > 0 ? v : 0 -- so a NaN becomes 0 --, and what is zero is dropped."""
    T = np.dtype(dt).type
    out = []
    with np.errstate(all="ignore"):
        for r in range(M):
            for j in range(N):
                if bias is None and (r, j) not in entries:
                    continue
                v = T(entries.get((r, j), T(0)) + (T(0) if bias is None else T(bias[j])))
                if relu and not v > 0:
                    v = T(0)
                if v != 0:
                    out.append((r, j, v))
    return out


@pytest.mark.parametrize("dt", DTYPES)
def test_bias_relu_on_non_finite_entries(_ctx_shared, port, dt):
    """relu(NaN) is 0 here (torch keeps the NaN): with relu, NaN, -inf, both zeros and negative subnormals are dropped, +inf,
    positive subnormals and max kept bit for bit; without relu only the zeros go and the NaN stays."""
    T, f = np.dtype(dt).type, np.finfo(dt)
    c = _ctx_shared
    c.algorithm = "outer"
    sub, mx = T(f.smallest_subnormal), T(f.max)
    V = [T(np.nan), T(np.inf), T(-np.inf), T(-0.0), T(0.0), sub, -sub, mx, T(1), -mx, T(f.tiny) / T(2)]
    B = [T(np.inf), T(-np.inf), T(np.nan), T(0.0), T(-0.0), T(1), -mx, sub, mx, -sub]
    M, N = len(V), 70                                    # more columns than a wave: two rounds of the biased pass
    entries = {(r, j): V[(r + j) % len(V)] for r in range(M) for j in range(N) if j % 5 != 4}
    bias = np.array([B[j % len(B)] for j in range(N)], T)
    # a result with exactly these entries: C = I * B
    keys = sorted(entries)
    b = (np.array([r for r, _ in keys], np.uint32), np.array([j for _, j in keys], np.uint32), np.array([entries[k] for k in keys], T))
    eye = (np.arange(M, dtype=np.uint32), np.arange(M, dtype=np.uint32), np.ones(M, T))
    p = Product(dt, M, M, N, eye, b)
    res = p.run(c)
    assert_same(res, p.want(port))
    im.assert_same_bits(res.vals, b[2])
    for use_bias, relu in ((False, True), (False, False), (True, True), (True, False)):
        got = res.bias_relu(bias if use_bias else None, relu=relu)
        want = _epilogue_model(dt, M, N, entries, bias if use_bias else None, relu)
        assert np.array_equal(np.repeat(np.arange(M), np.diff(got.rowptr)), [r for r, _, _ in want]), (use_bias, relu)
        assert np.array_equal(got.colidx, [j for _, j, _ in want]), (use_bias, relu)
        im.assert_same_bits(got.vals, np.array([v for _, _, v in want], T))
        if not use_bias:   # stated literally: what stays of each kind of entry
            kept = {T(x).tobytes() for x in got.vals if not np.isnan(x)}
            stay = [T(np.inf), sub, mx, T(1), T(f.tiny) / T(2)] + ([] if relu else [T(-np.inf), -sub, -mx])
            assert kept == {x.tobytes() for x in stay}, (relu, got.vals)
            assert np.isnan(got.vals).any() == (not relu)
        got.close()
    res.close()
