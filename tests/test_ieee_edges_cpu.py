"""The reference of tests/test_gpu_ieee_edges.py, pinned before the kernels are judged against it (no GPU needed).

For every sequence of tests/ieee_model.py, every pile length and both value types the CPU oracle's product must equal the
plain left-to-right chain of the model bit for bit, NaNs by position; and the NaN positions must be exactly the piles
DESIGNED to be NaN.  That cap keeps the position-only rule from hiding anything: an output that is NaN where the design
says a number (or the other way round) fails here, on the oracle, and so fails on the GPU.
"""
import numpy as np
import pytest

from tests import ieee_model as im

# designed NaN piles per length: per event position n2a, n2b, n3, n3A, and n1 where a pile holds two terms (events:
# {0, 1, 15, 16, 17, 79, 80, 81, L - 1} below L)
NAN_PILES = {1: 4, 2: 10, 15: 15, 16: 15, 17: 20, 63: 30, 64: 30, 65: 30, 80: 30, 81: 35, 300: 45}


def test_the_comparator_compares_bits():
    for dt in (np.float32, np.float64):
        f = np.finfo(dt)
        v = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, f.smallest_subnormal, f.tiny, f.max, 1.0], dt)
        im.assert_same_bits(v, v.copy())
        other_nan = v.copy()
        other_nan.view(im._uint(dt))[2] |= 1 << (8 * v.itemsize - 1)   # the NaN of the other sign: same position
        assert np.isnan(other_nan[2])
        im.assert_same_bits(v, other_nan)
        for i, x in ((0, -0.0), (1, 0.0), (2, 1.0), (8, np.nan), (5, 0.0), (7, np.inf), (8, np.nextafter(dt(1), dt(2)))):
            w = v.copy()
            w[i] = x
            with pytest.raises(AssertionError):
                im.assert_same_bits(v, w)
        with pytest.raises(AssertionError):
            im.assert_same_bits(v, v[:-1])
    with pytest.raises(AssertionError):
        im.assert_same_bits(np.zeros(3, np.float32), np.zeros(3, np.float64))


def test_the_model_on_hand_made_piles():
    for dt in (np.float32, np.float64):
        T, f = np.dtype(dt).type, np.finfo(dt)
        h = T(f.max / 4)
        assert np.signbit(im.chain(dt, [(1, -0.0)] * 3)) and not np.signbit(im.chain(dt, [(1, -0.0), (1, 0.0)]))
        assert np.signbit(im.chain(dt, [(-0.0, 3)])) and im.chain(dt, [(-0.0, 3)]) == 0
        assert im.chain(dt, [(0.5, f.tiny)]) == T(f.tiny) / 2 > 0
        assert im.chain(dt, [(1, h)] * 5 + [(1, -h)] * 5) == np.inf
        assert np.isfinite(im.chain(dt, [(1, h), (1, -h)] * 5))
        assert np.isnan(im.chain(dt, [(1, np.inf), (1, 1), (1, -np.inf)]))
        assert im.chain(dt, [(1, 3 * f.smallest_subnormal)] * 7) == 21 * T(f.smallest_subnormal)


@pytest.mark.parametrize("L", im.LENGTHS)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_oracle_equals_the_model(port, dt, L):
    from outerspace_amd import spgemm as S
    piles = im.sequences(dt, L)
    names = {p.name.split("/")[0] for p in piles}
    if L in (1, 17, 81, 300):   # every sequence at these lengths (a cancelling pair / an inf - inf need two terms)
        assert names >= {"z1", "z2", "z3a", "z3b", "u1a", "u1b", "u1c", "u2a", "u2b", "o1", "o2", "o3", "n2a", "n2b", "n3", "n3A",
                         "n4", "m1"} | ({"z4", "n1"} if L > 1 else set()), names
    pp = im.pile_product(dt, piles)
    assert pp["nan"].sum() == NAN_PILES[L] == im.nan_count(L)
    # the model says NaN exactly where the design does
    assert np.array_equal(np.isnan(pp["want"]), pp["nan"])
    acsc, bcsr = S.coo_to_csc(pp["K"], *pp["a"]), S.coo_to_csr(pp["K"], *pp["b"])
    got = port.spgemm(pp["M"], pp["K"], pp["N"], *acsc, *bcsr)
    assert got["partials"] == sum(len(p.terms) for p in piles)
    assert np.array_equal(np.repeat(np.arange(pp["M"]), np.diff(got["rowptr"])), pp["row"])   # every pile is an entry, zeros too
    assert np.array_equal(got["colidx"], pp["col"])
    im.assert_same_bits(got["vals"], pp["want"])
    assert np.isnan(got["vals"]).sum() == NAN_PILES[L]
    assert np.array_equal(np.isnan(got["vals"]), pp["nan"])
    # what the sequences are for: the signs of the zeros, the subnormals, the infinities
    by = dict(zip(pp["names"], got["vals"]))
    T, f = np.dtype(dt).type, np.finfo(dt)
    z = lambda n: by[f"{n}/L{L}"]   # noqa: E731
    assert z("z1") == 0 and np.signbit(z("z1")) and np.signbit(z("z3a")) and np.signbit(z("z3b")) and np.signbit(z("u1c"))
    assert z("z2") == 0 and np.signbit(z("z2")) == (L == 1) and z("u1b") == 0 and not np.signbit(z("u1b"))
    assert z("u1a") == T(f.tiny) / 2 and z("u2a") == T(3 * L) * T(f.smallest_subnormal)
    assert (0 < z("u2b") < f.tiny) == (L == 1)
    assert (z("o2") == np.inf) == (L >= 5) and (z("o3") == -np.inf) == (L >= 5)
    if L > 1:
        assert z("z4") == 0 and not np.signbit(z("z4"))
    assert all(by[n] == np.inf for n in by if n.startswith(("o1/", "n4/")))


def test_packing_into_rows_and_factors_on_the_a_side():
    """row_cap spreads the piles over output rows without changing a value; a_vals puts a factor on every plain slot."""
    dt = np.float32
    piles = im.sequences(dt, 17) + im.sequences(dt, 81)
    one, packed = im.pile_product(dt, piles), im.pile_product(dt, piles, row_cap=400)
    assert packed["M"] > one["M"] == 2 and packed["row_products"].max() <= 400
    got = dict(zip(packed["names"], packed["want"].view(np.uint32)))
    assert all(np.isnan(w) or got[n] == b for n, w, b in zip(one["names"], one["want"], one["want"].view(np.uint32)))
    t = np.float32(np.finfo(dt).tiny)
    pp = im.pile_product(dt, [im.Pile("x", [(1, t)] * 3)], a_vals=[np.float32(0.5), np.float32(0.25)])
    assert pp["a"][2].tolist() == [0.5, 0.25, 0.5] and pp["want"][0] == t * np.float32(1.25)
