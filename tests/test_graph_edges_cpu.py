"""CPU-side checks of the argument handling the Python surface shares: the one edge-list check
behind every torch builder of ``graph.py`` -- its refusals, the inferred ``n``, the empty list, the input kinds --, the
directed pattern builder against scipy, and the two conventions on which the index-list and dense-argument helpers of
``spgemm.py`` differ between their callers.  No GPU and no library handle."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from outerspace_amd import graph
from outerspace_amd import spgemm as S

# name -> (builder, takes weights)
BUILDERS = {"oriented_adjacency": (graph.oriented_adjacency, False), "walk_pattern": (graph.walk_pattern, True),
            "symmetric_adjacency": (graph.symmetric_adjacency, False), "weighted_adjacency": (graph.weighted_adjacency, True),
            "directed_pattern": (graph.directed_pattern, False)}
ROWS, COLS = [0, 1, 2, 4, 1], [1, 2, 0, 2, 1]   # (a triangle, a pendant edge, a self loop; vertex 3 has no edge)


@pytest.fixture(params=sorted(BUILDERS))
def builder(request):
    return BUILDERS[request.param]


def test_builders_refuse_a_malformed_edge_list(builder):
    fn, weighted = builder
    bad = [dict(rows=[0, 1, 2], cols=[1, 2]),                  # different lengths
           dict(rows=[[0, 1], [1, 2]], cols=[[1, 2], [2, 0]]),   # a 2-D list
           dict(rows=[0, -1], cols=[1, 0]),                    # a negative id
           dict(rows=[0, 3], cols=[1, 0], n=3)]                # an id equal to n
    if weighted:
        bad.append(dict(rows=ROWS, cols=COLS, weights=[1.0, 2.0]))   # not one weight per edge
    for kw in bad:
        with pytest.raises(ValueError):
            fn(**kw)
        with pytest.raises(ValueError):
            fn(**{k: np.asarray(v) if k != "n" else v for k, v in kw.items()})


def test_builders_infer_n_and_take_an_empty_list(builder):
    fn, _ = builder
    out = fn(ROWS, COLS)
    assert out[0] == 5 and out[1].shape == (6,) and out[1].dtype == torch.int64
    assert int(out[1][-1]) == out[2].numel()
    out = fn(ROWS, COLS, 9)
    assert out[0] == 9 and out[1].shape == (10,)
    out = fn([], [])
    assert out[0] == 0 and out[1].tolist() == [0] and out[2].numel() == 0


def test_builders_give_the_same_arrays_for_every_input_kind(builder):
    fn, weighted = builder
    w = [3.0, 1.0, 2.0, 5.0, 4.0]
    kinds = [lambda x, dt: list(x), lambda x, dt: np.asarray(x, dt), lambda x, dt: torch.as_tensor(np.asarray(x, dt))]
    outs = []
    for kind in kinds:
        kw = {"weights": kind(w, np.float64)} if weighted else {}
        outs.append(fn(kind(ROWS, np.int64), kind(COLS, np.int64), **kw))
    for other in outs[1:]:
        assert other[0] == outs[0][0] and len(other) == len(outs[0])
        for a, b in zip(outs[0][1:], other[1:]):
            assert a.dtype == b.dtype and torch.equal(a, b)
    # an int32 edge list is the same list
    again = fn(np.asarray(ROWS, np.int32), torch.as_tensor(COLS, dtype=torch.int32), **({"weights": np.asarray(w, np.float32)} if weighted else {}))
    for a, b in zip(outs[0][1:], again[1:]):
        assert torch.equal(a, b)


# ---- directed_pattern ------------------------------------------------------------------------------------------------------------
# 7 vertices: a self loop (0, 0), a duplicate edge (1, 2), an edge in both directions (2, 3) / (3, 2), vertex 5 without an
# edge, vertex 6 with in-edges only
D_ROWS = [4, 0, 1, 2, 1, 3, 0, 4]
D_COLS = [6, 0, 2, 3, 2, 2, 6, 1]


def test_directed_pattern_equals_scipys_deduplicated_pattern():
    n, rowptr, colidx, vals = graph.directed_pattern(D_ROWS, D_COLS, 7)
    ref = sp.csr_matrix((np.ones(len(D_ROWS)), (D_ROWS, D_COLS)), shape=(7, 7))
    ref.sum_duplicates()
    ref.sort_indices()
    assert n == 7 and rowptr.dtype == colidx.dtype == torch.int64 and vals.dtype == torch.float64
    assert rowptr.tolist() == ref.indptr.tolist() and colidx.tolist() == ref.indices.tolist()
    assert vals.tolist() == [1.0] * ref.nnz and ref.nnz == len(D_ROWS) - 1   # (only the duplicate went)
    dense = torch.zeros(7, 7)
    dense[torch.repeat_interleave(torch.arange(7), rowptr[1:] - rowptr[:-1]), colidx] = 1.0
    assert dense[0, 0] == 1.0                                   # the self loop is kept
    assert dense[2, 3] == 1.0 and dense[3, 2] == 1.0            # both directions are two entries
    assert dense[5].sum() == 0 and dense[:, 5].sum() == 0       # the vertex without an edge
    assert dense[6].sum() == 0 and dense[:, 6].sum() == 2       # in-edges only
    for i in range(7):
        row = colidx[rowptr[i]:rowptr[i + 1]]
        assert bool((row[1:] > row[:-1]).all())                 # columns ascend
    assert graph.directed_pattern(D_ROWS, D_COLS)[0] == 7       # inferred: the largest id + 1


# ---- the helpers of spgemm.py: the conventions that differ between their callers --------------------------------------------------
def test_an_empty_index_list_is_a_pointer_for_extract_and_null_for_build():
    for empty, space in (([], "host"), (np.zeros(0, np.int64), "host"), (torch.zeros(0, dtype=torch.int32), "device"), ((0x1000, 0), "device")):
        ptr, count, keep, ascending = S._index_arg(empty, space, "rows")   # extract: NULL would mean "every row"
        assert ptr.value and count == 0 and keep is not None and ascending is True
        addr, count, _ = S._u32_list(empty, space, "rows")                 # build: nothing to read
        if not isinstance(empty, tuple):
            assert addr == 0 and count == 0
    assert S._index_arg(None, "host", "rows") == (None, 0, None, True)
    ptr, count, keep, ascending = S._index_arg([2, 0, 1], "host", "cols")
    assert ptr.value == keep.ctypes.data and count == 3 and keep.dtype == np.uint32 and ascending is False
    assert S._index_arg(torch.tensor([0, 1, 5], dtype=torch.int32), "device", "cols")[3] is True
    assert S._index_arg((0x1000, 3), "device", "cols")[2:] == (None, None)


def test_a_bool_or_uint8_keep_vector_is_accepted():
    for v in ([True, False, True], np.array([1, 0, 2], np.uint8), np.array([True, False, True])):
        ptr, keep = S._dense_arg(v, (3,), np.uint8, "host", "keep_rows")
        assert ptr.value == keep.ctypes.data and keep.dtype == np.uint8 and (keep != 0).tolist() == [True, False, True]
    for v in (torch.tensor([True, False, True]), torch.tensor([1, 0, 2], dtype=torch.uint8)):
        ptr, keep = S._dense_arg(v, (3,), np.uint8, "device", "keep_rows")
        assert ptr.value == v.data_ptr() and keep is v
    with pytest.raises(S.OspError):
        S._dense_arg(torch.tensor([1, 0, 2], dtype=torch.int32), (3,), np.uint8, "device", "keep_rows")   # 4-byte elements
    ptr, keep = S._dense_arg(None, (0,), np.uint8, "device", "keep_rows")
    assert ptr is None and keep is None
    ptr, keep = S._dense_arg(torch.zeros(0, dtype=torch.uint8), (0,), np.uint8, "device", "keep_rows")
    assert ptr.value and keep.size == 1                              # an empty vector: never a null pointer
