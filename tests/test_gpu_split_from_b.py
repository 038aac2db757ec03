"""Stretch rows split straight from B (osp_split.h, split_count_kernel / split_scatter_kernel with FROM_B).

A long row beyond the one-workgroup planner is no longer staged and then moved: the stretch split walks B with the row
walker of expand_rows_kernel (osp_kernels.h, RowWalker) and forms the products it scatters, beside the plan of the next
panel.  The second buffer must hold the same bytes either way.  Every case here is one product of ten to a hundred
thousand partial products, built by hand so that job, round, wave-slice and block boundaries of the walker fall where it
can go wrong, and computed three ways: split from B (the default), with OSP_SPLIT_FROM_B=0 (the rows are expanded into the
staging buffer and split from their records after the multiply), and by the CPU oracle.  rowptr, colidx and vals must be
bit-identical across the three, the counters that describe the plan equal between the two settings, and the OSP_VERBOSE
line of plan_panel must say which way the stretch rows went.

Forcing stretch rows onto small products: OSP_DIRECT_MIN_NNZ=0 OSP_DIRECT_MAX=2500 OSP_SPLIT_ROW_MAX=6000 (rows above 2500
products are not planned, rows above 6000 are stretch rows).  With OSP_HUB_MIN_SHARE=0 OSP_HUB_MIN_RUN=0 beside them --
the soak's switches -- every stretch row becomes a HUB row, written through cells by the multiply: that path is not the
one under test (one case below checks it stays as it was).  So the cases run with OSP_HUB=0, and one with
OSP_HUB_MIN_SHARE=0 and an unreachable OSP_HUB_MIN_RUN: the hub plan is made, refused, and the rows are split with the hub
rows' blocks.

Operands: N = 2^20 columns.  (Below that a row of 70 000 products is a "capped" row -- bins as narrow as the dense
accumulators -- and a capped row is planned, whatever its length.)
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import assert_same, run_both

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 1 << 20
JOB, ROUND, WAVE_SPAN = 32768, 4096, 1024     # kSplitJob, kSplitStretch, a wave's part of a round
FORCE = {"OSP_DIRECT_MIN_NNZ": "0", "OSP_DIRECT_MAX": "2500", "OSP_SPLIT_ROW_MAX": "6000"}
# everything osp_result_info_t says about the plan, but for the expansion's own counters: the rows split from B are not expanded
PLAN_COUNTERS = ("panels", "plans_overlapped", "light_tiles", "heavy_rows", "heavy_partials", "direct_rows", "direct_partials",
                 "gathered_rows", "gathered_partials", "gathered_runs", "gathered_short_partials", "split_launches", "split_partials",
                 "hub_rows", "hub_partials", "sorted_segments", "sorted_partials", "dense_segments", "merge_launches",
                 "direct_plan_launches", "nnz_c", "partials")


class Operands:
    """B rows are appended as needed; a row of A is the list of B rows it multiplies, in ascending k."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b_cols, self.a_rows = [], []

    def b_row(self, length, cols=None):
        if cols is None:
            u = np.unique(self.rng.integers(0, N, length + 64))
            while len(u) < length:
                u = np.unique(np.concatenate([u, self.rng.integers(0, N, length)]))
            cols = np.sort(self.rng.choice(u, length, replace=False)) if len(u) > length else u
        self.b_cols.append(np.asarray(cols, np.uint32))
        return len(self.b_cols) - 1

    def a_row(self, lengths):
        self.a_rows.append([self.b_row(int(n)) for n in lengths])
        return int(sum(lengths))

    def coo(self):
        K = len(self.b_cols)
        b_rows = np.concatenate([np.full(len(c), k, np.uint32) for k, c in enumerate(self.b_cols)])
        b_cols = np.concatenate(self.b_cols)
        a_rows = np.concatenate([np.full(len(ks), i, np.uint32) for i, ks in enumerate(self.a_rows)])
        a_cols = np.concatenate([np.asarray(ks, np.uint32) for ks in self.a_rows])
        a = (a_rows, a_cols, self.rng.uniform(0.5, 1.5, len(a_rows)))
        b = (b_rows, b_cols, self.rng.uniform(0.5, 1.5, len(b_rows)))
        return len(self.a_rows), K, a, b


def stretch_lines(err):
    """(rows, partial products, which way) of every panel's stretch rows, from the OSP_VERBOSE lines of one product."""
    return [(int(r), int(p), how) for r, p, how in
            re.findall(r"stretch rows: (\d+) rows, (\d+) partial products split from (B, after the join|B|staged records)$", err, re.M)]


def three_ways(ctx, port, monkeypatch, capfd, ops, dt, want_rows, want_partials, hub="off", from_b=None, **kw):
    """from_b: the value of OSP_SPLIT_FROM_B for the run under test (None: unset, the default; "2": from B, after the join)."""
    how_on = "B, after the join" if from_b == "2" else "B"
    ctx.algorithm = "outer"
    M, K, a, b = ops.coo()
    for k, v in FORCE.items():
        monkeypatch.setenv(k, v)
    if hub == "off":
        monkeypatch.setenv("OSP_HUB", "0")
    else:   # planned as hub rows, refused for their short runs: split with the hub rows' blocks
        monkeypatch.setenv("OSP_HUB_MIN_SHARE", "0")
        monkeypatch.setenv("OSP_HUB_MIN_RUN", "1e18")
    monkeypatch.setenv("OSP_VERBOSE", "1")
    if from_b is None:
        monkeypatch.delenv("OSP_SPLIT_FROM_B", raising=False)
    else:
        monkeypatch.setenv("OSP_SPLIT_FROM_B", from_b)
    capfd.readouterr()
    on, want = run_both(ctx, port, M, K, N, a, b, dt, **kw)
    lines_on = stretch_lines(capfd.readouterr().err)
    monkeypatch.setenv("OSP_SPLIT_FROM_B", "0")
    off, _ = run_both(ctx, port, M, K, N, a, b, dt, **kw)
    lines_off = stretch_lines(capfd.readouterr().err)
    print(f"stretch rows: {lines_on} (OSP_SPLIT_FROM_B=0: {lines_off}); expand launches {on.info['expand_launches']} / "
          f"{off.info['expand_launches']}, expanded products {on.info['expand_partials']} / {off.info['expand_partials']}")
    assert_same(on, want)
    assert_same(off, want)
    for name in ("rowptr", "colidx", "vals"):
        assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), name
    assert {k: on.info[k] for k in PLAN_COUNTERS} == {k: off.info[k] for k in PLAN_COUNTERS}
    # the stretch rows took the new path: every one of them, in every panel that has any -- and the old one when switched off
    assert lines_on and all(how == how_on for _, _, how in lines_on), lines_on
    assert [(r, p) for r, p, _ in lines_on] == [(r, p) for r, p, _ in lines_off] and all(how == "staged records" for _, _, how in lines_off)
    assert sum(r for r, _, _ in lines_on) == want_rows and sum(p for _, p, _ in lines_on) == want_partials, (lines_on, want_rows, want_partials)
    assert on.info["hub_rows"] == 0
    # ... and were not expanded into the staging buffer first
    assert off.info["expand_partials"] - on.info["expand_partials"] == want_partials
    info = on.info
    on.close()
    off.close()
    return info


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
def test_one_job(_ctx_shared, port, monkeypatch, capfd, dt):
    """A stretch row of one job: 7 000 products, two rounds, the second one short."""
    ops = Operands(1)
    ops.a_row([40, 3])
    U = ops.a_row([100] * 70)
    ops.a_row([9])
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, U)


@pytest.mark.parametrize("hub", ["off", "refused"])
@pytest.mark.parametrize("dt", DTYPES)
def test_three_jobs_boundaries_inside_chunks(_ctx_shared, port, monkeypatch, capfd, dt, hub):
    """70 000 products in chunks of 177: no job, round or wave-span boundary falls on a chunk boundary."""
    ops = Operands(2)
    lengths = [177] * 395 + [85]
    U = ops.a_row(lengths)
    assert U == 70000 and -(-U // JOB) == 3
    ends = set(np.cumsum(lengths).tolist())
    assert not any(x in ends for x in range(WAVE_SPAN, U, WAVE_SPAN))
    ops.a_row([5, 5])
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, U, hub=hub)


@pytest.mark.parametrize("dt", DTYPES)
def test_thousands_of_tiny_chunks_and_empty_b_rows(_ctx_shared, port, monkeypatch, capfd, dt):
    """Chunks of 1 to 3 entries with empty B rows between them: several hundred chunks end inside one wave span (the walker
    holds 64 at a time), and the groups of 64 begin and end anywhere in the blocks."""
    ops = Operands(3)
    lengths = ops.rng.integers(0, 4, 6000)
    lengths[:3] = (0, 0, 1)                                 # the row begins with empty chunks
    lengths[-2:] = 0                                        # ... and ends with them
    U = ops.a_row(lengths)
    assert U > 6000 and (lengths == 0).sum() > 1000
    per_span = np.diff(np.searchsorted(np.cumsum(lengths), np.arange(0, U, WAVE_SPAN)))
    assert per_span.min() > 64, per_span
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, U)


@pytest.mark.parametrize("dt", DTYPES)
def test_dominant_chunk_between_tiny_ones(_ctx_shared, port, monkeypatch, capfd, dt):
    """One chunk longer than a round (5 000 entries) between tiny ones."""
    ops = Operands(4)
    lengths = [2] * 600 + [5000] + [3, 1, 0, 2] * 150
    assert 5000 > ROUND
    U = ops.a_row(lengths)
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, U)


@pytest.mark.parametrize("dt", DTYPES)
def test_last_job_of_one_product(_ctx_shared, port, monkeypatch, capfd, dt):
    ops = Operands(5)
    U = ops.a_row([128] * 255 + [127, 1, 1])
    assert U == JOB + 1
    three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, U)


def _two_panel_operands(seed):
    """Two halves of 10 000 to 14 000 products: short rows, a planned (direct) row and a stretch row each, and in the first a
    row that one workgroup splits (expanded into the staging buffer either way)."""
    ops = Operands(seed)
    halves, stretch = [], 0
    for lengths_stretch in ([61] * 120 + [7], [3] * 1500 + [900, 900, 900]):
        P = 0
        for k in range(6):
            P += ops.a_row(ops.rng.integers(1, 30, 4))
        P += ops.a_row([250] * 8)                            # 2 000 products: planned
        if not halves:
            P += ops.a_row([500] * 8)                        # 4 000 products: split by one workgroup
        U = ops.a_row(lengths_stretch)
        assert U > 6000
        stretch += U
        P += U
        for k in range(5):
            P += ops.a_row(ops.rng.integers(1, 30, 3))
        halves.append(P)
    return ops, halves, stretch


@pytest.mark.parametrize("dt", DTYPES)
def test_two_panels(_ctx_shared, port, monkeypatch, capfd, dt):
    """Two stretch rows beside direct and short rows, cut into two panels: the first panel's split runs beside the plan of
    the second, the second panel's beside nothing."""
    ops, halves, stretch = _two_panel_operands(6)
    info = three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 2, stretch, partial_capacity=max(halves) + 10)
    assert info["panels"] == 2 and info["plans_overlapped"] == 1 and info["direct_rows"] == 2 and info["expand_partials"] == 4000, info


@pytest.mark.parametrize("dt", DTYPES)
def test_two_panels_split_after_the_join(_ctx_shared, port, monkeypatch, capfd, dt):
    """OSP_SPLIT_FROM_B=2: the same split from B, queued in merge_panel where the split of records runs (the A/B switch for
    the move beside the plan)."""
    ops, halves, stretch = _two_panel_operands(6)
    info = three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 2, stretch, from_b="2", partial_capacity=max(halves) + 10)
    assert info["panels"] == 2 and info["plans_overlapped"] == 1 and info["expand_partials"] == 4000, info


@pytest.mark.parametrize("dt", DTYPES)
def test_duplicate_columns_across_chunks(_ctx_shared, port, monkeypatch, capfd, dt):
    """Every chunk holds the same 100 columns: each output entry is the sum of 75 products, in ascending k."""
    ops = Operands(7)
    cols = np.sort(ops.rng.choice(N, 100, replace=False))
    ops.a_rows.append([ops.b_row(100, cols) for _ in range(75)])
    ops.a_row([4])
    info = three_ways(_ctx_shared, port, monkeypatch, capfd, ops, dt, 1, 7500)
    assert info["nnz_c"] == 104


def test_hub_rows_keep_their_path(_ctx_shared, port, monkeypatch, capfd):
    """With the soak's switches the rows beyond the planner are hub rows, written through cells by the multiply: nothing
    of them is split, from B or otherwise."""
    ops = Operands(8)
    ops.a_row([100] * 70)
    M, K, a, b = ops.coo()
    _ctx_shared.algorithm = "outer"
    for k, v in dict(FORCE, OSP_HUB_MIN_SHARE="0", OSP_HUB_MIN_RUN="0", OSP_VERBOSE="1").items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    got, want = run_both(_ctx_shared, port, M, K, N, a, b, np.float64)
    assert_same(got, want)
    assert got.info["hub_rows"] == 1 and not stretch_lines(capfd.readouterr().err)
    got.close()


_POOL_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OSP_TEST_ROOT"])
from outerspace_amd import spgemm as S
from oracle import oracle   # checker only
from tests.ieee_model import assert_same_bits
from tests.test_gpu_split_from_b import N, _two_panel_operands
port = oracle.port()
ops, halves, stretch = _two_panel_operands(6)
M, K, a, b = ops.coo()
acsc, bcsr = S.coo_to_csc(K, *a), S.coo_to_csr(K, *b)
want = port.spgemm(M, K, N, *acsc, *bcsr)
with S.Context(0) as ctx:
    for rep in range(3):
        got = ctx.spgemm_csc_csr(M, K, N, *acsc, *bcsr, partial_capacity=max(halves) + 10)
        assert got.info["panels"] == 2 and got.info["plans_overlapped"] == 1 and got.info["expand_partials"] == 4000, got.info
        assert np.array_equal(got.rowptr, want["rowptr"]) and np.array_equal(got.colidx, want["colidx"])
        assert_same_bits(got.vals, want["vals"])
        got.close()
print("SPLIT_FROM_B_OK")
"""


@pytest.mark.parametrize("mode", ["OSP_POISON", "OSP_GUARD"])
def test_two_panels_under_poison_and_guard(mode, port):
    """The split of panel p runs between the fork of the second stream and the plan of panel p+1, where nothing may be taken
    from or given back to the pool (osp_context.h, Context::fork_window).  The two-panel product in a process of its own with
    every pooled buffer poisoned on allocation, or with guard zones around every buffer: bit-identical to the oracle."""
    env = dict(os.environ, OSP_TEST_ROOT=ROOT, OSP_PLAN_OVERLAP="1", OSP_HUB="0", **FORCE)
    env.pop("OSP_SPLIT_FROM_B", None)
    env[mode] = "1"
    r = subprocess.run([sys.executable, "-c", _POOL_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SPLIT_FROM_B_OK" in r.stdout, r.stdout + r.stderr
