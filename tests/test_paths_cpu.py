"""Which formulation a product runs (outerspace_amd/csrc/osp_paths.h): the decisions for a table of inputs, plain and under
AddressSanitizer + UBSan.  tests/paths_driver.cpp prints what the header decides; every case runs it in a child process of
its own.  The expected table was written out by hand from the nine booleans spgemm_impl held before the header existed
(rowwise, direct, dense_avg, gather_ok, gather_short, table, with_av, expand_rows_on, partials_only), not from the header."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "paths_driver.cpp")

OUTER, ROWWISE = 0, 1
SPLIT_ROW_MAX = 256 << 9        # osp_split.h: kSplitTarget << kSplitRowBits
DIRECT_DENSE_MAX = 1 << 20      # osp_split.h: kDirectDenseMax
MIN_NNZ = 2 << 20               # OSP_DIRECT_MIN_NNZ's default ...
MIN_NNZ_G0 = 8 << 20            # ... and with OSP_GATHER=0
BIG = 3_000_000                 # non-zeros above the first default, below the second
SIDE = 1_000_000                # M = N of the sparse cases: 8 p_all is far below 3 M N
P_SPARSE = 10_000_000

# the decisions as (rowwise, direct, gather_long, gather_short, av_ride_along, keep_table, expand_rows)
NONE = (False, False, False, False, False, False, False)
SPLIT = NONE                                               # outer products, every long row split after the multiply
ALL = (False, True, True, True, True, True, True)          # direct rows, long and short rows gathered, rows expanded
LONG_ONLY = (False, True, True, False, True, True, False)  # direct rows, long rows gathered
WRITTEN = (False, True, False, False, False, True, False)  # direct rows written by the multiply
RW_DIRECT = (True, True, False, False, False, True, False)
RW_SPLIT = (True, False, False, False, False, True, False)


def _dense_threshold(m, n):
    """the smallest p_all with 8 p_all >= 3 M N"""
    return -(-3 * m * n // 8)


M33 = 2**32 - 2   # 3 M N = 3 * 2^64 - ...: beyond 64 bits, and no multiple of 8 -- the threshold lies between two integers
M34 = 2**32 - 4   # 3 M N beyond 64 bits and a multiple of 8: equality exists
assert 3 * M33 * M33 > 2**64 and (3 * M33 * M33) % 8 != 0
assert 3 * M34 * M34 > 2**64 and (3 * M34 * M34) % 8 == 0 and 8 * _dense_threshold(M34, M34) == 3 * M34 * M34

# (id, environment, algorithm, nnz, p_all, M, N, partials_only, decisions, direct_max, direct_min_nnz)
CASES = [
    ("outer", {}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, ALL, SPLIT_ROW_MAX, MIN_NNZ),
    ("rowwise", {}, ROWWISE, BIG, P_SPARSE, SIDE, SIDE, 0, RW_DIRECT, SPLIT_ROW_MAX, MIN_NNZ),
    ("rowwise_small", {}, ROWWISE, 1000, P_SPARSE, SIDE, SIDE, 0, RW_SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("direct_off", {"OSP_DIRECT": "0"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("direct_off_rowwise", {"OSP_DIRECT": "0"}, ROWWISE, BIG, P_SPARSE, SIDE, SIDE, 0, RW_SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("gather0_below_its_min", {"OSP_GATHER": "0"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ_G0),
    ("gather0", {"OSP_GATHER": "0"}, OUTER, 9_000_000, P_SPARSE, SIDE, SIDE, 0, WRITTEN, SPLIT_ROW_MAX, MIN_NNZ_G0),
    ("gather1", {"OSP_GATHER": "1"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, LONG_ONLY, SPLIT_ROW_MAX, MIN_NNZ),
    ("gather2", {"OSP_GATHER": "2"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, ALL, SPLIT_ROW_MAX, MIN_NNZ),
    ("gather2_direct_off", {"OSP_GATHER": "2", "OSP_DIRECT": "0"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    # nnz just below and at direct_min_nnz: both defaults, and OSP_DIRECT_MIN_NNZ=0
    ("below_min", {}, OUTER, MIN_NNZ - 1, P_SPARSE, SIDE, SIDE, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("at_min", {}, OUTER, MIN_NNZ, P_SPARSE, SIDE, SIDE, 0, ALL, SPLIT_ROW_MAX, MIN_NNZ),
    ("gather0_below_min", {"OSP_GATHER": "0"}, OUTER, MIN_NNZ_G0 - 1, P_SPARSE, SIDE, SIDE, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ_G0),
    ("gather0_at_min", {"OSP_GATHER": "0"}, OUTER, MIN_NNZ_G0, P_SPARSE, SIDE, SIDE, 0, WRITTEN, SPLIT_ROW_MAX, MIN_NNZ_G0),
    ("min0", {"OSP_DIRECT_MIN_NNZ": "0"}, OUTER, 1, 1, SIDE, SIDE, 0, ALL, SPLIT_ROW_MAX, 0),
    ("min0_gather0", {"OSP_DIRECT_MIN_NNZ": "0", "OSP_GATHER": "0"}, OUTER, 1, 1, SIDE, SIDE, 0, WRITTEN, SPLIT_ROW_MAX, 0),
    ("min_set_below", {"OSP_DIRECT_MIN_NNZ": "5000"}, OUTER, 4999, 1, SIDE, SIDE, 0, SPLIT, SPLIT_ROW_MAX, 5000),
    ("min_set_at", {"OSP_DIRECT_MIN_NNZ": "5000", "OSP_GATHER": "0"}, OUTER, 5000, 1, SIDE, SIDE, 0, WRITTEN, SPLIT_ROW_MAX, 5000),
    # dense on average: 8 p_all >= 3 M N plans direct rows whatever nnz is
    ("dense_equal", {}, OUTER, 1, _dense_threshold(M34, M34), M34, M34, 0, ALL, SPLIT_ROW_MAX, MIN_NNZ),
    ("dense_one_below", {}, OUTER, 1, _dense_threshold(M34, M34) - 1, M34, M34, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("dense_over_2_64", {}, OUTER, 1, _dense_threshold(M33, M33), M33, M33, 0, ALL, SPLIT_ROW_MAX, MIN_NNZ),
    ("dense_over_2_64_one_below", {}, OUTER, 1, _dense_threshold(M33, M33) - 1, M33, M33, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("dense_small", {}, OUTER, 100, 6, 4, 4, 0, ALL, SPLIT_ROW_MAX, MIN_NNZ),
    ("dense_small_one_below", {}, OUTER, 100, 5, 4, 4, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    ("dense_direct_off", {"OSP_DIRECT": "0"}, OUTER, 100, 6, 4, 4, 0, SPLIT, SPLIT_ROW_MAX, MIN_NNZ),
    # OSP_DIRECT_MAX: capped at the planner's 21-bit count
    ("direct_max_above_cap", {"OSP_DIRECT_MAX": str(4 << 20)}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, ALL, DIRECT_DENSE_MAX, MIN_NNZ),
    ("direct_max_garbage", {"OSP_DIRECT_MAX": "-1"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, ALL, DIRECT_DENSE_MAX, MIN_NNZ),
    ("direct_max_below_cap", {"OSP_DIRECT_MAX": "1000"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, ALL, 1000, MIN_NNZ),
    # the multiply phase alone, and a shard without non-zeros: nothing is chosen
    ("partials_only", {"OSP_DIRECT_MIN_NNZ": "0"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 1, NONE, SPLIT_ROW_MAX, 0),
    ("partials_only_rowwise", {}, ROWWISE, BIG, P_SPARSE, SIDE, SIDE, 1, NONE, SPLIT_ROW_MAX, MIN_NNZ),
    ("partials_only_dense", {}, OUTER, 100, 6, 4, 4, 1, NONE, SPLIT_ROW_MAX, MIN_NNZ),
    ("nnz0", {"OSP_DIRECT_MIN_NNZ": "0"}, OUTER, 0, 0, SIDE, SIDE, 0, NONE, SPLIT_ROW_MAX, 0),
    ("nnz0_rowwise_dense", {}, ROWWISE, 0, 6, 4, 4, 0, NONE, SPLIT_ROW_MAX, MIN_NNZ),
    ("nnz0_empty_result", {}, OUTER, 0, 0, 0, 0, 0, NONE, SPLIT_ROW_MAX, MIN_NNZ),
    ("expand_rows_off", {"OSP_EXPAND_ROWS": "0"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, ALL[:6] + (False,), SPLIT_ROW_MAX, MIN_NNZ),
    ("expand_rows_gather1", {"OSP_EXPAND_ROWS": "1", "OSP_GATHER": "1"}, OUTER, BIG, P_SPARSE, SIDE, SIDE, 0, LONG_ONLY, SPLIT_ROW_MAX, MIN_NNZ),
]
KEYS = ("rowwise", "direct", "gather_long", "gather_short", "av_ride_along", "keep_table", "expand_rows")


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, DRIVER], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "paths_driver", ["-O1"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "paths_driver_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                          "-fno-omit-frame-pointer"])


def _decide(exe, case):
    _, env_vars, algo, nnz, p_all, m, n, partials_only = case[:8]
    env = {k: v for k, v in os.environ.items() if not k.startswith("OSP_")}
    env.update(env_vars)
    args = [str(v) for v in (algo, nnz, p_all, m, n, partials_only, SPLIT_ROW_MAX, DIRECT_DENSE_MAX)]
    r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout)


def _expected(case):
    want = dict(zip(KEYS, case[8]))
    want["direct_max"], want["direct_min_nnz"] = case[9], case[10]
    return want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decisions(driver, case):
    assert _decide(driver, case) == _expected(case)


def test_decisions_under_sanitizers(driver_san):
    """The same driver as a stand-alone program under AddressSanitizer + UBSan, every case."""
    for case in CASES:
        assert _decide(driver_san, case) == _expected(case), case[0]


def test_header_is_plain_cpp():
    """No HIP in the header, and nothing of the library but the settings and the public C header."""
    text = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_paths.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<algorithm>", "<cstdint>", '"../../include/outerspace_spgemm.h"', '"osp_settings.h"']
