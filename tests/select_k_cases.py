"""What tests/test_gpu_select_k.py and its child processes share: the operand family of the sweep (random values, every
seventh entry one of ``test_gpu_apply_mask._special``), uploaded through ``Context.build(dup="error")``, and a fixed slice of
the sweep whose outputs are hashed.  A helper, not a test file.

``python -m tests.select_k_cases`` runs the slice on a context of its own and prints ``SELECT_K_SLICE <sha256> calls=<n>``:
the test starts it under OSP_POISON=1 and under OSP_GUARD=1 (both are read once per process) and compares the digest with
the one of its own process.  Any exception ends the child at once with DEVICE_ERROR_STATUS: it starts nothing more on the
GPU."""
import hashlib
import os
import sys
import traceback

import numpy as np

from tests import kron_cases as kc
from tests import select_k_model as model

ROOT = kc.ROOT
DEVICE_ERROR_STATUS = 3
KS = (1, 2, 7, 64, (1 << 32) - 1)
LONG_MIN = model.LONG_MIN

csr_of = kc.csr_of     # random values, every seventh entry a special one
build = kc.build       # Context.build(dup="error"): the three arrays come back bit for bit


def random_rows(lengths, ncol, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(ncol, int(m), replace=False)) for m in lengths]


def with_ties(csr, seed, distinct=3):
    """The same pattern with values from a handful of numbers: most ranks are decided by the column."""
    rowptr, col, val = csr
    rng = np.random.default_rng(seed)
    pool = np.array([2.5, -1.0, 0.0, -0.0, 7.0, np.inf][:max(distinct, 1)], val.dtype)
    return rowptr, col, pool[rng.integers(0, len(pool), len(col))]


RAGGED = [0, 1, 0, 0, 2, 3, 0, 1, 0, 7, 8, 9, 63, 64, 65, 70, 130, 0, 257]


def family(dt):
    """name -> ((rowptr, col, val), columns): rows below, at and above every k of the sweep, in both classes."""
    ragged = random_rows(RAGGED, 300, 5)
    long_rows = random_rows([LONG_MIN + 1, 3, LONG_MIN, 0, 2 * LONG_MIN + 77], 3 * LONG_MIN, 6)
    return {"one": (csr_of([[0]], dt, 1), 1),
            "row": (csr_of([np.arange(70)], dt, 2), 70),
            "column": (csr_of([[0] if i % 2 == 0 else [] for i in range(70)], dt, 3), 1),
            "ragged": (csr_of(ragged, dt, 4), 300),
            "dense": (csr_of([np.arange(7)] * 5, dt, 5), 7),
            "empty": (csr_of([[]] * 4, dt, 6), 6),
            "ties": (with_ties(csr_of(ragged, dt, 7), 8), 300),
            "long": (csr_of(long_rows, dt, 9), 3 * LONG_MIN),
            "long ties": (with_ties(csr_of(long_rows, dt, 10), 11, 2), 3 * LONG_MIN)}


# the slice that the children repeat: every order and both dtypes, rows of both classes, ties, the no-work paths
SLICE = ["ragged", "ties", "long", "long ties", "column", "empty"]
SLICE_KS = (1, 7, 64, (1 << 32) - 1)


def slice_digest(ctx):
    """sha256 over the three arrays of every select of the slice, and the number of selects."""
    h = hashlib.sha256()
    calls = 0
    for dt in (np.float32, np.float64):
        fam = family(dt)
        made = {name: build(ctx, *fam[name]) for name in SLICE}
        try:
            for name in SLICE:
                for order in model.ORDERS:
                    for k in SLICE_KS:
                        res, st = made[name].select_k(k, order, seed=calls)
                        try:
                            for x in res.to_host():
                                h.update(np.ascontiguousarray(x).tobytes())
                            h.update(repr((res.shape, res.nnz, st["rows_capped"], st["rows_long"], st["launches"], st["readbacks"])).encode())
                        finally:
                            res.close()
                        calls += 1
        finally:
            for x in made.values():
                x.close()
    return h.hexdigest(), calls


def main():
    try:
        from outerspace_amd import spgemm as S
        ctx = S.Context(0)
        digest, calls = slice_digest(ctx)
        ctx.close()
    except BaseException:   # a device or runtime error, or anything else: nothing further is started on the GPU
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(DEVICE_ERROR_STATUS)
    print(f"SELECT_K_SLICE {digest} calls={calls}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
