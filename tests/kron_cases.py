"""What tests/test_gpu_kron.py and its child processes share: the operand family of the sweep, the upload of a CSR through
``Context.build``, and a fixed slice of the sweep whose outputs are hashed.  A helper, not a test file.

``python -m tests.kron_cases`` runs the slice on a context of its own and prints ``KRON_SLICE <sha256> calls=<n>``: the test
starts it under OSP_POISON=1 and under OSP_GUARD=1 (both are read once per process) and compares the digest with the one of
its own process.  Any exception ends the child at once with DEVICE_ERROR_STATUS: it starts nothing more on the GPU."""
import hashlib
import os
import re
import sys
import traceback

import numpy as np

from tests import kron_model as model
from tests import test_gpu_apply_mask as am   # the special values only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "outerspace_amd", "csrc", "osp_kron.h")).read()
# the output positions one workgroup of the entries kernel takes
CHUNK = int(re.search(r"kKronThreads\s*=\s*(\d+)", _SRC).group(1)) * int(re.search(r"kKronEntries\s*=\s*(\d+)", _SRC).group(1))
DEVICE_ERROR_STATUS = 3


special = am._special   # NaNs with payloads, infinities, both zeros, denormals, the largest number and 1


def csr_of(lists, dt, seed):
    """A CSR from one ascending column array per row: random values, every seventh entry a special one."""
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(dt)
    sp = special(dt)
    val[::7] = np.resize(np.roll(sp, seed), len(val[::7]))
    return rowptr, col, val


RAGGED = [0, 1, 0, 0, 2, 3, 0, 1, 0]


def family(dt):
    """name -> ((rowptr, col, val), columns): the operands of the sweep, on either side."""
    rng = np.random.default_rng(5)
    ragged = [np.sort(rng.choice(11, k, replace=False)) for k in RAGGED]
    return {"one": (csr_of([[0]], dt, 1), 1),
            "row": (csr_of([np.arange(70)], dt, 2), 70),
            "column": (csr_of([[0] if i % 2 == 0 else [] for i in range(70)], dt, 3), 1),
            "ragged": (csr_of(ragged, dt, 4), 11),
            "dense": (csr_of([np.arange(7)] * 5, dt, 5), 7),
            "empty": (csr_of([[]] * 4, dt, 6), 6)}


def build(ctx, csr, ncol, dt=None):
    """The CSR as a library result through ``Context.build(dup="error")``; its three arrays come back bit for bit."""
    rowptr, col, val = csr
    dt = val.dtype.type if dt is None else dt
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.uint32), np.diff(rowptr))
    res = ctx.build(len(rowptr) - 1, ncol, rows, col, val, dup="error", dtype=dt, space="host")[0]
    return res


# the slice of the sweep that the children repeat: every operator and both dtypes on pairs that cross chunk edges inside a
# row (row x row), walk runs of empty rows (ragged, column) and take the no-work path (empty)
SLICE = [("ragged", "ragged"), ("row", "row"), ("column", "ragged"), ("ragged", "column"), ("dense", "row"), ("one", "ragged"),
         ("empty", "dense"), ("dense", "empty")]


def slice_digest(ctx):
    """sha256 over the three arrays of every product of the slice, and the number of products."""
    h = hashlib.sha256()
    calls = 0
    for dt in (np.float32, np.float64):
        fam = family(dt)
        made = {name: build(ctx, csr, ncol) for name, (csr, ncol) in fam.items()}
        try:
            for an, bn in SLICE:
                for op in model.OPS:
                    res, st = made[an].kron(made[bn], op)
                    try:
                        for x in res.to_host():
                            h.update(np.ascontiguousarray(x).tobytes())
                        h.update(repr((res.shape, res.nnz, st["launches"], st["readbacks"])).encode())
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
    print(f"KRON_SLICE {digest} calls={calls}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
