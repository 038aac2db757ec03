"""What tests/test_gpu_scan.py, tests/test_gpu_draw.py and their child processes share: the operand family of the sweeps
(the k-select's family, whose builders are imported, plus rows at the edges of the scan's blocks), and a fixed slice of both
sweeps whose outputs are hashed.  A helper, not a test file.

``python -m tests.scan_cases`` runs the slice on a context of its own and prints ``SCAN_SLICE <sha256> calls=<n>``
(``python -m tests.scan_cases draw``: the draws' own slice, ``DRAW_SLICE ...``): the tests
start it under OSP_POISON=1 and under OSP_GUARD=1 (both are read once per process) and compare the digest with the one of
their own process.  Any exception ends the child at once with DEVICE_ERROR_STATUS: it starts nothing more on the GPU."""
import hashlib
import os
import sys
import traceback

import numpy as np

from tests import kron_cases as kc
from tests import scan_model as model
from tests import select_k_cases as skc

ROOT = kc.ROOT
DEVICE_ERROR_STATUS = 3
DRAWS = (1, 2, 7, 64)

csr_of = kc.csr_of             # random values, every seventh entry a special one
build = kc.build               # Context.build(dup="error"): the three arrays come back bit for bit
random_rows = skc.random_rows

B = model.BLOCK
# one and two blocks; 16 and 17 blocks (the chain's lane and wave paths); 64 blocks, one load of the chain's wave path, and two
BLOCK_EDGES = [0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 16 * B - 1, 16 * B, 16 * B + 1, 17 * B, 17 * B + 1,
               64 * B - 1, 64 * B, 64 * B + 1, 128 * B - 1, 128 * B, 128 * B + 1]


def positive(csr, seed):
    """The same pattern with positive finite values of many magnitudes, a fifth of them zero: a clean CDF."""
    rowptr, col, val = csr
    rng = np.random.default_rng(seed)
    v = np.ldexp(rng.random(len(col)) + 0.5, rng.integers(-20, 20, len(col))).astype(val.dtype)
    v[rng.random(len(col)) < 0.2] = 0
    return rowptr, col, v


def family(dt):
    """name -> ((rowptr, col, val), columns)."""
    fam = dict(skc.family(dt))
    ncol = 130 * B
    fam["edges"] = (csr_of(random_rows(BLOCK_EDGES, ncol, 12), dt, 13), ncol)
    fam["edges positive"] = (positive(fam["edges"][0], 14), ncol)
    fam["ragged positive"] = (positive(fam["ragged"][0], 15), fam["ragged"][1])
    return fam


# the slice that the children repeat: both dtypes, every op, rows of one block, of a few and of many, the no-work paths
SLICE = ["ragged", "edges", "edges positive", "long", "column", "empty"]
SLICE_DRAWS = (1, 7)


def slice_digest(ctx):
    """sha256 over the outputs of every scan and draw of the slice, and the number of calls."""
    h = hashlib.sha256()
    calls = 0
    for dt in (np.float32, np.float64):
        fam = family(dt)
        made = {name: build(ctx, *fam[name]) for name in SLICE}
        try:
            for name in SLICE:
                for op in model.OPS:
                    res, st = made[name].scan(op)
                    try:
                        for x in res.to_host():
                            h.update(np.ascontiguousarray(x).tobytes())
                        h.update(repr((res.shape, res.nnz, st["blocks"], st["launches"], st["readbacks"])).encode())
                    finally:
                        res.close()
                    calls += 1
                for s in SLICE_DRAWS:
                    cols, pos, st = made[name].draw(s, seed=calls, positions=True, space="host")
                    h.update(cols.tobytes())
                    h.update(pos.tobytes())
                    h.update(repr((cols.shape, st["rows_without"], st["launches"], st["readbacks"])).encode())
                    calls += 1
        finally:
            for x in made.values():
                x.close()
    return h.hexdigest(), calls


DRAW_SLICE = ["ragged", "ragged positive", "edges positive", "long", "column", "empty"]
DRAW_SLICE_DRAWS = (1, 2, 64)


def draw_slice_digest(ctx):
    """sha256 over the outputs of every draw of the draws' own slice (with and without positions, host and device outputs),
    and the number of calls."""
    h = hashlib.sha256()
    calls = 0
    for dt in (np.float32, np.float64):
        fam = family(dt)
        made = {name: build(ctx, *fam[name]) for name in DRAW_SLICE}
        try:
            for name in DRAW_SLICE:
                for s in DRAW_SLICE_DRAWS:
                    cols, pos, st = made[name].draw(s, seed=calls, positions=True, space="host")
                    only, st2 = made[name].draw(s, seed=calls)
                    for x in (cols, pos, only.cpu().numpy()):
                        h.update(np.ascontiguousarray(x).tobytes())
                    h.update(repr((cols.shape, st["rows_without"], st["launches"], st["readbacks"], st2["rows_without"])).encode())
                    calls += 2
        finally:
            for x in made.values():
                x.close()
    return h.hexdigest(), calls


def main():
    draws = sys.argv[1:] == ["draw"]
    try:
        from outerspace_amd import spgemm as S
        ctx = S.Context(0)
        digest, calls = draw_slice_digest(ctx) if draws else slice_digest(ctx)
        ctx.close()
    except BaseException:   # a device or runtime error, or anything else: nothing further is started on the GPU
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(DEVICE_ERROR_STATUS)
    print(f"{'DRAW' if draws else 'SCAN'}_SLICE {digest} calls={calls}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
