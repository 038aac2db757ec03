"""Regression test for round 1's intermittent GPU memory fault.

The persistent merge kernel hands out tiles by ticket.  A workgroup that starts late -- because the CUs are busy with
another kernel or another process -- can find every ticket taken; it then held a tile descriptor slot in LDS that was
never filled, and indexing the kernel-argument arrays with that garbage faulted.  With the GPU to itself the library
hit this perhaps once in sixty small, skewed products; beside a second process that keeps the CUs busy it failed every
time.  So this test runs products whose tile counts are close to the merge grid while a neighbour process
(tools/gpu_neighbor.py, plain torch matmuls) shares the device, and checks every result against the oracle."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from outerspace_amd import generators as gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_products_beside_a_busy_neighbour_process(ctx, port):
    from outerspace_amd import spgemm as S
    nb = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "gpu_neighbor.py"), "compute", "22"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        time.sleep(8)  # its start-up (import torch, first matmul) -- from here on the CUs are contended
        assert nb.poll() is None, nb.stdout.read().decode(errors="replace")
        n, rows, cols, vals = gen.rmat_coo(14, 16, "g500", seed=5)
        acsc = S.coo_to_csc(n, rows, cols, vals)
        bcsr = S.coo_to_csr(n, rows, cols, vals)
        cuts = [0, n // 64, n // 8, n // 2, n]
        wants = [port.spgemm(n, n, n, *acsc, *bcsr, cuts[i], cuts[i + 1]) for i in range(4)]
        t_end = time.time() + 8
        rounds = 0
        while time.time() < t_end:
            for i in range(4):  # k slabs of very different skew: few tiles to many, over-long segments in the first
                got = ctx.spgemm_csc_csr(n, n, n, *acsc, *bcsr, k_range=(cuts[i], cuts[i + 1]), validate=False)
                assert np.array_equal(got.rowptr, wants[i]["rowptr"]) and np.array_equal(got.colidx, wants[i]["colidx"])
                assert np.array_equal(got.vals, wants[i]["vals"])
                got.close()
            rounds += 1
        assert rounds >= 1
        assert nb.poll() is None, "the neighbour ended early: " + nb.stdout.read().decode(errors="replace")
    finally:
        nb.kill()
        nb.wait()


_OVERLAP_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OSP_TEST_ROOT"])
from outerspace_amd import generators as gen
from outerspace_amd import spgemm as S
from oracle import oracle   # checker only
port = oracle.port()
n, rows, cols, vals = gen.rmat_coo(13, 16, "g500", seed=9)
acsc, bcsr = S.coo_to_csc(n, rows, cols, vals), S.coo_to_csr(n, rows, cols, vals)
want = port.spgemm(n, n, n, *acsc, *bcsr)
with S.Context(0) as ctx:
    for rep in range(3):
        got = ctx.spgemm_csc_csr(n, n, n, *acsc, *bcsr, partial_capacity=150000)
        assert got.info["panels"] > 3 and got.info["plans_overlapped"] == got.info["panels"] - 1, got.info
        assert np.array_equal(got.rowptr, want["rowptr"]) and np.array_equal(got.colidx, want["colidx"]) and np.array_equal(got.vals, want["vals"])
        got.close()
print("OVERLAP_OK")
"""


@pytest.mark.parametrize("mode", ["OSP_POISON", "OSP_GUARD", "OSP_GATHER_MAX_RUNS"])
def test_plan_overlap_under_poison_and_guard(mode, port):
    """The plan of panel p+1 runs on the context's second stream beside the multiply of panel p, and the buffer pool is not
    stream-aware (osp_context.h, Context::fork_window).  Products of many panels with the plans overlapped, in a process of
    their own with every pooled buffer poisoned on allocation (OSP_POISON: a read of memory nobody wrote gives the same
    wrong bits every time) or with guard zones around every buffer, checked when it is released (OSP_GUARD): bit-identical
    to the oracle, and the library's own check that nothing is released inside the fork window stays silent."""
    env = dict(os.environ, OSP_TEST_ROOT=ROOT, OSP_DIRECT_MIN_NNZ="0", OSP_PLAN_OVERLAP="1")
    env[mode] = "1"
    if mode == "OSP_GATHER_MAX_RUNS":
        # not a checking mode but a limit (read per call, like its neighbours): panels whose run table would hold 300 descriptors or more
        # write their planned rows through the multiply's cells while the short rows stay gathered -- the fallback of a panel
        # whose run table does not fit 32-bit addressing
        env[mode] = "300"
    r = subprocess.run([sys.executable, "-c", _OVERLAP_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OVERLAP_OK" in r.stdout, r.stdout + r.stderr
