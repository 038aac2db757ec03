"""The chains of tests/result_chain.py on the GPU: in this process on the session's context, then in a fresh child process
with every pool buffer poisoned on allocation (OSP_POISON=1: a read of scratch nobody wrote gives the same wrong bits every
time) and in one with guard zones around every buffer, checked at release (OSP_GUARD=1: a write one word past ``nwords``,
``M + 1`` or ``nnz``, which bucket rounding otherwise hides, is named).  Both modes are read once per process, hence the
children; one child runs at a time.  The tests run in this order.  Only a mismatch (an AssertionError here, exit status 1
of a child) or missing coverage (status 2) lets the next test start: a device or runtime error in this process, a child that
reports one (status rc.DEVICE_ERROR_STATUS), dies (abort() is 134 or -6) or hangs stops everything after it.

Replay one seed with ``python -m tests.result_chain --seeds 7``."""
import os
import re
import subprocess
import sys
import time

import pytest
import torch

from tests import result_chain as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# A hang guard, not a performance assertion: the in-process test takes IN_PROCESS_S on an MI355X (MEASUREMENTS.md
# section 0m), and a child -- which also starts Python, loads the library and creates a context -- gets sixty times that
# (a child took 4.6 s under OSP_POISON and 5.0 s under OSP_GUARD; the in-process run 1.9 s).
IN_PROCESS_S = 2
CHILD_TIMEOUT_S = 120
assert CHILD_TIMEOUT_S >= 10 * IN_PROCESS_S
_state = {"steps": None, "stop": None}


@pytest.fixture(scope="module")
def mctx(_ctx_shared):
    yield _ctx_shared
    if not _state["stop"]:                          # (after a device error nothing more runs on the GPU, not even this)
        _ctx_shared.trim()
        torch.cuda.empty_cache()


def test_chains_on_the_shared_context(mctx):
    t0 = time.perf_counter()
    try:
        cov = rc.run_seeds(rc.GpuBackend(mctx))
    except rc.ChainMismatch:                        # a comparison that differs, or a call the library refused: the device is well
        raise
    except BaseException as e:                      # (OspError(ERR_HIP), an error of torch, ...: maybe a GPU fault)
        _state["stop"] = f"the in-process run ended with {type(e).__name__}"
        raise
    print(f"in-process: {cov.steps} steps in {time.perf_counter() - t0:.1f} s")
    print(cov.matrix())
    assert cov.missing() == [] and cov.skipped == 0
    _state["steps"] = cov.steps


def _child(mode):
    if _state["stop"]:
        pytest.skip(f"{_state['stop']}: nothing further is started on the GPU")
    env = dict(os.environ, OSP_DIRECT_MIN_NNZ="0")
    env[mode] = "1"
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.result_chain"], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _state["stop"] = f"the child under {mode} hung"
        raise
    print(f"child under {mode}=1: exit {r.returncode} after {time.perf_counter() - t0:.1f} s")
    # 1: a mismatch, 2: coverage.  Anything else stops the module: DEVICE_ERROR_STATUS is a device or runtime error that
    # the child caught, and a child that died has abort()'s 134 or -6, or a signal's
    assert rc.DEVICE_ERROR_STATUS not in (0, 1, 2)
    if r.returncode not in (0, 1, 2):
        _state["stop"] = f"the child under {mode} ended with status {r.returncode}"
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CHAIN_OK")]
    assert len(line) == 1, r.stdout[-4000:]
    steps = int(re.search(r"steps=(\d+)", line[0]).group(1))
    assert "skipped=0" in line[0] and steps == (_state["steps"] if _state["steps"] is not None else steps)
    assert _state["steps"] is not None, "the in-process run did not finish: no step count to compare with"
    return r


def test_chains_in_a_child_under_poison():
    _child("OSP_POISON")


def test_chains_in_a_child_under_guard():
    r = _child("OSP_GUARD")
    assert "[osp] OSP_GUARD:" not in r.stderr, r.stderr[-4000:]
