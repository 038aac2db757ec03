"""The environment's settings are read per call (outerspace_amd/csrc/osp_settings.h, Context::env): ONE context, one process,
the environment changed between calls, in each kind of frame -- a product, a result made from a result, a vector made from a
result.  What the settings mean is the business of the tests that set them; tests/test_settings_cpu.py checks the parsing."""
import numpy as np
import pytest

from tests import mxv_model
from tests import test_gpu_apply_mask as am   # the input builders only

pytestmark = pytest.mark.gpu


def test_every_call_reads_the_environment_anew(_ctx_shared, monkeypatch, capfd):
    ctx = _ctx_shared
    for name in ("OSP_VERBOSE", "OSP_TRANSPOSE_PATH", "OSP_MXV_GROUP"):
        monkeypatch.delenv(name, raising=False)
    ncol = 300
    csr = rowptr, col, val = am._csr_from_lengths([3, 0, 5, 4], ncol, np.float64, seed=7)

    # ---- a product: X^T X, verbose on the second call only ----
    def product():
        capfd.readouterr()
        res = ctx.spgemm_csc_csr(ncol, 4, ncol, rowptr, col, val, rowptr, col, val)
        try:
            return (res.rowptr.copy(), res.colidx.copy(), am._bits(res.vals).copy()), capfd.readouterr().err
        finally:
            res.close()

    quiet, err0 = product()
    monkeypatch.setenv("OSP_VERBOSE", "1")
    loud, err1 = product()
    monkeypatch.delenv("OSP_VERBOSE")
    again, err2 = product()
    assert "[osp]" not in err0 and "[osp]" not in err2, (err0, err2)
    assert "[osp] spgemm M=300 K=4 N=300" in err1 and "[osp] product done" in err1, err1
    assert len(quiet[1]) > 0
    for a, b in zip(quiet, loud):
        assert np.array_equal(a, b)
    for a, b in zip(quiet, again):
        assert np.array_equal(a, b)

    src = am._upload(ctx, ncol, csr)
    try:
        # ---- result to result: four rows take the row mask unless the sort is asked for ----
        def path():
            res, st = src.transpose()
            res.close()
            return st["path"]

        assert path() == 1
        monkeypatch.setenv("OSP_TRANSPOSE_PATH", "sort")
        assert path() == 2
        monkeypatch.delenv("OSP_TRANSPOSE_PATH")
        assert path() == 1

        # ---- result to vector ----
        x = np.random.default_rng(8).standard_normal(ncol)

        def group():
            return src.mxv(x, "plus", "times", space="host")[1]["group"]

        auto = group()
        assert auto in mxv_model.GROUPS
        monkeypatch.setenv("OSP_MXV_GROUP", "4")
        assert group() == 4
        monkeypatch.setenv("OSP_MXV_GROUP", "64")
        assert group() == 64
        monkeypatch.delenv("OSP_MXV_GROUP")
        assert group() == auto
    finally:
        src.close()
