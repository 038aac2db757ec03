"""bench.py as the driver runs it: the plain line (the headline and nothing else), --dump-outputs against the oracle, --full.
The GPU runs are small products in child processes, each under a time limit."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(*args, timeout=600):
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_refuses_bad_step_counts_and_dumps_of_several_gpus():
    for args in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "x"]):
        r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "error:" in r.stderr, (args, r.stderr)


def _operands(scale, dt):
    import torch
    spec = importlib.util.spec_from_file_location("osp_bench", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    from outerspace_amd import generators as gen
    tdt = torch.float64 if dt == np.float64 else torch.float32
    n, csr, csc = m.rmat_device(scale, 16, gen.RMAT_PRESETS["mild"], 1, torch.device("cuda", 0), tdt)
    host = [t.cpu().numpy() for t in (*csc, *csr)]
    return n, [a.view(np.uint32) if a.dtype == np.int32 else a for a in host]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plain_run_and_its_outputs(tmp_path, port, dtype):
    """The plain line holds the headline (value = nnz(C) per second of one step, ms_per_step over exactly --steps steps) and
    none of what --full adds; the dumped sample of C equals the oracle's product of the same seeded operands bit for bit,
    and a streamed run dumps the same arrays."""
    dt = np.float64 if dtype == "f64" else np.float32
    d = run_bench("--gpus", "1", "--scale", "12", "--steps", "3", "--warmup", "1", "--dtype", dtype, "--dump-outputs", str(tmp_path / "a"))
    assert d["metric"] == "spgemm_output_nnz_per_s" and d["unit"] == "nnz/s" and d["higher_is_better"] is True
    assert d["dtype"] == dtype and d["steps"] == 3 and len(d["steps_ms"]["total"]) == 3
    assert d["value"] == pytest.approx(d["config"]["nnz_c"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "result_check", "cpu_baseline", "ingest", "cost_model", "extra_workloads"):
        assert k not in d, k
    n, host = _operands(12, dt)
    want = port.spgemm(n, n, n, *host)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["C_sample_cols", "C_sample_row_nnz", "C_sample_rows", "C_sample_vals", "C_summary"]
    assert got["C_sample_vals"].dtype == dt and all(a.dtype == np.float64 for k, a in got.items() if k != "C_sample_vals")
    rows = got["C_sample_rows"].astype(np.int64)
    assert len(rows) == n and np.array_equal(rows, np.arange(n))   # n = 4096 < 2^20: every row, in order
    rp = want["rowptr"]
    assert np.array_equal(got["C_sample_row_nnz"], np.diff(rp)) and d["config"]["nnz_c"] == rp[-1]
    for i in np.flatnonzero(got["C_sample_row_nnz"]):
        j = rp[i] + np.searchsorted(want["colidx"][rp[i]:rp[i + 1]], got["C_sample_cols"][i])
        assert want["colidx"][j] == got["C_sample_cols"][i] and want["vals"][j] == got["C_sample_vals"][i]
    assert np.all(got["C_sample_cols"][got["C_sample_row_nnz"] == 0] == -1)
    s = got["C_summary"]
    assert s[:3].tolist() == [n, n, rp[-1]] and s[3] == pytest.approx(want["vals"].sum(dtype=np.float64), rel=1e-9)
    run_bench("--gpus", "1", "--scale", "12", "--steps", "2", "--warmup", "0", "--dtype", dtype, "--stream-output",
              "--dump-outputs", str(tmp_path / "b"))
    for k, a in got.items():
        b = np.load(tmp_path / "b" / f"{k}.npy")
        if k == "C_summary":   # the value sum adds panel by panel
            assert np.array_equal(a[:3], b[:3]) and b[3] == pytest.approx(a[3], rel=1e-9)
        else:
            assert np.array_equal(a, b), k


@pytest.mark.gpu
def test_full_run_adds_the_checks(tmp_path):
    """--full still measures and checks what it did before it was an option (the secondary workloads belong to the default
    size only): whole-result check, roofline, CPU baseline and both parities, ingest, cost model."""
    d = run_bench("--gpus", "1", "--scale", "14", "--steps", "2", "--warmup", "1", "--full", "--cpu-partials", "1e6")
    assert d["steps"] == 2 and d["roofline"]["bound"] == "hbm" and d["roofline"]["peak_measured"] > 0
    assert d["result_check"]["rel_err"] < 1e-9 and d["whole_product"]["frac_of_measured"] > 0
    assert d["slab_parity"]["status"] == "ok" and d["row_slab_parity"]["status"] == "ok" and d["cpu_baseline"]["value"] > 0
    assert "device_coo_to_compressed" in d["ingest"] and "cost_model" in d
