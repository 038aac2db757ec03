"""The chain driver of tests/result_chain.py without a GPU: the default seeds on the model backend pass and meet every
coverage condition, and the driver's comparison BITES -- a model backend with one planted defect fails at the step the
defect was planted in, and the report alone (its seed) reproduces it."""
import re

import numpy as np
import pytest

from tests import build_model, sddmm_model
from tests import result_chain as rc


def test_default_seeds_pass_on_the_model_backend_and_cover_every_class(capsys):
    assert rc.main(["--backend", "model"]) == 0
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith("CHAIN_OK")]
    assert len(line) == 1, out
    head = dict(re.findall(r"(seeds|steps|pairs|redraws|skipped)=(\d+)", line[0]))
    assert int(head["seeds"]) == len(rc.DEFAULT_SEEDS) >= 12 and int(head["skipped"]) == 0 and int(head["pairs"]) > 0
    assert 6 * 2 * len(rc.DEFAULT_SEEDS) <= int(head["steps"]) <= 10 * 2 * len(rc.DEFAULT_SEEDS)
    total = {}
    for dt in ("float32", "float64"):
        counts = dict(re.findall(r"([\w:]+)=(\d+)", re.search(dt + r"\[([^\]]*)\]", line[0]).group(1)))
        want = [k.split(":", 1)[1] if k.startswith("op:") else k for k in rc.Coverage.REQUIRED]
        assert sorted(counts) == sorted(want)
        assert all(int(v) >= 1 for v in counts.values()), (dt, counts)
        for k in rc.KINDS:
            total[k] = total.get(k, 0) + int(counts[k])
    assert all(v >= 5 for v in total.values()), total
    assert "input made by" in out                                    # the matrix of ordered pairs is printed


def test_the_starting_operands_hold_the_class_edges():
    for dt in rc.DTYPES:
        (_, fn, F), (_, n, A), (_, pn, P) = rc.starting_operands(rc.DEFAULT_SEEDS[0], dt)
        want = {0, 1, 63, 64, 65}
        for edge in (rc.SHORT_CAP, rc.CHUNK, rc.BLOCK):           # the library's own constants, read from its sources
            want |= {edge - 1, edge, edge + 1}
        for csr, ncol in ((F, fn), (A, n)):
            lens = np.diff(csr[0])
            assert want <= set(lens.tolist()) and lens.max() >= max(want) + 101 and lens[0] == lens[-1] == 0
            assert len(csr[1]) % 64 and len(lens) % 64 and csr[1].max() < ncol
        assert len(P[1]) % 64 and (len(P[0]) - 1) % 64 and np.diff(P[0])[0] == np.diff(P[0])[-1] == 0
        assert len(F[0]) - 1 <= rc.ROWMASK_MAX < len(A[0]) - 1 and fn == 1 << 16 and pn == n
        sp_ = rc._special(dt)
        assert all(np.any(rc._bits(A[2]) == b) for b in rc._bits(sp_)) and rc.all_nan_rows(A).any()
        assert np.all(np.isfinite(P[2])) and np.all(P[2] > 0) and np.all(np.isfinite(F[2]))
        # one row of A alone reaches the long-row class of mxm under the growth cap
        assert rc.PRODUCT_CAP > 3 * rc.SHORT_CAP


@pytest.mark.parametrize("shape", [(0, 7), (5, 0), (0, 0)])
def test_every_kind_is_drawn_and_modelled_on_a_result_without_rows_or_columns(shape):
    """The draws and the numpy models on the results that extract makes from an empty list: every kind has a legal call on
    them (with a partner that conforms), the model answers it, and what it answers has the sizes the shape gives."""
    M, N = shape
    for dt in rc.DTYPES:
        ch = rc.Chain(rc.ModelBackend(), 0, dt, rc.Coverage())
        none = lambda m: (np.zeros(m + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, dt))
        ch.live = [rc._Live(rc._Held(s, none(s[0])), s, "extract") for s in (shape, (N, M), shape)]
        for kind in rc.KINDS:
            legal = 0
            for _ in range(30):                                  # (the variants of the draw)
                ch._host = {}
                drawn = getattr(ch, "draw_" + kind)()
                if drawn is None:
                    continue
                legal += 1
                p, inputs, aux = drawn
                ins = [ch.host(L) for L in inputs]
                want = rc.expected(kind, p, ins, aux)
                got, st = ch.be.run(kind, p, [L.h for L in inputs], aux)
                assert all(st[k] == v for k, v in want["stats"].items()), (kind, p)
                if "csr" in want:
                    rowptr, col, val = want["csr"]
                    assert len(rowptr) == want["shape"][0] + 1 and not rowptr.any() and len(col) == len(val) == 0 and val.dtype == dt, (kind, p)
                    assert 0 in want["shape"] or kind in ("mxm", "matmul"), (kind, p)     # (an inner dimension of zero: a product of zeros)
                else:
                    m = ins[0][0][0]
                    vec = want["vec"] if isinstance(want["vec"], tuple) else (want["vec"],)
                    want_rows = ins[0][0][1] if kind == "reduce" and p["axis"] == "cols" else m
                    assert all(v is None or len(v) == want_rows for v in vec), (kind, p)
                    if kind == "mxv_arg":
                        assert (vec[1] == -1).all() and want["stats"]["rows_without"] == m
                    ch.same_dense(kind, p, got, want["vec"], want["nan_ok"])
            assert legal, (kind, shape)


# ---- sensitivity: one planted defect at a time ----------------------------------------------------------------------------------------
def _select_last_value_off_by_one_ulp(kind, p, out, ins, aux):
    if kind == "select" and len(out.csr[1]):
        val = out.csr[2].copy()
        rc._bits(val)[-1] += 1
        out.csr = (out.csr[0], out.csr[1], val)
        return True


def _ewise_drops_its_last_entry(kind, p, out, ins, aux):
    if kind == "ewise" and len(out.csr[1]):
        rowptr = out.csr[0].copy()
        rowptr[rowptr == rowptr[-1]] -= 1                      # (the last non-empty row and the empty rows behind it)
        out.csr = (rowptr, out.csr[1][:-1].copy(), out.csr[2][:-1].copy())
        return True


def _mxv_flips_the_sign_of_a_zero(kind, p, out, ins, aux):
    if kind == "mxv" and np.any(out == 0):
        i = int(np.flatnonzero(out == 0)[0])
        out[i] = -out[i]
        return True


def _transpose_swaps_two_entries_of_equal_column(kind, p, out, ins, aux):
    """Two entries of one column of the input are neighbours in a row of the output: an unstable sort swaps them."""
    lens = np.diff(out.csr[0]) if kind == "transpose" else np.zeros(0)
    if np.any(lens >= 2):
        b = int(out.csr[0][int(np.flatnonzero(lens >= 2)[0])])
        col, val = out.csr[1].copy(), out.csr[2].copy()
        col[[b, b + 1]], val[[b, b + 1]] = col[[b + 1, b]], val[[b + 1, b]]
        out.csr = (out.csr[0], col, val)
        return True


def _reduce_gives_the_identity_for_a_row_of_nans(kind, p, out, ins, aux):
    if kind == "reduce" and p["axis"] == "rows" and p["op"] == "plus":
        rows = np.flatnonzero(rc.all_nan_rows(ins[0][1]))
        if len(rows):
            out[rows[0]] = 0.0
            return True


def _extract_drops_the_second_copy_of_a_repeated_row(kind, p, out, ins, aux):
    rows = aux.get("rows") if kind == "extract" else None
    if rows is not None and len(np.unique(rows)) < len(rows):
        seen = set()
        i = next(i for i, r in enumerate(rows.tolist()) if r in seen or seen.add(r))     # the first index that names a row again
        rowptr, col, val = out.csr
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        out.csr = (np.concatenate([rowptr[:i + 1], rowptr[i + 2:] - (e - b)]), np.delete(col, slice(b, e)), np.delete(val, slice(b, e)))
        return True


def _build_folds_a_run_in_reverse_list_order(kind, p, out, ins, aux):
    """Under "first" and "last" the direction of the fold decides which end of a run is kept."""
    if kind == "build" and p["dup"] in ("first", "last") and "b_vals" in aux:
        (M, N), x = ins[0]
        val = build_model.build(M, N, aux["b_rows"], aux["b_cols"], aux["b_vals"], "last" if p["dup"] == "first" else "first", x[2].dtype)[0][2]
        if not np.array_equal(rc._bits(val), rc._bits(out.csr[2])):
            out.csr = (out.csr[0], out.csr[1], val)
            return True


def _mxd_last_corner_off_by_one_ulp(kind, p, out, ins, aux):
    if kind == "mxd" and out.size and not np.isnan(out[-1, -1]):
        rc._bits(out)[-1, -1] += 1
        return True


def _sddmm_applies_accum_with_the_operands_exchanged(kind, p, out, ins, aux):
    if kind == "sddmm" and p["accum"] in sddmm_model.ARITHMETIC and len(out.csr[1]):
        val = rc.sddmm_accum_exchanged(p, ins[0][1], aux)
        if val is not None:
            out.csr = (out.csr[0], out.csr[1], val)
            return True


def _mxv_arg_gives_a_tie_to_the_larger_column(kind, p, out, ins, aux):
    if kind == "mxv_arg":
        rows, cols = rc.arg_ties(p, ins[0][1], aux)
        if len(rows):
            out[1][rows[0]] = cols[0]
            return True


def _a_dim0_input_gives_a_row_pointer_one_entry_too_long(kind, p, out, ins, aux):
    if kind != "extract" and isinstance(out, rc._Held) and any(0 in shape for shape, _ in ins):
        out.csr = (np.concatenate([out.csr[0], out.csr[0][-1:]]), out.csr[1], out.csr[2])
        return True


def _writes_past_a_callers_output(kind, p, framed):
    """ModelBackend.margin_hook: the element behind the first caller-owned output gets a value (its own last one, or 1)."""
    name = sorted(framed)[0]
    fr, bits = framed[name]
    bits[fr.pad + fr.n] = bits[fr.pad + fr.n - 1] if fr.n else 1
    return name


DEFECTS = {
    "select: the last value is off by one ulp": _select_last_value_off_by_one_ulp,
    "ewise: the last entry is dropped": _ewise_drops_its_last_entry,
    "mxv: a zero has the other sign": _mxv_flips_the_sign_of_a_zero,
    "transpose: two entries of equal column are swapped": _transpose_swaps_two_entries_of_equal_column,
    "reduce: the identity for an all-NaN row under plus": _reduce_gives_the_identity_for_a_row_of_nans,
    "extract: the second copy of a repeated row is dropped": _extract_drops_the_second_copy_of_a_repeated_row,
    "build: a run is folded in reverse list order under first or last": _build_folds_a_run_in_reverse_list_order,
    "mxd: the last column's last row is off by one ulp": _mxd_last_corner_off_by_one_ulp,
    "sddmm: an arithmetic accum is applied with the operands exchanged": _sddmm_applies_accum_with_the_operands_exchanged,
    "mxv_arg: a tie goes to the larger column": _mxv_arg_gives_a_tie_to_the_larger_column,
    "any kind on a dim0 input: the output's row pointer has one entry too many": _a_dim0_input_gives_a_row_pointer_one_entry_too_long,
    "margin: one element past a caller's output is written": _writes_past_a_callers_output,
}
# the defect of the margins goes in through ModelBackend.margin_hook: it damages the buffer around an output, not the output
HOOKED = {"margin: one element past a caller's output is written"}


class Defective(rc.ModelBackend):
    """The model backend but for ONE damaged output: the first call that offers the defect something to damage.  ``fired``
    and ``fired_kind`` say where that was."""

    def __init__(self, damage, hooked=False):
        self.damage, self.hooked, self.calls, self.fired, self.fired_kind = damage, hooked, 0, None, None
        if hooked:
            self.margin_hook = self._hook

    def _hook(self, kind, p, framed):
        if self.fired is None and self.damage(kind, p, framed):
            self.fired, self.fired_kind = self.calls, kind

    def run(self, kind, p, handles, staged):
        try:
            out, st = super().run(kind, p, handles, staged)
        finally:
            step, self.calls = self.calls, self.calls + 1
        if self.fired is None and self.damage is not None and not self.hooked:
            # (never the model's own arrays)
            out = out.copy() if isinstance(out, np.ndarray) else tuple(None if o is None else o.copy() for o in out) if isinstance(out, tuple) else out
            if self.damage(kind, p, out, [self.read(h) for h in handles], staged):
                self.fired, self.fired_kind = step, kind
        return out, st


def _first_failure(name, seeds):
    """(the mismatch, the step the defect was planted in, the kind it was planted in) of the first chain that fails, or
    (None, None, None)."""
    for seed in seeds:
        for dt in rc.DTYPES:
            be = Defective(DEFECTS[name], name in HOOKED)            # one chain per backend: a chain makes one call per step
            try:
                rc.Chain(be, seed, dt, rc.Coverage()).run()
            except rc.ChainMismatch as e:
                return e, be.fired, be.fired_kind
            assert be.fired is None, f"planted in seed {seed} {np.dtype(dt).name} step {be.fired} and NOT noticed"
    return None, None, None


@pytest.mark.parametrize("name", list(DEFECTS))
def test_a_planted_defect_fails_at_its_step(name):
    err, planted, kind = _first_failure(name, rc.DEFAULT_SEEDS)
    if err is None:
        pytest.fail(f"{name}: not detected")
    # (the defects of one kind carry its name; the two that fit any kind fail in the kind they were planted in)
    assert err.kind == kind == (name.split(":")[0] if name.split(":")[0] in rc.KINDS else kind) and err.step == planted, (str(err), planted)
    text = str(err)
    assert f"seed={err.seed} " in text and f"step={err.step} " in text and f"op={err.kind} " in text and "params={" in text
    if name in HOOKED:                                                                   # the side and the offset
        assert re.search(r"(vector|arg): the margin past the caller's output of \d+ elements changed at offset 1 past its last element", text), text
    else:
        assert re.search(r"(rowptr|col|val|vector|arg)\[\d+\]|entries", text), text            # the first differing position
    # the seed alone reproduces it
    again, planted2, kind2 = _first_failure(name, [err.seed])
    assert again is not None and (again.seed, again.dtype, again.step, planted2, kind2) == (err.seed, err.dtype, err.step, planted, kind)


def test_main_reports_a_mismatch_and_exits_non_zero(monkeypatch, capsys):
    monkeypatch.setattr(rc, "ModelBackend", lambda: Defective(_ewise_drops_its_last_entry))
    assert rc.main(["--backend", "model", "--seeds"] + [str(s) for s in rc.DEFAULT_SEEDS]) == 1
    out = capsys.readouterr().out
    seed = re.search(r"CHAIN_MISMATCH seed=(\d+) dtype=float\d+ step=\d+ op=ewise params=\{", out).group(1)
    assert "CHAIN_OK" not in out and f"python -m tests.result_chain --seeds {seed}" in out


# ---- errors that are no mismatch: they must leave the driver as themselves -------------------------------------------------------------
class _Failing(rc.ModelBackend):
    """The model backend, but the third call raises ``error``; counts what the driver does to it afterwards."""

    def __init__(self, error):
        self.error, self.calls, self.after = error, 0, 0

    def run(self, kind, p, handles, staged):
        self.calls += 1
        if self.calls == 3:
            raise self.error
        self.after += self.calls > 3
        return super().run(kind, p, handles, staged)

    def read(self, h):
        self.after += self.calls >= 3
        return super().read(h)

    def close(self, h):
        self.after += self.calls >= 3
        super().close(h)


def _osp_error(status):
    from outerspace_amd import _lib
    assert _lib.ERR_HIP == rc.ERR_HIP
    return _lib.OspError(status, "planted")


def test_a_refused_call_is_a_mismatch_and_a_device_error_is_not(monkeypatch, capsys):
    from outerspace_amd import _lib
    for refusal in (ValueError("planted"), TypeError("planted"), _osp_error(_lib.ERR_ARG), _osp_error(_lib.ERR_CAPACITY)):
        assert rc.is_refusal(refusal)
        be = _Failing(refusal)
        with pytest.raises(rc.ChainMismatch, match="the call raised " + type(refusal).__name__) as ei:
            rc.Chain(be, rc.DEFAULT_SEEDS[0], np.float32, rc.Coverage()).run()
        assert ei.value.step == 2
    # what may be a GPU fault: the library's HIP status, any error of torch (a RuntimeError), anything unknown
    for fault in (_osp_error(_lib.ERR_HIP), RuntimeError("HIP error: an illegal memory access was encountered"), KeyError("x")):
        assert not rc.is_refusal(fault)
        be = _Failing(fault)
        with pytest.raises(type(fault)) as ei:
            rc.Chain(be, rc.DEFAULT_SEEDS[0], np.float32, rc.Coverage()).run()
        assert ei.value is fault and not isinstance(ei.value, AssertionError)
        assert be.calls == 3 and be.after == 0          # nothing was run, read or closed behind it
        # main() has a status of its own for it, apart from a mismatch's 1 and the coverage's 2
        be = _Failing(fault)
        be.finish = lambda: pytest.fail("the context is closed after a device error")
        monkeypatch.setattr(rc, "ModelBackend", lambda: be)
        assert rc.main(["--backend", "model"]) == rc.DEVICE_ERROR_STATUS not in (0, 1, 2)
        out = capsys.readouterr().out
        assert "CHAIN_DEVICE_ERROR " + type(fault).__name__ in out and "CHAIN_OK" not in out and "CHAIN_MISMATCH" not in out
        assert be.after == 0


class _Quieting(rc.ModelBackend):
    """An upload that changes the NaNs it is given: ``change`` maps their bit patterns."""

    def __init__(self, change):
        self.change = change

    def upload(self, ncol, csr):
        val = csr[2].copy()
        nan = np.isnan(val)
        rc._bits(val)[nan] = self.change(rc._bits(val)[nan])
        return super().upload(ncol, (csr[0], csr[1], val))


@pytest.mark.parametrize("dt", rc.DTYPES)
def test_an_upload_may_quiet_a_nan_and_change_nothing_else(dt):
    quiet, low = (1 << 22, 1) if dt == np.float32 else (1 << 51, 1)
    sign = 1 << (31 if dt == np.float32 else 63)
    u = rc._bits(np.zeros(1, dt)).dtype.type
    seed = rc.DEFAULT_SEEDS[0]
    rc.Chain(_Quieting(lambda b: b | u(quiet)), seed, dt, rc.Coverage()).run()
    for name, change in (("payload", lambda b: b ^ u(low)), ("sign", lambda b: b ^ u(sign)), ("made signalling", lambda b: b & ~u(quiet) | u(low << 1))):
        with pytest.raises(rc.ChainMismatch, match="op=upload params=A: val") as ei:
            rc.Chain(_Quieting(change), seed, dt, rc.Coverage()).run()
        assert ei.value.step == -1, name
