"""The library's environment settings (outerspace_amd/csrc/osp_settings.h): parsing against libc, the reader under
AddressSanitizer + UBSan, and the table as the single source of truth.  tests/settings_driver.cpp prints what the header makes
of the environment; every case runs it in a child process of its own."""
import ctypes
import glob
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "outerspace_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "settings_driver.cpp")

UNSET = None
VALUES = [UNSET, "", "0", "1", "2", "-1", "abc", " 7", "7x", "0x10", "0.5", "1e3", "18446744073709551615", "99999999999999999999"]

libc = ctypes.CDLL(None)
libc.atoi.restype, libc.atoi.argtypes = ctypes.c_int, [ctypes.c_char_p]
libc.atol.restype, libc.atol.argtypes = ctypes.c_long, [ctypes.c_char_p]
libc.strtoull.restype, libc.strtoull.argtypes = ctypes.c_ulonglong, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
libc.atof.restype, libc.atof.argtypes = ctypes.c_double, [ctypes.c_char_p]


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, DRIVER], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "settings_driver", ["-O1"])


def _run(exe, env_vars, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("OSP_")}
    env.update(env_vars)
    r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope="module")
def table(driver):
    """[(name, kind, when)] as the header's table has them"""
    rows = [tuple(line.split()) for line in _run(driver, {}, "--names").splitlines()]
    assert len(rows) == len({r[0] for r in rows}) and all(len(r) == 3 for r in rows)
    return rows


def _expected(kind, v):
    """What the parent commit's expression made of the value `v` (None: unset), by the same libc functions, plus the rule of
    the kind; an empty value counts as unset for every kind but the presence flags."""
    b = None if v is None else v.encode()
    given = bool(b)
    if kind == "Flag":      # getenv(X) != nullptr; OSP_GUARD: ... && atoi(getenv(X)) == 2
        return {"set": b is not None, "value": libc.atoi(b) if b is not None else 0}
    if kind == "Switch":    # !(getenv(X) && atoi(getenv(X)) == 0)
        return not (given and libc.atoi(b) == 0)
    if kind == "Int":       # getenv(X) ? atoi(getenv(X)) : dflt
        return {"set": given, "value": libc.atoi(b) if given else 0}
    if kind == "Long":      # getenv(X) ? atol(getenv(X)) : dflt
        return {"set": given, "value": libc.atol(b) if given else 0}
    if kind == "U64":       # getenv(X) ? strtoull(getenv(X), nullptr, 10) : dflt
        return {"set": given, "value": libc.strtoull(b, None, 10) if given else 0}
    if kind == "Real":      # getenv(X) ? atof(getenv(X)) : dflt
        return {"set": given, "value": libc.atof(b) if given else 0.0}
    if kind == "Word":      # getenv(X) && strcmp(getenv(X), word) == 0
        return v or ""
    raise AssertionError(f"unknown kind {kind}")


def _decode(kind, got):
    if kind == "Real":
        return {"set": got["set"], "value": float.fromhex(got["value"])}
    return got


@pytest.mark.parametrize("value", VALUES, ids=lambda v: "unset" if v is None else repr(v))
def test_every_setting_parses_as_libc_does(driver, table, value):
    """Every setting of the table set to the same value (or none of them set): each member is what libc makes of it."""
    kinds = {kind for _, kind, _ in table}
    assert kinds == {"Flag", "Switch", "Int", "Long", "U64", "Real", "Word"}
    got = json.loads(_run(driver, {} if value is None else {name: value for name, _, _ in table}))
    assert set(got) == {name for name, _, _ in table}
    for name, kind, _ in table:
        assert _decode(kind, got[name]) == _expected(kind, value), (name, kind, value)


def test_rules_of_the_kinds(driver):
    """The rules themselves, spelled out once (the libc comparison above cannot tell a wrong rule from a right one that both
    sides share): presence flags, off switches, the signed clamp's input, the value OSP_DIRECT_MIN_NNZ's default hangs on."""
    got = json.loads(_run(driver, {"OSP_VERBOSE": "0", "OSP_GUARD": "2", "OSP_SYNC": "", "OSP_DIRECT": "abc", "OSP_HUB": "1", "OSP_PLAN_SMALL": "",
                                   "OSP_PLAN_SMALL_CELLS": "-5", "OSP_GATHER": "0", "OSP_DIRECT_MIN_NNZ": "", "OSP_HUB_MIN_SHARE": "0.5",
                                   "OSP_TRANSPOSE_PATH": "sort", "OSP_DIRECT_MAX": "-1"}))
    assert got["OSP_VERBOSE"] == {"set": True, "value": 0}            # OSP_VERBOSE=0 is verbose
    assert got["OSP_GUARD"] == {"set": True, "value": 2}
    assert got["OSP_SYNC"]["set"] is True                             # a presence flag: even empty
    assert got["OSP_POISON"]["set"] is False
    assert got["OSP_DIRECT"] is False                                 # atoi("abc") == 0 switches it off
    assert got["OSP_HUB"] is True and got["OSP_PLAN_SMALL"] is True   # (empty: unset)
    assert got["OSP_EXPAND_ROWS"] is True
    assert got["OSP_PLAN_SMALL_CELLS"] == {"set": True, "value": -5}  # signed: the use site clamps it to the minimum
    assert got["OSP_GATHER"] == {"set": True, "value": 0}             # ... which makes OSP_DIRECT_MIN_NNZ default to 8 M
    assert got["OSP_DIRECT_MIN_NNZ"]["set"] is False
    assert float.fromhex(got["OSP_HUB_MIN_SHARE"]["value"]) == 0.5
    assert got["OSP_TRANSPOSE_PATH"] == "sort" and got["OSP_TRANSPOSE_GATHER"] == ""
    assert got["OSP_DIRECT_MAX"] == {"set": True, "value": 2**64 - 1}  # strtoull("-1")


def test_reader_under_sanitizers(tmp_path_factory, table):
    """The same driver as a stand-alone program under AddressSanitizer + UBSan."""
    exe = _build(tmp_path_factory, "settings_driver_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer"])
    for value in (UNSET, "", "abc", " 7", "-1", "99999999999999999999", "x" * 5000):
        got = json.loads(_run(exe, {} if value is None else {name: value for name, _, _ in table}))
        for name, kind, _ in table:
            assert _decode(kind, got[name]) == _expected(kind, value), (name, kind, value[:20] if value else value)


def test_getenv_only_in_the_settings_header():
    files = [f for ext in ("h", "hip", "cpp") for f in glob.glob(os.path.join(CSRC, f"*.{ext}"))]
    assert len(files) > 20
    users = sorted(os.path.basename(f) for f in files if "getenv" in open(f).read())
    assert users == ["osp_settings.h"]


def test_table_equals_the_documented_settings(table):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 7. "):]
    documented = set()
    for line in sec.splitlines():
        m = re.match(r"\|\s*`(OSP_[A-Z0-9_]+)", line)
        if m:
            documented.add(m.group(1))
    assert "OSP_LIBRARY" in documented          # read by Python, not by the library
    assert documented - {"OSP_LIBRARY"} == {name for name, _, _ in table}
    # ... and when each of them is read
    when = {name: w for name, _, w in table}
    assert {n for n, w in when.items() if w == "process"} == {"OSP_GUARD", "OSP_POISON", "OSP_SYNC"}
    assert {n for n, w in when.items() if w == "context"} == {"OSP_RANK", "OSP_DENSE_ADD"}
