"""Batch solutions on the device (lp_solution_canonical, lp_solution_gather,
result= of the four batch solve functions): the parts that need no GPU.

The grids of the flat kernels and the lane -> LP lookup of csrc/batch_plan.h
are pure functions: csrc/batch_solution_check.cpp drives them from stdin, built
here with -fsanitize=address,undefined and run as a child process, so a
sanitizer report fails the test that met it."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import _solution_cases as sc
from lpsol_amd import _lib, solve_batch, solve_lp_batch, solve_lp_ragged, solve_ragged

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
SYMBOLS = {"lp_solution_canonical", "lp_solution_gather"}


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpgpu.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(lp_solution_\w+)\s*\(", text)) == SYMBOLS
    assert {s for s in _lib.EXPORTS if s.startswith("lp_solution_")} == SYMBOLS
    for name in SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        for method in ("derive_basis", "solution"):
            p = inspect.signature(getattr(cls, method)).parameters
            assert p["first"].default == 0 and p["count"].default is None
    for fn in (solve_batch, solve_lp_batch, solve_ragged, solve_lp_ragged):
        assert inspect.signature(fn).parameters["result"].default == "full"


def test_null_batch_is_refused():
    lib = _lib.load()
    flags = np.full(4, -9, dtype=np.int32)
    bad = ctypes.c_int64(-9)
    assert lib.lp_solution_canonical(None, 0, 4, flags.ctypes.data_as(_lib._P32), ctypes.byref(bad)) == _lib.BAD_ARG
    assert flags.tolist() == [-9] * 4 and bad.value == -9
    x, z = np.full(8, 7.0), np.full(4, 7.0)
    assert lib.lp_solution_gather(None, 0, 4, _lib._ptr(x), _lib._ptr(z)) == _lib.BAD_ARG
    assert x.tolist() == [7.0] * 8 and z.tolist() == [7.0] * 4
    assert lib.lp_solution_canonical(None, 0, 0, None, None) == _lib.BAD_ARG
    assert lib.lp_solution_gather(None, 0, 0, None, None) == _lib.BAD_ARG


def test_unknown_result_is_refused_before_any_device_call():
    T = sc.e2e_mixed()[:2]
    for fn, arg in ((solve_batch, T), (solve_lp_batch, T), (solve_ragged, list(T)), (solve_lp_ragged, list(T))):
        with pytest.raises(ValueError, match="result must be one of"):
            fn(arg, result="nonsense", device=1 << 20)
        with pytest.raises(ValueError, match="result must be one of"):
            fn(arg, result=None)


def test_solution_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    T = sc.e2e_mixed()[:2]
    for fn, arg in ((solve_batch, T), (solve_lp_batch, T), (solve_ragged, list(T)), (solve_lp_ragged, list(T))):
        with pytest.raises(_lib.EngineUnavailable):
            fn(arg, result="solution")


# ---------------------------------------------------------------------------
# the launch rules under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_solution_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_solution_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return [dict(kv.split("=") for kv in ln.split()) for ln in got]
    return run


def test_row_slices_follow_the_tallest_lp(check):
    ms = [1, 8, 16, 17, 64, 128, 129, 513, 100000]
    got = [int(g["slices"]) for g in check(["slices m=%d" % m for m in ms])]
    assert got == [1, 1, 1, 4, 4, 4, 16, 16, 16]


def test_scan_grid_at_both_ends_of_the_range(check):
    small, one, edge, none, huge = check([
        "scan cols=%d m=8" % (16384 * 11),      # 16384 LPs of 9 x 11: one wave per workgroup, a lane per column
        "scan cols=514 m=513",                  # one 513 x 513 LP: sixteen waves share each column
        "scan cols=64 m=3",
        "scan cols=0 m=3",
        "scan cols=%d m=3" % (1 << 40),         # more than a grid holds
    ])
    assert small == dict(blocks=str(16384 * 11 // 64), threads="64", slices="1")
    assert one == dict(blocks="9", threads="1024", slices="16")
    assert edge == dict(blocks="1", threads="64", slices="1")
    assert none["blocks"] == "0" and huge["blocks"] == "-1"


def test_flat_grid(check):
    got = check(["flat lanes=%d per=256 threads=256" % k for k in (1, 256, 257, 0)])
    assert [g["blocks"] for g in got] == ["1", "1", "2", "0"] and all(g["threads"] == "256" for g in got)


def test_scan_grid_sweep(check):
    (got,) = check(["sweep cols=400 m=140"])
    assert got == dict(checked=str(400 * 140), bad="0")


def test_lane_lookup_on_ragged_windows(check):
    shapes = [(m, 13) for m in range(1, 13)] + [(1, 1), (1, 1), (70, 200), (1, 1), (3, 1)]
    text = ",".join("%d:%d" % s for s in shapes)
    windows = [(0, len(shapes)), (0, 1), (len(shapes) - 1, 1), (2, 3), (11, 4), (13, 4)]
    got = check(["locate shapes=%s first=%d count=%d" % (text, f, c) for f, c in windows])
    for (f, c), g in zip(windows, got):
        assert int(g["lanes"]) == sum(n + 1 for _, n in shapes[f:f + c])
        assert int(g["entries"]) == sum(m for m, _ in shapes[f:f + c])
        assert g["bad"] == "0"
