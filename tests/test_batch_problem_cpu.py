"""Problem-form batches (lp_problem_*; solve_problems, solve_problems_ragged):
the parts that need no GPU.

The slack table, the grid of k_assemble and its lane walk are pure functions
of csrc/batch_plan.h: csrc/batch_problem_check.cpp drives them from stdin,
built here with -fsanitize=address,undefined and run as a child process, so a
sanitizer report fails the test that met it."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import _problem_cases as pc
import lpsol_amd
from lpsol_amd import _lib, solve_problems, solve_problems_ragged

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
SYMBOLS = {"lp_problem_columns", "lp_problem_set_senses", "lp_problem_vars", "lp_problem_upload",
           "lp_problem_duals"}


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpgpu.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(lp_problem_\w+)\s*\(", header)) == SYMBOLS
    assert {s for s in _lib.EXPORTS if s.startswith("lp_problem_")} == SYMBOLS
    for name in SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    assert re.search(r"#define\s+LP_SENSE_LE\s+0\b", header) and re.search(r"#define\s+LP_SENSE_GE\s+1\b", header)
    assert re.search(r"#define\s+LP_SENSE_EQ\s+2\b", header)
    assert (_lib.SENSE_LE, _lib.SENSE_GE, _lib.SENSE_EQ) == (0, 1, 2)
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        for method in ("set_senses", "upload_problems", "duals", "nvars"):
            assert callable(getattr(cls, method))
        p = inspect.signature(cls.duals).parameters
        assert p["first"].default == 0 and p["count"].default is None
        assert inspect.signature(cls.upload_problems).parameters["first"].default == 0
    assert {"solve_problems", "solve_problems_ragged", "ProblemResult", "ProblemRaggedResult", "problem_columns",
            "assemble_tableaux", "problem_duals", "pack_problems"} <= set(lpsol_amd.__all__)
    p = inspect.signature(solve_problems).parameters
    assert p["sense"].default is None and p["place"].default == "lds" and p["log_cap"].default == 0


def test_sense_codes():
    assert _lib.sense_codes(["<=", ">=", "==", 0, 1, 2, np.int8(2)]).tolist() == [0, 1, 2, 0, 1, 2, 2]
    assert _lib.sense_codes([]).dtype == np.int8
    for bad in ("<", "=", 3, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="a sense must be"):
            _lib.sense_codes([0, bad])


def test_null_batch_is_refused():
    lib = _lib.load()
    sense = np.zeros(4, dtype=np.int8)
    assert lib.lp_problem_set_senses(None, sense.ctypes.data_as(_lib._P8)) == _lib.BAD_ARG
    assert lib.lp_problem_set_senses(None, None) == _lib.BAD_ARG
    ns = ctypes.c_int64(-9)
    assert lib.lp_problem_vars(None, 0, ctypes.byref(ns)) == _lib.BAD_ARG and ns.value == -9
    src = np.full(8, 7.0)
    assert lib.lp_problem_upload(None, 0, 1, _lib._ptr(src)) == _lib.BAD_ARG
    assert lib.lp_problem_upload(None, 0, 0, None) == _lib.BAD_ARG
    y = np.full(8, 7.0)
    assert lib.lp_problem_duals(None, 0, 2, _lib._ptr(y)) == _lib.BAD_ARG
    assert y.tolist() == [7.0] * 8 and src.tolist() == [7.0] * 8


def test_problem_columns():
    lib = _lib.load()

    def columns(sense, ns, m=None):
        a = np.array(sense, dtype=np.int8)
        return lib.lp_problem_columns(a.ctypes.data_as(_lib._P8), len(a) if m is None else m, ns)

    assert columns([0, 0, 0], 5) == 8
    assert columns([2, 2], 5) == 5
    assert columns(pc.MIXED_SENSE, 4) == 8
    assert columns([1], 1) == 2
    assert columns([0, 1, 2, 7], 3, m=3) == 5          # only m entries are read
    assert lib.lp_problem_columns(None, 3, 5) == _lib.BAD_ARG
    for sense, ns, m in (([0], 0, None), ([0], -1, None), ([0], 3, 0), ([0], 3, -2), ([0, 3], 2, None),
                         ([-1, 0], 2, None)):
        assert columns(sense, ns, m) == _lib.BAD_ARG
    assert lpsol_amd.problem_columns(["<=", "==", ">="], 3) == 5
    with pytest.raises(ValueError):
        lpsol_amd.problem_columns([], 3)
    with pytest.raises(ValueError):
        lpsol_amd.problem_columns([0], 0)


def test_argument_errors_come_before_any_device_call():
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2))
    c, A, b = pc.parts(T, ns)
    far = dict(device=1 << 20)
    with pytest.raises(ValueError, match="a sense must be"):
        solve_problems(c, A, b, ["<=", "=<", "<="], **far)
    with pytest.raises(ValueError, match="a sense must be"):
        solve_problems(c, A, b, [0, 1, 3], **far)
    with pytest.raises(ValueError, match="sense must hold 3 entries"):
        solve_problems(c, A, b, ["<=", "<="], **far)
    with pytest.raises(ValueError, match="c must be"):
        solve_problems(c[:, :4], A, b, **far)
    with pytest.raises(ValueError, match="b must be"):
        solve_problems(c, A, b[:1], **far)
    with pytest.raises(ValueError, match="A must be"):
        solve_problems(c, A[0], b, **far)
    with pytest.raises(ValueError, match="place must be"):
        solve_problems(c, A, b, place="hbm", **far)
    one = (c[0], A[0], b[0], None)
    with pytest.raises(ValueError, match="empty batch"):
        solve_problems_ragged([], **far)
    with pytest.raises(ValueError, match="LP 1: sense must hold 3 entries"):
        solve_problems_ragged([one, (c[1], A[1], b[1], ["<="])], **far)
    with pytest.raises(ValueError, match="LP 1: c must be"):
        solve_problems_ragged([one, (c[1][:2], A[1], b[1], None)], **far)
    with pytest.raises(ValueError, match="a sense must be"):
        solve_problems_ragged([(c[0], A[0], b[0], ["<=", "<=", "!="])], **far)
    with pytest.raises(ValueError, match=r"LP 0 must be \(c, A, b, sense\)"):
        solve_problems_ragged([(c[0], A[0], b[0])], **far)


def test_problem_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2))
    c, A, b = pc.parts(T, ns)
    with pytest.raises(_lib.EngineUnavailable):
        solve_problems(c, A, b)
    with pytest.raises(_lib.EngineUnavailable):
        solve_problems_ragged([(c[0], A[0], b[0], None)])


# ---------------------------------------------------------------------------
# the rules under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_problem_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_problem_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return [dict(kv.split("=") for kv in ln.split()) for ln in got]
    return run


def digits(sense):
    return "".join(str(int(s)) for s in sense)


def test_slack_table(check):
    got = check(["table senses=%s n=9" % digits(pc.MIXED_SENSE),
                 "table senses=222 n=3",            # all ==: k = 0, a pure copy
                 "table senses=0 n=2",              # m = 1
                 "table senses=1 n=2",
                 "table senses=000 n=4"])           # ns = 1
    assert got[0] == dict(ns="5", row="-1", table="-6,0,7,8,-9", untouched="1")
    assert got[1] == dict(ns="3", row="-1", table="0,0,0", untouched="1")
    # the entry is the TABLEAU column 1 + j of variable column j = ns + t
    assert got[2]["ns"] == "1" and got[2]["table"] == "2"
    assert got[3]["ns"] == "1" and got[3]["table"] == "-2"
    assert got[4] == dict(ns="1", row="-1", table="2,3,4", untouched="1")


def test_slack_table_refusals_leave_the_output_alone(check):
    got = check(["table senses=0130 n=9",           # a sense outside 0..2: names the row
                 "table senses=00 n=2",             # k = n
                 "table senses=011 n=2",            # k > n
                 "table senses=2 n=0"])
    assert got[0] == dict(ns="-1", row="2", table="-", untouched="1")
    assert got[1]["ns"] == "-2" and got[2]["ns"] == "-2" and got[3]["ns"] == "-3"
    assert all(g["untouched"] == "1" for g in got)


def test_assemble_grid(check):
    got = check(["grid elems=%d" % e for e in (0, 1, 256, 257, 65 * 9 * 19, 1 << 50)])
    run = int(got[0]["run"])
    assert run >= 1 and all(g["threads"] == "256" for g in got)
    want = [-(-(-(-e // run)) // 256) for e in (0, 1, 256, 257, 65 * 9 * 19)]      # ceil(ceil(e / run) / 256)
    assert [int(g["blocks"]) for g in got[:5]] == want
    assert got[5]["blocks"] == "-1"                 # more than a grid holds


def sweep_line(shapes, senses, first, count, uniform):
    """shapes: (m, ns) per LP; the check takes (m, n)"""
    text = ",".join("%d:%d" % (m, ns + int(np.count_nonzero(np.asarray(s) != pc.EQ)))
                    for (m, ns), s in zip(shapes, senses))
    return "sweep shapes=%s senses=%s first=%d count=%d uniform=%d" % (
        text, "/".join(digits(s) for s in senses), first, count, uniform)


UNIFORM_SWEEPS = [          # (m, ns, senses, LPs)
    (3, 5, [pc.LE] * 3, 5),
    (8, 10, [pc.LE] * 8, 65),                       # 65 x 171 elements: no multiple of 256, several workgroups
    (1, 1, [pc.GE], 3),                             # m = 1, ns = 1
    (1, 1, [pc.EQ], 1),                             # a 1 x 1 copy
    (4, 1, [pc.LE, pc.GE, pc.LE, pc.GE], 7),        # ns = 1
    (1, 6, [pc.LE], 9),                             # m = 1
    (6, 3, [pc.EQ] * 6, 4),                         # all ==: k = 0
    (5, 4, pc.MIXED_SENSE, 11),
]


def test_lane_walk_on_uniform_windows(check):
    lines, elems = [], []
    for m, ns, sense, B in UNIFORM_SWEEPS:
        n = ns + sum(1 for s in sense if s != pc.EQ)
        for first, count in ((0, B), (B - 1, 1), (B // 2, B - B // 2)):
            lines.append(sweep_line([(m, ns)] * B, [sense] * B, first, count, 1))
            elems.append(count * (m + 1) * (n + 1))
    for g, e in zip(check(lines), elems):
        assert int(g["elems"]) == e and g["bad_map"] == "0" and g["bad_cells"] == "0", g


def test_lane_walk_on_ragged_windows(check):
    shapes = pc.RAGGED_SHAPES
    senses = [pc.cycled_senses(i, m) for i, (m, _) in enumerate(shapes)]
    lines = [sweep_line(shapes, senses, f, c, 0) for f, c in pc.RAGGED_WINDOWS]
    # the uniform shapes once more through the ragged lookup
    lines += [sweep_line([(m, ns)] * B, [sense] * B, 0, B, 0) for m, ns, sense, B in UNIFORM_SWEEPS]
    got = check(lines)
    for (f, c), g in zip(pc.RAGGED_WINDOWS, got):
        want = sum((m + 1) * (ns + int(np.count_nonzero(s != pc.EQ)) + 1)
                   for (m, ns), s in zip(shapes[f:f + c], senses[f:f + c]))
        assert int(g["elems"]) == want
    assert all(g["bad_map"] == "0" and g["bad_cells"] == "0" for g in got), got
