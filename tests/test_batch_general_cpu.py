"""General-form batches (lp_general_*; solve_problems with bounds, maximize
and c0): the parts that need no GPU.

The counts, the per-LP tables, the shift loop, the cell classifier and the
lane walks are pure functions of csrc/batch_plan.h: csrc/batch_general_check.cpp
drives them from stdin, built here with -fsanitize=address,undefined and run as
a child process, so a sanitizer report fails the test that met it."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import _general_cases as gc
import _problem_cases as pc
import lpsol_amd
from lpsol_amd import _lib, solve_problems, solve_problems_ragged

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
SYMBOLS = {"lp_general_rows", "lp_general_columns", "lp_general_set_form", "lp_general_vars", "lp_general_upload",
           "lp_general_solution", "lp_general_duals"}


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpgpu.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(lp_general_\w+)\s*\(", header)) == SYMBOLS
    assert {s for s in _lib.EXPORTS if s.startswith("lp_general_")} == SYMBOLS
    for name in SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    for code, name in enumerate(("PLAIN", "LOWER", "BOXED", "UPPER", "FREE")):
        assert re.search(r"#define\s+LP_VAR_%s\s+%d\b" % (name, code), header)
        assert getattr(_lib, "VAR_" + name) == code and getattr(lpsol_amd, "VAR_" + name) == code
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        for method in ("set_form", "upload_general", "general_solution", "general_duals", "general_vars"):
            assert callable(getattr(cls, method))
        p = inspect.signature(cls.general_duals).parameters
        assert p["first"].default == 0 and p["count"].default is None
        assert inspect.signature(cls.upload_general).parameters["first"].default == 0
    assert {"general_kinds", "general_shape", "pack_general", "general_standard_form", "general_recover",
            "general_duals"} <= set(lpsol_amd.__all__)
    for fn in (solve_problems, solve_problems_ragged):
        p = inspect.signature(fn).parameters
        assert p["lb"].default is None and p["ub"].default is None and p["maximize"].default is False
        assert p["c0"].default is None
    assert isinstance(lpsol_amd.ProblemResult.reduced_costs, property)


def test_null_batch_is_refused():
    lib = _lib.load()
    one = np.ones(1, dtype=np.int64)
    codes = np.zeros(4, dtype=np.int8)
    p8, p64 = codes.ctypes.data_as(_lib._P8), one.ctypes.data_as(_lib._P64)
    assert lib.lp_general_set_form(None, p64, p64, p8, p8, p8) == _lib.BAD_ARG
    assert lib.lp_general_set_form(None, None, None, None, None, None) == _lib.BAD_ARG
    m, ns = ctypes.c_int64(-9), ctypes.c_int64(-8)
    assert lib.lp_general_vars(None, 0, ctypes.byref(m), ctypes.byref(ns)) == _lib.BAD_ARG
    assert (m.value, ns.value) == (-9, -8)
    src, x, z = np.full(8, 7.0), np.full(8, 6.0), np.full(8, 5.0)
    assert lib.lp_general_upload(None, 0, 1, _lib._ptr(src)) == _lib.BAD_ARG
    assert lib.lp_general_upload(None, 0, 0, None) == _lib.BAD_ARG
    assert lib.lp_general_solution(None, 0, 2, _lib._ptr(x), _lib._ptr(z)) == _lib.BAD_ARG
    assert lib.lp_general_duals(None, 0, 2, _lib._ptr(x), _lib._ptr(z)) == _lib.BAD_ARG
    assert src.tolist() == [7.0] * 8 and x.tolist() == [6.0] * 8 and z.tolist() == [5.0] * 8


def test_general_rows_and_columns():
    lib = _lib.load()

    def shape(sense, kind, m=None, ns=None):
        s, k = np.array(sense, dtype=np.int8), np.array(kind, dtype=np.int8)
        args = (s.ctypes.data_as(_lib._P8), k.ctypes.data_as(_lib._P8), len(s) if m is None else m,
                len(k) if ns is None else ns)
        return lib.lp_general_rows(*args), lib.lp_general_columns(*args)

    assert shape([0, 0, 0], [0] * 5) == (3, 8)                  # all PLAIN: lp_problem_columns
    assert shape([0, 1, 2], [0, 1, 2, 3, 4]) == (4, 9)
    assert shape([2], [2]) == (2, 2)                            # an equality and a box
    assert shape([0], [4]) == (1, 3)
    assert shape(pc.MIXED_SENSE, [2] * 5) == (10, 14)
    assert shape([0, 1, 7], [0, 9], m=2, ns=1) == (2, 3)        # only m and ns entries are read
    k = np.zeros(2, dtype=np.int8).ctypes.data_as(_lib._P8)
    assert lib.lp_general_rows(None, k, 2, 2) == _lib.BAD_ARG and lib.lp_general_columns(k, None, 2, 2) == _lib.BAD_ARG
    for sense, kind, m, ns in (([0], [0], 0, 1), ([0], [0], 1, 0), ([0], [0], -1, 1), ([3], [0], None, None),
                               ([-1], [0], None, None), ([0], [5], None, None), ([0], [-1], None, None)):
        assert shape(sense, kind, m, ns) == (_lib.BAD_ARG, _lib.BAD_ARG)
    for s, kd in (([0, 1, 2], [0, 1, 2, 3, 4]), (pc.MIXED_SENSE, [2, 4, 4, 0, 3])):
        assert lpsol_amd.general_shape(s, kd) == shape(s, kd)
    with pytest.raises(ValueError):
        lpsol_amd.general_shape([], [0])
    with pytest.raises(ValueError, match="a kind must be"):
        lpsol_amd.general_shape([0], [5])


def test_pack_general():
    P, s, kind, lb, ub = gc.general_lp(5)
    G = lpsol_amd.pack_general(P, lb, ub)
    assert G.shape == (6 * 6 + 10,)
    assert pc.same_bits(G[:36], P.ravel()) and pc.same_bits(G[36:41], lb) and pc.same_bits(G[41:], ub)
    G2 = lpsol_amd.pack_general(np.stack([P, P]), lb, np.stack([ub, ub + 1]))
    assert G2.shape == (2, 46) and pc.same_bits(G2[0], G) and pc.same_bits(G2[1, 41:], ub + 1)
    assert pc.same_bits(lpsol_amd.pack_general(P, None, None)[36:], np.r_[np.zeros(5), np.full(5, np.inf)])


# ---------------------------------------------------------------------------
# the rules under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_general_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_general_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return [dict(kv.split("=") for kv in ln.split()) for ln in got]
    return run


def digits(codes):
    return "".join(str(int(s)) for s in codes)


def test_counts_and_tables_of_each_kind_alone(check):
    got = check(["counts senses=0 kinds=%d" % k for k in range(5)] + ["tables senses=0 kinds=%d" % k for k in range(5)])
    want = {0: (0, 0, 1, 2), 1: (0, 0, 1, 2), 2: (0, 1, 2, 3), 3: (0, 0, 1, 2), 4: (1, 0, 1, 3)}
    for k in range(5):
        g = got[k]
        assert g["st"] == "0" and (int(g["nf"]), int(g["nb"]), int(g["rows"]), int(g["cols"])) == want[k], (k, g)
        assert g["m"] == "1" and g["ns"] == "1" and g["k"] == "1"
    tabs = got[5:]
    # var entries are src:brow:neg:kind; src = 2 j + flip
    assert tabs[0] == dict(st="0", var="0:0:0:0", slack="2", bvar="-1")
    assert tabs[1] == dict(st="0", var="0:0:0:1", slack="2", bvar="-1")
    assert tabs[2] == dict(st="0", var="0:2:0:2", slack="2,3", bvar="-1,0")       # its bound row is tableau row 2
    assert tabs[3] == dict(st="0", var="1:0:0:3", slack="2", bvar="-1")           # flipped
    assert tabs[4] == dict(st="0", var="0:0:2:4,1:0:0:4", slack="3", bvar="-1")   # the negative part in column 2


def test_counts_and_tables_of_mixed_forms(check):
    got = check(["counts senses=012 kinds=01234", "tables senses=012 kinds=01234",
                 "counts senses=202 kinds=2202", "tables senses=202 kinds=2202",       # equalities mixed with boxes
                 "tables senses=%s kinds=44" % digits(pc.MIXED_SENSE)])
    assert (got[0]["nf"], got[0]["nb"], got[0]["k"], got[0]["rows"], got[0]["cols"]) == ("1", "1", "2", "4", "9")
    assert got[1] == dict(st="0", var="0:0:0:0,2:0:0:1,4:4:0:2,7:0:0:3,8:0:6:4,9:0:0:4", slack="7,-8,0,9",
                          bvar="-1,-1,-1,2")
    assert (got[2]["nf"], got[2]["nb"], got[2]["k"], got[2]["rows"], got[2]["cols"]) == ("0", "3", "1", "6", "8")
    # the <= row owns the first slack column, the three bound rows the next three, in variable order
    assert got[3] == dict(st="0", var="0:4:0:2,2:5:0:2,4:0:0:0,6:6:0:2", slack="0,5,0,6,7,8", bvar="-1,-1,-1,0,1,3")
    assert got[4]["var"] == "0:0:3:4,2:0:4:4,1:0:0:4,3:0:0:4" and got[4]["slack"] == "-5,0,6,7,-8"


def test_refusals_leave_the_output_alone(check):
    got = check(["counts senses=0130 kinds=01",        # a sense outside 0..2: names the row
                 "counts senses=01 kinds=0150",        # a kind outside 0..4: names the variable
                 "counts senses=0 kinds=0 m=0",
                 "counts senses=0 kinds=0 ns=-2",
                 "counts senses= kinds=0 m=1"])         # NULL senses
    assert (got[0]["st"], got[0]["bad"]) == ("-1", "2") and (got[1]["st"], got[1]["bad"]) == ("-2", "2")
    assert got[2]["st"] == "-3" and got[3]["st"] == "-3" and got[4]["st"] == "-3"
    assert all(g["untouched"] == "1" for g in got)


def test_grid(check):
    got = check(["grid lanes=%d" % e for e in (0, 1, 256, 257, 65 * 9 * 19, 1 << 50)])
    assert all(g["threads"] == "256" for g in got)
    assert [int(g["blocks"]) for g in got[:5]] == [-(-e // 256) for e in (0, 1, 256, 257, 65 * 9 * 19)]
    assert got[5]["blocks"] == "-1"                 # more than a grid holds


def sweep_line(lps, first, count, uniform):
    """lps: (m, ns, senses, kinds, maximise) per LP"""
    return "sweep shapes=%s senses=%s kinds=%s max=%s first=%d count=%d uniform=%d" % (
        ",".join("%d:%d" % (m, ns) for m, ns, _, _, _ in lps), "/".join(digits(s) for _, _, s, _, _ in lps),
        "/".join(digits(k) for _, _, _, k, _ in lps), digits(int(x) for _, _, _, _, x in lps), first, count, uniform)


def elems_of(lps):
    total = 0
    for m, ns, s, k, _ in lps:
        mp, n = lpsol_amd.general_shape(s, k)
        total += (mp + 1) * (n + 1)
    return total


UNIFORM_SWEEPS = [          # (m, ns, senses, kinds, maximise, LPs)
    (1, 1, [pc.LE], [gc.PLAIN], 0, 3),
    (1, 1, [pc.GE], [gc.LOWER], 1, 3),
    (1, 1, [pc.EQ], [gc.BOXED], 0, 2),
    (1, 1, [pc.LE], [gc.UPPER], 1, 5),
    (1, 1, [pc.GE], [gc.FREE], 0, 4),
    (5, 5, pc.MIXED_SENSE, [0, 1, 2, 3, 4], 1, 11),
    (5, 5, pc.MIXED_SENSE, [0, 1, 2, 3, 4], 0, 11),
    (8, 10, [pc.LE] * 8, [gc.BOXED] * 10, 0, 65),       # 65 x 19 x 29 elements: several workgroups, no multiple of 256
    (3, 4, [pc.EQ] * 3, [2, 4, 2, 4], 1, 6),            # equalities mixed with boxes: the only slacks are the bounds'
    (4, 1, [pc.LE, pc.GE, pc.LE, pc.GE], [gc.FREE], 1, 7),
    (3, 5, [pc.LE] * 3, [gc.PLAIN] * 5, 0, 5),          # the problem form's layout
]


def assert_clean(g, elems):
    assert int(g["elems"]) == elems, g
    for key in ("bad_shift", "bad_map", "bad_cells", "bad_recover", "bad_duals"):
        assert g[key] == "0", g


def test_lane_walks_on_uniform_windows(check):
    lines, elems = [], []
    for m, ns, s, k, mx, B in UNIFORM_SWEEPS:
        lps = [(m, ns, s, k, mx)] * B
        for first, count in ((0, B), (B - 1, 1), (B // 2, B - B // 2)):
            lines.append(sweep_line(lps, first, count, 1))
            elems.append(elems_of(lps[first:first + count]))
    for g, e in zip(check(lines), elems):
        assert_clean(g, e)


def ragged_lps():
    return [(P.shape[0] - 1, P.shape[1] - 1, s, k, mx) for P, s, k, _, _, mx in gc.ragged_general()]


def test_lane_walks_on_ragged_windows(check):
    lps = ragged_lps()
    assert [(m, ns) for m, ns, _, _, _ in lps] == pc.RAGGED_SHAPES
    lines = [sweep_line(lps, f, c, 0) for f, c in pc.RAGGED_WINDOWS]
    elems = [elems_of(lps[f:f + c]) for f, c in pc.RAGGED_WINDOWS]
    # the uniform forms once more through the ragged lookup
    for m, ns, s, k, mx, B in UNIFORM_SWEEPS:
        lines.append(sweep_line([(m, ns, s, k, mx)] * B, 0, B, 0))
        elems.append(elems_of([(m, ns, s, k, mx)] * B))
    for g, e in zip(check(lines), elems):
        assert_clean(g, e)
