"""Warm cuts (lp_cut_extend; extend_into, extend, add_rows): the parts that need
no GPU.

The table of the window, the cell classifier, the lane lookups of the three
kernels and the grouped row loop are pure functions of csrc/batch_plan.h:
csrc/batch_cut_check.cpp drives them from stdin, built here with
-fsanitize=address,undefined and run as a child process, so a sanitizer report
fails the test that met it."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import _cut_cases as cc
from lpsol_amd import _lib
from lpsol_amd.problem import ProblemRaggedResult, ProblemResult

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
NAMES = ["lp_cut_extend"]


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpgpu.h")).read(), flags=re.S)
    assert re.findall(r"\b(lp_cut_\w+)\s*\(", header) == NAMES
    assert [s for s in _lib.EXPORTS if s.startswith("lp_cut_")] == NAMES
    fn = lib.lp_cut_extend
    res, argt = _lib._PROTOS["lp_cut_extend"]
    assert fn.restype is res and list(fn.argtypes) == list(argt)
    assert argt == [_lib._H, _lib._H, _lib._I64, _lib._I64, _lib._PD, _lib._P8]
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        assert list(inspect.signature(cls.extend_into).parameters)[1:] == ["dst", "rows", "sense", "first"]
        assert inspect.signature(cls.extend_into).parameters["first"].default == 0
        p = inspect.signature(cls.extend).parameters
        assert list(p)[1:] == ["rows", "sense", "log_cap", "place", "team"]
        assert all(p[k].default is None and p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[3:])
    for cls in (ProblemResult, ProblemRaggedResult):
        p = inspect.signature(cls.add_rows).parameters
        assert list(p)[1:] == ["A", "b", "sense", "max_pivots", "place"]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("max_pivots", "place"))
    knobs = open(os.path.join(CSRC, "knobs.h")).read()
    plan = open(os.path.join(CSRC, "batch_plan.h")).read()
    assert re.findall(r"define LPK_CUT_GROUP (\d+)", knobs) == re.findall(r"define LPK_CUT_GROUP (\d+)", plan) != []


def test_null_batch_is_refused():
    lib = _lib.load()
    a, s = np.full(8, 7.0), np.zeros(2, dtype=np.int8)
    assert lib.lp_cut_extend(None, None, 0, 1, _lib._ptr(a), s.ctypes.data_as(_lib._P8)) == _lib.BAD_ARG
    assert lib.lp_cut_extend(None, None, 0, 0, None, None) == _lib.BAD_ARG
    assert a.tolist() == [7.0] * 8


# ---------------------------------------------------------------------------
# add_rows: everything wrong with a call is found before any device call
# ---------------------------------------------------------------------------

class _NoEngine:
    """stands where a live engine would: any use of it is a device call"""
    m, n = 3, 8

    def __getattr__(self, name):
        raise AssertionError("device call: " + name)


B, M, NS = 2, 3, 5


def _result(sense=("<=",) * M, kind=None, cls=ProblemResult, rows=M):
    s = _lib.sense_codes(sense)
    z = np.zeros(B, dtype=np.int64)
    n = NS + int(np.count_nonzero(s != _lib.SENSE_EQ))
    data = dict(c=np.ones((B, NS)), b=np.ones((B, M)))
    if cls is ProblemRaggedResult:
        data = {k: list(v) for k, v in data.items()}
        return cls(_NoEngine(), "plain", [s] * B, [NS] * B, z, z, z + rows, z, z, z, np.zeros(B), None,
                   [np.zeros(n)] * B, kind=None if kind is None else [kind] * B,
                   maximize=None if kind is None else [False] * B, **data)
    return cls(_NoEngine(), "plain", s, NS, z, z, z + rows, z, z, z, np.zeros(B), None, np.zeros((B, n)), kind=kind,
               maximize=None if kind is None else False, **data)


@pytest.mark.parametrize("cls", [ProblemResult, ProblemRaggedResult])
def test_add_rows_refuses_before_any_device_call(cls):
    rag = cls is ProblemRaggedResult
    wrap = (lambda a: list(a)) if rag else (lambda a: a)
    A, b = np.ones((B, 2, NS)), np.ones((B, 2))
    res = _result(cls=cls)
    with pytest.raises(ValueError, match="general-form result"):
        _result(kind=np.zeros(NS, dtype=np.int8), cls=cls).add_rows(wrap(A), wrap(b))
    with pytest.raises(ValueError, match='LP 0 is given an "==" row'):
        res.add_rows(wrap(A), wrap(b), [["<=", "=="]] * B if rag else ["<=", "=="])
    with pytest.raises(ValueError, match="max_pivots"):
        res.add_rows(wrap(A), wrap(b), max_pivots=-1)
    with pytest.raises(ValueError, match="LP 0: phase 1 left 2 of its 3 rows live"):
        _result(cls=cls, rows=2).add_rows(wrap(A), wrap(b))
    # shapes
    with pytest.raises(ValueError, match="A of LP 1 must be" if rag else "A must be"):
        res.add_rows([A[0], A[1][:, :4]] if rag else A[:, :, :4], wrap(b))
    with pytest.raises(ValueError, match="A of LP 0 must be" if rag else "b must be"):
        res.add_rows(wrap(A), wrap(b[:, :1]))
    with pytest.raises(ValueError, match="one entry per LP" if rag else "A must be"):
        res.add_rows(wrap(A[:1]), wrap(b[:1]))
    with pytest.raises(ValueError, match="sense of LP 0 must hold 2" if rag else "sense must hold 2"):
        res.add_rows(wrap(A), wrap(b), [["<="]] * B if rag else ["<="])
    with pytest.raises(ValueError, match="a sense must be"):
        res.add_rows(wrap(A), wrap(b), [["<=", "<"]] * B if rag else ["<=", "<"])
    # a good call goes on to the engine; an "==" row among the old ones is no obstacle
    for r in (res, _result(("<=", "==", ">="), cls=cls)):
        with pytest.raises(AssertionError, match="device call"):
            r.add_rows(wrap(A), wrap(b), [["<=", ">="]] * B if rag else ["<=", ">="])
    if rag:     # q_i = 0 is a shape of its own
        with pytest.raises(AssertionError, match="device call"):
            res.add_rows([A[0], np.zeros((0, NS))], [b[0], []])


# ---------------------------------------------------------------------------
# the rules under the host sanitizers
# ---------------------------------------------------------------------------

def build(objdir=None, defs=None):
    cmd = ["make", "-s", "-C", CSRC, "batch_cut_check"]
    if objdir:
        cmd += ["OBJDIR=" + objdir, "DEFS=" + defs]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, objdir or "build", "batch_cut_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return [dict(kv.split("=") for kv in ln.split()) for ln in got]
    return run


@pytest.fixture(scope="module")
def check():
    return build()


@pytest.fixture(scope="module")
def check_run4():
    """the same rules with four destination elements per lane of k_cut_copy and two new rows per group"""
    return build("build/cut_run4", "-DLPK_ASSEMBLE_RUN=4 -DLPK_CUT_GROUP=2")


def restate(shapes, first, count):
    """what the three launches write, from the header's statement alone -> (cells, basis, lanes of k_cut_rows)"""
    src = np.concatenate([[0], np.cumsum([(m + 1) * (n + 1) for m, n, _ in shapes])])
    sb = np.concatenate([[0], np.cumsum([m for m, _, _ in shapes])])
    cells, basis = [], []
    for i, (m, n, q) in enumerate(shapes):
        inside = first <= i < first + count
        for row in range(m + q + 1):
            for col in range(n + q + 1):
                if not inside:
                    cells.append("-")
                elif row <= m:
                    cells.append("c%d" % (src[i] + row * (n + 1) + col) if col <= n else "z")
                elif col <= n:
                    cells.append("p")
                else:
                    cells.append("o" if col - n == row - m else "z")
        for r in range(m + q):
            basis.append("-" if not inside else "s%d" % (sb[i] + r) if r < m else "n%d" % (n + r - m))
    return cells, basis


WALKS = [([(1, 1, 1)], 0, 1),
         ([(8, 18, 2)] * 5, 0, 5), ([(8, 18, 2)] * 5, 1, 3), ([(8, 18, 2)] * 40, 3, 36),
         # a ragged window with q in {0, 1, 3}, and windows that begin and end on an LP without a lane of k_cut_rows
         ([(8, 18, 0), (24, 48, 1), (1, 2, 3), (8, 18, 3), (1, 2, 0), (24, 48, 0), (3, 4, 1), (2, 1, 3), (5, 9, 0)], 0, 9),
         ([(8, 18, 0), (24, 48, 1), (1, 2, 3), (8, 18, 3), (1, 2, 0), (24, 48, 0), (3, 4, 1), (2, 1, 3), (5, 9, 0)], 4, 2),
         ([(8, 18, 0), (24, 48, 1), (1, 2, 3), (8, 18, 3), (1, 2, 0), (24, 48, 0), (3, 4, 1), (2, 1, 3), (5, 9, 0)], 2, 6),
         # widths 1 + n + q around a run of four: the run crosses a row end, the copied / zero border, the
         # last row of an LP and the window's end
         ([(2, 2, 1)] * 3, 0, 3), ([(2, 3, 1)] * 3, 0, 2), ([(1, 1, 3), (2, 4, 2), (1, 1, 1)], 0, 3),
         ([(3, 5, 5), (1, 7, 9)], 0, 2), ([(2, 6, 0), (2, 6, 1)] * 3, 1, 4)]


def assert_walks(run, group, per_lane):
    lines = ["walk shapes=%s first=%d count=%d" % (",".join("%d:%d:%d" % s for s in shapes), f, c)
             for shapes, f, c in WALKS]
    knobs = run(["knobs"])[0]
    assert (int(knobs["group"]), int(knobs["run"]), int(knobs["threads"])) == (group, per_lane, 256)
    for (shapes, f, c), g in zip(WALKS, run(lines)):
        cells, basis = restate(shapes, f, c)
        assert g["bad"] == "0", (shapes, f, c)
        assert g["cells"].split(",") == cells, (shapes, f, c)
        assert g["basis"].split(",") == basis, (shapes, f, c)
        window = shapes[f:f + c]
        assert int(g["elems"]) == sum((m + q + 1) * (n + q + 1) for m, n, q in window)
        assert int(g["nbasis"]) == sum(m + q for m, _, q in window)
        assert int(g["lanes"]) == sum(-(-q // group) * (n + 1) for _, n, q in window)


def test_cells_and_lanes(check):
    group = int(re.search(r"define LPK_CUT_GROUP (\d+)", open(os.path.join(CSRC, "knobs.h")).read()).group(1))
    assert_walks(check, group, 1)


def test_cells_and_lanes_with_runs_of_four(check_run4):
    assert_walks(check_run4, 2, 4)


def hexes(a):
    return ",".join("%016x" % v for v in np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64))


def rows_line(g, T, basis, rows, sense):
    return "rows g=%d n=%d basis=%s cells=%s rows=%s sense=%s" % (
        g, T.shape[1] - 1, ",".join(map(str, basis)), hexes(T[1:]), hexes(rows), ",".join(str(int(s)) for s in sense))


@pytest.mark.parametrize("which", ["check", "check_run4"])
def test_the_grouped_loop_gives_the_stated_bits(which, request):
    """one accumulator per row of a group, a column read once per group: the bits of extend() for a group of 1,
    a full group, and one row more than a group"""
    run = request.getfixturevalue(which)
    group = int(run(["knobs"])[0]["group"])
    lines, want = [], []
    for shape, seed, q in ((cc.SMALL, 1, 1), (cc.SMALL, 2, group), (cc.SMALL, 3, group + 1), ((1, 1), 4, group + 1),
                           (cc.MID, 5, 2 * group + 1)):
        c = cc.case(*shape, seed, "lege", q)
        basis = c["basis"].copy()
        if len(basis) > 2:
            basis[1], basis[2] = -1, c["opt"].shape[1] - 1       # skipped: a dropped row's entry, and n
        D, _ = cc.extend(c["opt"], basis, c["rows"], c["sense"])
        for g in sorted({0, 1, group}):
            lines.append(rows_line(g, c["opt"], basis, c["rows"], c["sense"]))
            want.append(hexes(D[c["opt"].shape[0]:, :c["opt"].shape[1]]))
    # products an fma would round differently, and the odd cells
    third = 1.0 / 3.0
    T = np.array([[0.0, 0.0, 0.0], [third, 3.0, third], [3.0, third, 1.0]])
    rows = np.array([[1.0, third, third / 3.0], [third, 3.0, third]])
    D, _ = cc.extend(T, [0, 1], rows, [cc.LE, cc.GE])
    lines.append(rows_line(0, T, [0, 1], rows, [cc.LE, cc.GE]))
    want.append(hexes(D[3:, :3]))
    To, bo, ro, so = cc.odd_case()
    Do, _ = cc.extend(To, bo, ro, so)
    lines.append(rows_line(0, To, bo, ro, so))
    want.append(hexes(Do[4:, :5]))
    for g, w in zip(run(lines), want):
        gv = np.array([int(h, 16) for h in g["priced"].split(",")], dtype=np.uint64).view(np.float64)
        wv = np.array([int(h, 16) for h in w.split(",")], dtype=np.uint64).view(np.float64)
        nan = np.isnan(wv)
        assert np.array_equal(np.isnan(gv), nan) and gv[~nan].tobytes() == wv[~nan].tobytes()
