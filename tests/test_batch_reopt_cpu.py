"""Warm re-optimisation (lp_reopt_set_costs, lp_reopt_set_general; set_costs,
set_general, reoptimize): the parts that need no GPU.

The grid of k_cost, its lane -> (LP, column) lookup, its row-0 loop and the
border -> block map of k_general_restage are pure functions of
csrc/batch_plan.h: csrc/batch_reopt_check.cpp drives them from stdin, built
here with -fsanitize=address,undefined and run as a child process, so a
sanitizer report fails the test that met it."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import _general_cases as gc
import _problem_cases as pc
import _reopt_cases as rc
from lpsol_amd import _lib
from lpsol_amd.problem import ProblemRaggedResult, ProblemResult, general_shape

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
NAMES = ["lp_reopt_set_costs", "lp_reopt_set_general"]


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpgpu.h")).read(), flags=re.S)
    assert re.findall(r"\b(lp_reopt_\w+)\s*\(", header) == NAMES
    assert [s for s in _lib.EXPORTS if s.startswith("lp_reopt_")] == NAMES
    for name in NAMES:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt)
        assert argt == [_lib._H, _lib._I64, _lib._I64, _lib._PD]
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        assert inspect.signature(cls.set_costs).parameters["first"].default == 0
        assert inspect.signature(cls.set_general).parameters["first"].default == 0
    for cls in (ProblemResult, ProblemRaggedResult):
        p = inspect.signature(cls.reoptimize).parameters
        assert list(p)[1:] == ["b", "c", "lb", "ub", "c0", "max_pivots"]
        assert all(p[k].default is None and p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])


def test_null_batch_is_refused():
    lib = _lib.load()
    a = np.full(8, 7.0)
    for name in NAMES:
        assert getattr(lib, name)(None, 0, 1, _lib._ptr(a)) == _lib.BAD_ARG
        assert getattr(lib, name)(None, 0, 0, None) == _lib.BAD_ARG
    assert a.tolist() == [7.0] * 8


# ---------------------------------------------------------------------------
# reoptimize: everything wrong with a call is found before any device call
# ---------------------------------------------------------------------------

class _NoEngine:
    """stands where a live engine would: any use of it is a device call"""
    m, n = 3, 8

    def __getattr__(self, name):
        raise AssertionError("device call: " + name)


B, M, NS = 2, 3, 5


def _result(sense=("<=",) * M, kind=None, cls=ProblemResult, host=True):
    s = _lib.sense_codes(sense)
    z = np.zeros(B, dtype=np.int64)
    n = NS + int(np.count_nonzero(s != _lib.SENSE_EQ)) if kind is None else general_shape(s, kind)[1]
    data = {}
    if host:
        lb = np.zeros((B, NS)) if kind is None else np.stack([gc.bounds_of(kind, np.ones(NS))[0]] * B)
        ub = np.full((B, NS), np.inf) if kind is None else np.stack([gc.bounds_of(kind, np.ones(NS))[1]] * B)
        data = dict(c=np.ones((B, NS)), b=np.ones((B, M)), lb=lb, ub=ub)
    if cls is ProblemRaggedResult:
        data = {k: list(v) for k, v in data.items()}
        return cls(_NoEngine(), "plain", [s] * B, [NS] * B, z, z, z + M, z, z, z, np.zeros(B), None,
                   [np.zeros(n)] * B, kind=None if kind is None else [kind] * B,
                   maximize=None if kind is None else [False] * B, **data)
    return cls(_NoEngine(), "plain", s, NS, z, z, z + M, z, z, z, np.zeros(B), None, np.zeros((B, n)), kind=kind,
               maximize=None if kind is None else False, **data)


KIND = np.array([gc.PLAIN, gc.LOWER, gc.BOXED, gc.UPPER, gc.FREE], dtype=np.int8)


@pytest.mark.parametrize("cls", [ProblemResult, ProblemRaggedResult])
def test_reoptimize_refuses_before_any_device_call(cls):
    rag = cls is ProblemRaggedResult
    wrap = (lambda a: list(a)) if rag else (lambda a: a)
    b, c = np.ones((B, M)), np.ones((B, NS))
    res = _result(cls=cls)
    with pytest.raises(ValueError, match="one side per call"):
        res.reoptimize(b=wrap(b), c=wrap(c))
    with pytest.raises(ValueError, match="one side per call"):
        res.reoptimize()
    with pytest.raises(ValueError, match="one side per call"):
        res.reoptimize(c0=1.0)
    with pytest.raises(ValueError, match="one side per call"):
        _result(kind=KIND, cls=cls).reoptimize(ub=wrap(np.ones((B, NS))), c=wrap(c))
    with pytest.raises(ValueError, match="max_pivots"):
        res.reoptimize(c=wrap(c), max_pivots=-1)
    # shapes
    with pytest.raises(ValueError, match="b of LP 1 must hold 3" if rag else "b must be"):
        res.reoptimize(b=[b[0], b[1][:2]] if rag else b[:, :2])
    with pytest.raises(ValueError, match="c of LP 0 must hold 5" if rag else "c must be"):
        res.reoptimize(c=[c[0][:4], c[1]] if rag else c[:, :4])
    with pytest.raises(ValueError, match="c must hold one array per LP" if rag else "c must be"):
        res.reoptimize(c=wrap(c[:1]))
    # bounds on a result that has none
    with pytest.raises(ValueError, match="general-form result"):
        res.reoptimize(ub=wrap(np.ones((B, NS))))
    # an equality row: the dual side, and either side of a general-form result
    eq = ("<=", "==", ">=")
    with pytest.raises(ValueError, match='LP 0 has an "==" row'):
        _result(eq, cls=cls).reoptimize(b=wrap(b))
    with pytest.raises(ValueError, match='LP 0 has an "==" row'):
        _result(eq, kind=KIND, cls=cls).reoptimize(c=wrap(c))


@pytest.mark.parametrize("cls", [ProblemResult, ProblemRaggedResult])
def test_reoptimize_keeps_the_pattern_of_finite_bounds(cls):
    wrap = (lambda a: list(a)) if cls is ProblemRaggedResult else (lambda a: a)
    lb0, ub0 = gc.bounds_of(KIND, np.ones(NS))
    inf = np.inf
    # (variable, its kind's name in the message, lb or ub, the value that breaks the pattern)
    for j, side, value in ((0, "lb", 1.0), (0, "ub", 5.0), (1, "lb", -inf), (1, "ub", 5.0), (2, "lb", -inf),
                           (2, "ub", inf), (3, "lb", 0.0), (3, "ub", inf), (4, "lb", 0.0), (4, "ub", 5.0),
                           (2, "lb", np.nan), (1, "ub", np.nan)):
        new = np.stack([lb0 if side == "lb" else ub0] * B)
        new[1, j] = value
        with pytest.raises(ValueError, match="LP 1, variable %d" % j):
            _result(kind=KIND, cls=cls).reoptimize(**{side: wrap(new)})
    # lb > ub on a BOXED variable is no refusal of the host's: the call goes on to the engine
    new = np.stack([ub0] * B)
    new[0, 2] = lb0[2] - 1.0
    with pytest.raises(AssertionError, match="device call"):
        _result(kind=KIND, cls=cls).reoptimize(ub=wrap(new))
    # a general-form result without the first call's data cannot build the border
    with pytest.raises(ValueError, match="was not kept"):
        _result(kind=KIND, cls=cls, host=False).reoptimize(ub=wrap(np.stack([ub0] * B)))


def test_a_stale_result_refuses_reoptimize_and_resolve_still_refuses_general_form():
    res = _result()
    res._y = np.ones((B, M))
    res._stale = True
    with pytest.raises(RuntimeError, match="resolve"):
        res.reoptimize(c=np.ones((B, NS)))
    with pytest.raises(RuntimeError, match="resolve"):
        res.reoptimize(b=np.ones((B, M)))
    with pytest.raises(ValueError, match="general-form"):
        _result(kind=np.zeros(NS, dtype=np.int8)).resolve(np.ones((B, M)))
    # the constructors' positional order is what it was; the host copies are keywords with defaults
    p = list(inspect.signature(ProblemResult.__init__).parameters)
    assert p[1:14] == ["engine", "path", "sense", "ns", "status", "stage", "rows", "ninit", "npiv", "nstd",
                       "objective", "basis", "xall"]
    assert p[14:] == ["kind", "maximize", "x", "z0", "c", "b", "lb", "ub"]


# ---------------------------------------------------------------------------
# the rules under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_reopt_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_reopt_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return [dict(kv.split("=") for kv in ln.split()) for ln in got]
    return run


def test_grid(check):
    got = check(["grid pairs=%d" % p for p in (0, 1, 256, 257, 64 * 19, 1 << 50)])
    assert all(g["threads"] == "256" for g in got)
    assert [int(g["blocks"]) for g in got[:5]] == [0, 1, 1, 2, 5]
    assert got[5]["blocks"] == "-1"                 # more than a grid holds


def hexes(a):
    return ",".join("%016x" % v for v in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64))


def test_the_loop_gives_numpy_float64_bits(check):
    """acc - c * t with every product and difference rounded: the same bits as the statement the GPU tests use"""
    lines, want = [], []
    for (m, ns), seed, how in ((rc.SMALL, 1, "tilt"), (rc.SMALL, 2, "swing"), ((1, 1), 3, "tilt"), ((5, 3), 4, "swing"),
                               (rc.LARGE, 5, "tilt")):
        c = rc.cost_case(m, ns, seed, how)
        T, basis, n = c["opt"], c["basis"].copy(), c["opt"].shape[1] - 1
        row = rc.some_costs(n, seed)
        if m > 1:
            basis[m // 2] = -1              # a dropped row's entry: skipped
        new = rc.reprice(T, basis, row)
        for col in sorted({0, 1, n // 2, n}):
            lines.append("cell col=%d n=%d basis=%s cells=%s costs=%s"
                         % (col, n, ",".join(map(str, basis)), hexes(T[1:, col]), hexes(row)))
            want.append("%016x" % new[0, col:col + 1].view(np.uint64)[0])
    # products that an fma would round differently, a NaN that must spread, an overflow, an entry of n (skipped)
    third, big = 1.0 / 3.0, 1.7e308
    for cells, costs, basis in (([third, 3.0], [1.0, third, third / 3.0], [0, 1]),
                                ([np.nan, 1.0], [0.0, 1.0, 1.0], [0, 1]),
                                ([big, -big], [0.0, 2.0, 2.0], [0, 1]),
                                ([5.0, 7.0], [1.0, 2.0, 3.0], [2, -1])):
        T = np.zeros((3, 3))
        T[1:, 0] = cells
        with np.errstate(all="ignore"):
            new = rc.reprice(T, basis, costs)
        lines.append("cell col=0 n=2 basis=%s cells=%s costs=%s" % (",".join(map(str, basis)), hexes(cells), hexes(costs)))
        want.append("%016x" % new[0, :1].view(np.uint64)[0])
    got = [g["acc"] for g in check(lines)]
    nan = [np.isnan(np.array([int(w, 16)], dtype=np.uint64).view(np.float64)[0]) for w in want]
    for g, w, is_nan in zip(got, want, nan):
        if is_nan:
            assert np.isnan(np.array([int(g, 16)], dtype=np.uint64).view(np.float64)[0])
        else:
            assert g == w
    assert sum(nan) == 2            # the NaN cell, and -inf + inf
    assert want[-1] == "%016x" % np.array([1.0]).view(np.uint64)[0]       # both entries skipped


def line(what, shapes, first, count, uniform):
    return "%s shapes=%s first=%d count=%d uniform=%d" % (what, ",".join("%d:%d" % s for s in shapes), first, count,
                                                         uniform)


UNIFORM = [(3, 8, 5), (8, 18, 64), (1, 1, 3), (2, 1, 300), (40, 80, 8), (5, 6, 7)]       # (m, n, LPs); n = 1 twice


def windows(count):
    return sorted({(0, count), (0, 1), (count - 1, 1), (count // 2, count - count // 2), (1, max(1, count - 2)),
                   (2, max(1, count - 4))} if count > 4 else {(0, count), (0, 1), (count - 1, 1)})


def test_cost_lanes_on_uniform_windows(check):
    lines, pairs = [], []
    for m, n, count in UNIFORM:
        for first, cnt in windows(count):
            lines.append(line("sweep", [(m, n)] * count, first, cnt, 1))
            pairs.append(cnt * (n + 1))
    for g, p in zip(check(lines), pairs):
        assert g == dict(pairs=str(p), bad_map="0", bad_cells="0", bad_rest="0"), g
    assert 64 * 19 % 256 != 0 and 256 % 19 != 0         # 8 x 18: LP boundaries inside every block, a partial last one


def test_cost_lanes_on_ragged_windows(check):
    shapes = [(m, ns + m) for m, ns in pc.RAGGED_SHAPES] + [(m, ns + m) for m, ns in rc.RAGGED_SHAPES]
    wins = windows(len(shapes)) + [(12, 1), (13, 4), (16, 5)]
    lines = [line("sweep", shapes, f, c, 0) for f, c in wins]
    # the uniform shapes once more through the ragged lookup
    lines += [line("sweep", [(m, n)] * count, 1, count - 1, 0) for m, n, count in UNIFORM]
    got = check(lines)
    for (f, c), g in zip(wins, got):
        assert int(g["pairs"]) == sum(n + 1 for _, n in shapes[f:f + c])
    assert all((g["bad_map"], g["bad_cells"], g["bad_rest"]) == ("0", "0", "0") for g in got), got


def test_border_lanes(check):
    """every border double lands on its own cell of the stored block, and A stays"""
    lines, lanes = [], []
    for m, ns, count in [(3, 5, 5), (8, 10, 64), (1, 1, 3), (1, 6, 300), (24, 24, 16), (4, 1, 7)]:
        for first, cnt in windows(count):
            lines.append(line("restage", [(m, ns)] * count, first, cnt, 1))
            lanes.append(cnt * (3 * ns + m + 1))
    shapes = pc.RAGGED_SHAPES + rc.RAGGED_SHAPES
    for first, cnt in windows(len(shapes)) + [(12, 1), (13, 4)]:
        lines.append(line("restage", shapes, first, cnt, 0))
        lanes.append(sum(3 * ns + m + 1 for m, ns in shapes[first:first + cnt]))
    for g, n in zip(check(lines), lanes):
        assert g == dict(lanes=str(n), bad_map="0", bad_cells="0", bad_rest="0"), g
