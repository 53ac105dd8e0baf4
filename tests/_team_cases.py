"""Shared inputs and helpers of the teamed-batch tests (test_gpu_batch_team.py,
test_gpu_batch_team_edges.py, test_team_cases_cpu.py): the engine helpers of
the teamed suites, and the builders of the edge inputs -- LPs whose pivot row
and column sit in every wave of the team's workgroup and in the selection's
second pass, rows around twice the workgroup's width, teams as large as an LP
takes, and a pivot row above 64 KiB of LDS.  The shapes follow the knobs of
csrc/knobs.h.  A plain module: no fixtures; nothing here touches the GPU until
an engine helper is called."""
import os
import re

import numpy as np

import _contract_cases as cc
import _ragged_cases as rc
from lpsol_amd import _lib
from lpsol_amd import generators as gen

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "linear-program-solver_amd", "csrc")


def knob(name):
    text = open(os.path.join(CSRC, "knobs.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


WAVES = knob("LPK_TEAM_WAVES")
NT = 64 * WAVES                     # threads of one workgroup of a team
TEAM_MAX = knob("LPK_TEAM_MAX")
WINDOW = knob("LPK_TEAM_WINDOW")

CAP = 4096
STANDARD, MIN_INDEX = cc.RULE_STANDARD, cc.RULE_MIN_INDEX
RULES = (STANDARD, MIN_INDEX)


# ------------------------------------------------------------------ oracle
_ORACLE = {}


def _key(T, *rest):
    return (T.shape, T.tobytes()) + rest


def oracle_solve(T, cap=CAP, tol=None):
    """cc.oracle_solve, computed once per input"""
    key = _key(T, "solve", cap, tuple(sorted((tol or {}).items())))
    if key not in _ORACLE:
        with np.errstate(all="ignore"):
            _ORACLE[key] = cc.oracle_solve(T, cap, tol)
    return _ORACLE[key]


def oracle_run(T, rule, k):
    """cc.oracle_run, computed once per input"""
    key = _key(T, "run", rule, k)
    if key not in _ORACLE:
        with np.errstate(all="ignore"):
            _ORACLE[key] = cc.oracle_run(T, rule, k)
    return _ORACLE[key]


# ------------------------------------------------------------------ device
def records(eng, st, npiv, nstd, basis):
    T, z = eng.download(), eng.objective()
    bs = eng.get_basis() if basis is not None else None
    return [dict(status=int(st[i]), npiv=int(npiv[i]), nstd=int(nstd[i]), log=eng.log(i).tolist(), T=T[i], z=z[i],
                 basis=None if bs is None else list(bs[i])) for i in range(eng.count)]


def make_engine(stack, place, team, log_cap):
    if isinstance(stack, np.ndarray):
        return _lib.BatchEngine(stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1, log_cap=log_cap, place=place,
                                team=team)
    return _lib.RaggedEngine([rc.shape_of(T) for T in stack], log_cap=log_cap, place=place, team=team)


def check_plan(eng, teams):
    """team_plan() against team_of(): the teamed LPs ascending, each with its G
    ranges covering its elements in order, cut at even offsets of the buffer"""
    assert [eng.team_of(i) for i in range(eng.count)] == teams
    plan = eng.team_plan()
    assert [(p["lp"], p["team"]) for p in plan] == [(i, g) for i, g in enumerate(teams) if g > 1]
    shapes = getattr(eng, "shapes", None) or [(eng.m, eng.n)] * eng.count
    toff = np.concatenate([[0], np.cumsum([(m + 1) * (n + 1) for m, n in shapes])])
    for p in plan:
        m, n = shapes[p["lp"]]
        r = p["ranges"]
        assert len(r) == p["team"] and r[0][0] == 0 and r[-1][1] == (m + 1) * (n + 1)
        assert all(a < b for a, b in r) and all(r[k][1] == r[k + 1][0] for k in range(len(r) - 1))
        assert all((toff[p["lp"]] + a) % 2 == 0 for a, _ in r[1:])


def teamed_solve(stack, team, *, place="device", cap=CAP, tol=None, window=None, log_cap=CAP, basis=None,
                 teams=None):
    """one lp_batch_solve of a uniform stack or a list of LPs -> one record per LP"""
    eng = make_engine(stack, place, team, log_cap)
    try:
        if teams is not None:
            check_plan(eng, teams)
        if tol:
            eng.set_tol(**tol)
        if window is not None:
            eng.set_window(window)
        eng.upload(stack)
        if basis is not None:
            eng.set_basis(basis)
        return records(eng, *eng.solve(cap), basis)
    finally:
        eng.close()


def run_records(eng, rule, k):
    """one lp_batch_run on an engine that holds its input -> one record per LP"""
    st, done = eng.run(rule, k)
    return records(eng, st, done, np.zeros_like(done), None)


def teamed_run(stack, team, rule, k, *, place="device", window=None, log_cap=64, teams=None):
    """one lp_batch_run of a uniform stack or a list of LPs -> one record per LP"""
    eng = make_engine(stack, place, team, log_cap)
    try:
        if teams is not None:
            check_plan(eng, teams)
        if window is not None:
            eng.set_window(window)
        eng.upload(stack)
        return run_records(eng, rule, k)
    finally:
        eng.close()


def check(got, want, *, finite=True, what=""):
    """one LP's device record against the oracle's (or another device record)"""
    same = cc.same_bits if finite else cc.same_values
    assert got["status"] == want["status"], what
    assert (got["npiv"], got["nstd"]) == (want["npiv"], want["nstd"]), what
    assert got["log"] == want["log"], what
    assert same(got["T"], want["T"]), what
    assert same(np.atleast_1d(np.float64(got["z"])), np.atleast_1d(np.float64(want["z"]))), what


def check_stack(got, stack, *, cap=CAP, tol=None, finite=True, basis0=None):
    want = [oracle_solve(T, cap, tol) for T in stack]
    for i, (g, w) in enumerate(zip(got, want)):
        check(g, w, finite=finite, what=f"LP {i}")
        if basis0 is not None:
            b = list(basis0[i])
            for r, c in w["log"]:
                b[r] = c
            assert g["basis"] == b, i
    return want


def check_run(got, stack, rule, k):
    want = [oracle_run(T, rule, k) for T in stack]
    for i, (g, w) in enumerate(zip(got, want)):
        check(g, w, what=f"LP {i} rule {rule} run {k}")
    return want


def offsets(stack):
    """first double of every LP in the batch's buffers (and the end)"""
    return np.concatenate([[0], np.cumsum([T.size for T in stack])]).tolist()


# ---------------------------------------------------------------------------
# A. the winner of a reduction in every wave
# ---------------------------------------------------------------------------
# thread tid of the selection handles row 1 + tid and column 1 + tid: one index
# per wave at a different lane each, then the first and the last index of the
# selection loops' second pass
SPOTS = [1 + 64 * k + (7 * k) % 64 for k in range(WAVES)] + [NT + 1, NT + 64]
TIE = (SPOTS[WAVES - 2], SPOTS[2])      # two spots in different waves, the higher first
LONG = NT + 64


def row_lp(*rs):
    """m = NT + 64, n = 4: column 1 (cost -1, all ones) enters, every ratio is 3
    but 2 at rows rs"""
    T = np.zeros((LONG + 1, 5))
    T[0, 1] = -1.0
    T[1:, 1] = 1.0
    T[1:, 0] = 3.0
    for r in rs:
        T[r, 0] = 2.0
    return T


def row_stack():
    """one LP per spot, then the tie: the leaving row, the winning ratio and the first eligible row's wave"""
    return np.stack([row_lp(r) for r in SPOTS] + [row_lp(*TIE)])


def col_lp(rule, *cs):
    """m = 3, n = NT + 64, A all ones, b = (1, 2, 3): row 0 leaves.  Standard
    rule: cost -1 everywhere, -2 at columns cs.  Min-index rule: cost 0 before
    cs[0], -1 from there on."""
    T = np.zeros((4, LONG + 1))
    T[1:, 1:] = 1.0
    T[1:, 0] = [1.0, 2.0, 3.0]
    if rule == STANDARD:
        T[0, 1:] = -1.0
        for c in cs:
            T[0, c] = -2.0
    else:
        T[0, cs[0]:] = -1.0
    return T


def col_stack(rule):
    return np.stack([col_lp(rule, c) for c in SPOTS] + ([col_lp(rule, *TIE)] if rule == STANDARD else []))


# cc.CASES with the case's rows in the last two waves and in the second pass
LONG_EMBEDDING = (LONG, 40, (NT - 62, NT - 12, LONG))


# ---------------------------------------------------------------------------
# B. widths and heights around the stride of bpivot_dev's team walk, 2 NT
# ---------------------------------------------------------------------------
WIDE_WIDTHS = [2 * NT - 1, 2 * NT, 2 * NT + 1, 2 * NT + 2]      # n + 1: dj = 2 NT - 1 (di = 1), dj = 0, di = 0
WIDE_TEAMS = (2, 3, 7)
WIDE_RUNS = (3, 4)                                              # an odd and an even count: either buffer


def wide_stack(width):
    """3 rows of `width` doubles; an odd width makes E odd, LP 1 start at an odd double and pairs straddle rows"""
    return np.stack([gen.tableau("tall", 2, width - 1, s) for s in (1, 2)])


def narrow_stack():
    """w = 2: every pair is one row, di = NT"""
    return np.stack([gen.tableau("tall", NT + 3, 1, s) for s in (1, 2)])


def high_stack():
    """more rows than threads: the ratio test takes a second pass"""
    return np.stack([gen.tableau("tall", NT + 2, 7, s) for s in (1, 2)])


# ---------------------------------------------------------------------------
# C. ranges
# ---------------------------------------------------------------------------
def pair_stacks():
    """(stack, team E / 2): 3 x 3 (E = 9, the middle LP at an odd double) and the 4 x 6 base LP"""
    return [(np.stack([gen.tableau("tall", 2, 2, s) for s in (1, 2, 3)]), 4),
            (np.stack([cc.base_lp()] * 3), 12)]


def team_max_stacks():
    """the 9 x 19 shape (E odd) and mixed 40 x 40, for a team of TEAM_MAX"""
    return [gen.mixed_stack(8, 10, range(1, 4)), gen.mixed_stack(40, 40, (1, 2))]


# ---------------------------------------------------------------------------
# D. the team's LDS above 64 KiB
# ---------------------------------------------------------------------------
BIG_ROW = 8200
BIG_LDS = 65752


def big_row_stack():
    return np.stack([gen.tableau("tall", 1, BIG_ROW, s) for s in (1, 2)])


# ---------------------------------------------------------------------------
# E. more workgroups than the chip holds
# ---------------------------------------------------------------------------
FULL_SEEDS = range(1, 97)
RESIDENT = 256 * (2048 // NT)       # workgroups of NT threads the chip's 256 CUs hold at once, at the most


def full_stack():
    return gen.mixed_stack(8, 10, FULL_SEEDS)


# ---------------------------------------------------------------------------
# F. the stall band's edge (the other contract inputs are _contract_cases')
# ---------------------------------------------------------------------------
def stall_band(km):
    """Klee-Minty starts at objective 0 and moves at every pivot, so under a
    stall tolerance s the standard pivots count as stuck while |z| <= s.
    -> (lo, hi) = |z| after m + n - 1 and after m + n pivots.  With lo <= s < hi
    the counter is reset by pivot m + n, one short of the switch to the
    min-index rule; with s = hi the switch happens.  A stall test that saw the
    objective one pivot late would switch at every s in [lo, hi]."""
    k = km.shape[0] + km.shape[1] - 2
    return abs(oracle_solve(km, k - 1)["z"]), abs(oracle_solve(km, k)["z"])


def stall_edges(km):
    lo, hi = stall_band(km)
    return [lo, (lo + hi) / 2, hi]


# ---------------------------------------------------------------------------
# G. calls
# ---------------------------------------------------------------------------
def ragged_mix():
    """-> (lps, teams): LDS-placed LPs, team-1 device LPs and teams of 2, 3, 5
    and 7, in a scrambled order; the 3 x 3 LP makes the LPs behind it start at
    odd doubles"""
    lps = [gen.tableau("mixed", 8, 10, 1), gen.tableau("tall", 2, 2, 1), gen.tableau("mixed", 40, 40, 3),
           gen.tableau("mixed", 100, 100, 1), gen.tableau("mixed", 8, 10, 2), gen.tableau("mixed", 16, 16, 1),
           gen.tableau("mixed", 100, 100, 2), gen.tableau("mixed", 24, 32, 1), gen.tableau("mixed", 8, 10, 3)]
    return lps, [1, 1, 5, 1, 3, 1, 2, 7, 1]


CONTINUED_CAP = 51


def continued_stack():
    return gen.mixed_stack(100, 100, (1, 2))
