"""Teamed batches on the GPU, the edges of k_batch_team (csrc/batch.hip;
DESIGN.md 4l) that test_gpu_batch_team.py's shapes do not reach: a reduction's
winner in each of the workgroup's waves and in the selection's second pass,
rows around and above the stride of bpivot_dev's team walk, teams of one pair per
workgroup and of LPK_TEAM_MAX, a pivot row above 64 KiB of LDS, a grid above
the chip's residency, the placed suite's contract sections at a team, and the
calls not yet made on a teamed batch.  The inputs are tests/_team_cases.py's;
test_team_cases_cpu.py checks from the oracle alone that they reach these.

Every comparison is exact: status, pivot counts, the log, the basis and the
objective are equal to the oracle's (oracle/lp_f64.c through
_contract_cases.oracle_solve / oracle_run), and the tableaux are bit-identical
(same_values where the input holds non-finite cells).  Every device call
carries a finite pivot cap."""
import numpy as np
import pytest

import _contract_cases as cc
import _ragged_cases as rc
import _team_cases as tm
import test_gpu_batch_team as team_suite
from _team_cases import (CAP, RULES, TEAM_MAX, check, check_plan, check_run, check_stack, make_engine, oracle_solve,
                         records, run_records, teamed_run, teamed_solve)
from lpsol_amd import _lib
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis

pytestmark = pytest.mark.gpu

STANDARD, MIN_INDEX = tm.STANDARD, tm.MIN_INDEX


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def no_basis(stack):
    """a basis of -1 for LPs that are not canonical: only the pivots' own entries show"""
    return np.full((len(stack), stack[0].shape[0] - 1), -1, dtype=np.int32)


# ---------------------------------------------------------------------------
# A. the winner of a reduction in every wave
# ---------------------------------------------------------------------------

def solve_and_run(stack, team, spots):
    """the solve and a run of both rules, each against the oracle -> the logs of [solve, standard, min-index]"""
    teams = [team] * len(stack)
    got = teamed_solve(stack, team, log_cap=8, basis=no_basis(stack), teams=teams)
    check_stack(got, stack, basis0=no_basis(stack))
    logs = [[g["log"] for g in got]]
    for rule in RULES:
        got = teamed_run(stack, team, rule, 3, log_cap=8, teams=teams)
        check_run(got, stack, rule, 3)
        logs.append([g["log"] for g in got])
    assert len(spots) == len(stack)
    return logs


def test_leaving_row_in_every_wave():
    """the ratio test's minimum, its first eligible row and the leaving row: the
    row with the smallest ratio in each wave and at both ends of the second
    pass; on the tie the lower row, from another wave, leaves"""
    spots = tm.SPOTS + [min(tm.TIE)]
    for logs in solve_and_run(tm.row_stack(), 3, spots):
        assert logs == [[[r - 1, 0]] for r in spots]


@pytest.mark.parametrize("rule", RULES, ids=["standard", "min_index"])
def test_entering_column_in_every_wave(rule):
    """the most negative cost (standard rule) and the first negative cost
    (min-index rule) in each wave and at both ends of the second pass; on the
    tie the lower column, from another wave, enters"""
    spots = tm.SPOTS + ([min(tm.TIE)] if rule == STANDARD else [])
    logs = solve_and_run(tm.col_stack(rule), 3, spots)
    for of_call in (logs[0], logs[1 + rule]):
        assert of_call == [[[0, c - 1]] for c in spots]
    assert [log[-1] for log in logs[2 - rule]] == [[0, c - 1] for c in spots]


def test_special_cases_in_the_last_waves():
    """test_gpu_batch_team.test_special_cases with the case's rows in the
    workgroup's last two waves and in the ratio test's second pass"""
    m, n, row_at = tm.LONG_EMBEDDING
    assert m > tm.NT and [(r - 1) // 64 for r in row_at] == [tm.WAVES - 1, tm.WAVES - 1, tm.WAVES]
    team_suite.test_special_cases(m, n, row_at)


# ---------------------------------------------------------------------------
# B. widths and heights around the stride of the walk
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("width", tm.WIDE_WIDTHS)
def test_rows_around_the_stride(width):
    """n + 1 = 2 NT - 1, 2 NT, 2 NT + 1, 2 NT + 2: the walk's row step is 1 with
    the largest column step, 1 with none, and 0; an odd width starts LP 1 at an
    odd double and lets pairs straddle the row ends.  run(3) and run(4), so an
    LP comes home from the second buffer or ends in the first, on buffers that
    still hold the runs before."""
    stack = tm.wide_stack(width)
    assert stack.shape[1:] == (3, width) and tm.offsets(stack)[1] % 2 == width % 2
    for team in tm.WIDE_TEAMS:
        eng = make_engine(stack, "device", team, 8)
        try:
            check_plan(eng, [team] * 2)
            for rule in RULES:
                for k in tm.WIDE_RUNS:
                    eng.upload(stack)
                    want = check_run(run_records(eng, rule, k), stack, rule, k)
                    assert all(w["npiv"] >= 1 for w in want) and (rule == STANDARD or want[0]["npiv"] == k)
        finally:
            eng.close()


def test_rows_of_one_pair():
    """n + 1 = 2: the walk steps NT rows and no column"""
    stack = tm.narrow_stack()
    assert stack.shape[1:] == (tm.NT + 4, 2)
    got = teamed_solve(stack, 5, log_cap=8, basis=no_basis(stack), teams=[5] * 2)
    want = check_stack(got, stack, basis0=no_basis(stack))
    assert [w["npiv"] for w in want] == [1, 1]
    for rule in RULES:
        check_run(teamed_run(stack, 5, rule, 3, log_cap=8), stack, rule, 3)


def test_more_rows_than_threads():
    stack = tm.high_stack()
    assert stack.shape[1:] == (tm.NT + 3, 8)
    got = teamed_solve(stack, 3, log_cap=16, basis=no_basis(stack), teams=[3] * 2)
    want = check_stack(got, stack, basis0=no_basis(stack))
    assert all(w["npiv"] >= 2 for w in want)
    for rule in RULES:
        check_run(teamed_run(stack, 3, rule, 3, log_cap=8), stack, rule, 3)


# ---------------------------------------------------------------------------
# C. ranges
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1], ids=["3x3_team4", "4x6_team12"])
def test_a_team_of_one_pair_each(which):
    """team E / 2: ranges of two elements, and on the 3 x 3 LP that starts at
    an odd double a range that is the peeled head alone"""
    stack, team = tm.pair_stacks()[which]
    eng = make_engine(stack, "device", team, 8)
    try:
        check_plan(eng, [team] * 3)
        sizes = [[b - a for a, b in p["ranges"]] for p in eng.team_plan()]
        assert all(2 in s for s in sizes)
        if which == 0:
            assert tm.offsets(stack)[1] % 2 == 1
            assert sizes[1][0] == 1 and 1 not in sizes[0] + sizes[2]       # the head alone
            assert sizes[1] == [1, 2, 2, 4] and sizes[0] == [2, 2, 2, 3]
        else:
            assert sizes == [[2] * 12] * 3
        basis0 = no_basis(stack)
        eng.upload(stack)
        eng.set_basis(basis0)
        want = check_stack(records(eng, *eng.solve(CAP), basis0), stack, basis0=basis0)
        assert all(w["npiv"] >= 1 for w in want)
        for rule in RULES:
            eng.upload(stack)
            check_run(run_records(eng, rule, 2), stack, rule, 2)
    finally:
        eng.close()


@pytest.mark.parametrize("which", [0, 1], ids=["9x19", "41x81"])
def test_the_largest_team(which):
    stack = tm.team_max_stacks()[which]
    basis0 = canonical_basis(stack)
    got = teamed_solve(stack, TEAM_MAX, log_cap=64, basis=basis0, teams=[TEAM_MAX] * len(stack))
    want = check_stack(got, stack, basis0=basis0)
    assert all(w["status"] == cc.OPTIMAL and w["npiv"] >= 2 for w in want)


# ---------------------------------------------------------------------------
# D. the team's LDS above 64 KiB
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("team", [2, TEAM_MAX, 1])
def test_a_pivot_row_above_64k_of_lds(team):
    """2 x 8201: the pivot row alone is above the 64 KiB a kernel gets unasked;
    the row is also eight strides of the walk long"""
    stack = tm.big_row_stack()
    m, n = rc.shape_of(stack[0])
    assert _lib.batch_device_lds_bytes(m, n) == tm.BIG_LDS > 64 * 1024
    eng = make_engine(stack, "device", team, 64)
    try:
        check_plan(eng, [team] * 2)
        for rule in RULES:
            eng.upload(stack)
            want = check_run(run_records(eng, rule, 3), stack, rule, 3)
            assert all(w["npiv"] >= 1 for w in want) and (rule == STANDARD or want[0]["npiv"] == 3)
        basis0 = no_basis(stack)
        eng.upload(stack)
        eng.set_basis(basis0)
        want = check_stack(records(eng, *eng.solve(64), basis0), stack, cap=64, basis0=basis0)
        assert all(w["npiv"] >= 1 for w in want)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# E. more workgroups than the chip holds
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("window", [1, None], ids=["window1", "window_default"])
def test_a_grid_above_residency(window):
    """96 LPs at the largest team: with 512 threads each a CU holds four
    workgroups at the most, the chip 1024, and the launch has 3072; the LPs take
    2 to 12 pivots, so they finish at different launches and in both buffers"""
    stack = tm.full_stack()
    assert len(stack) * TEAM_MAX > tm.RESIDENT
    basis0 = canonical_basis(stack)
    got = teamed_solve(stack, TEAM_MAX, window=window, log_cap=16, basis=basis0, teams=[TEAM_MAX] * len(stack))
    want = check_stack(got, stack, basis0=basis0)
    assert {w["npiv"] % 2 for w in want} == {0, 1} and len({w["npiv"] for w in want}) > 4


# ---------------------------------------------------------------------------
# F. the placed suite's contract sections at a team (test_gpu_batch_device.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,ns,k", cc.DIRTY_SHAPES)
def test_dirty_stacks(m, ns, k):
    stack = cc.dirty_stack(m, ns, k, range(1, 33))
    got = teamed_solve(stack, 3, cap=cc.DIRTY_CAP, log_cap=cc.DIRTY_CAP, teams=[3] * 32)
    want = check_stack(got, stack, cap=cc.DIRTY_CAP, finite=False)
    assert max(w["npiv"] for w in want) < cc.DIRTY_CAP


@pytest.mark.parametrize("name,tol", cc.TOL_SETS, ids=cc.TOL_IDS)
@pytest.mark.parametrize("m,ns,team", [(8, 10, 2), (31, 33, 5)])
def test_each_tolerance_field(m, ns, team, name, tol):
    stack = gen.mixed_stack(m, ns, range(1, 9))
    got = teamed_solve(stack, team, tol=tol, log_cap=512, teams=[team] * 8)
    want = check_stack(got, stack, tol=tol)
    plain = [oracle_solve(T) for T in stack]
    assert any(cc.result_differs(a, b) for a, b in zip(want, plain))
    if name == "zero" and (m, ns) == (31, 33):
        assert [g["status"] for g in got] == [cc.OBJ_INCREASED] * 8


@pytest.mark.parametrize("window", [1, None], ids=["window1", "window_default"])
@pytest.mark.parametrize("padded", [False, True])
def test_stall_field(padded, window):
    """the stall test reads the objective that every workgroup of the team
    computes for itself, not the cell rank 0's owner stores"""
    km = cc.km8_padded() if padded else gen.klee_minty(8)
    m, n = km.shape[0] - 1, km.shape[1] - 1
    stack = np.stack([km, km])
    tol = dict(stall=cc.STALL)
    got = teamed_solve(stack, 3, tol=tol, window=window, log_cap=256, teams=[3, 3])
    check_stack(got, stack, tol=tol)
    assert got[0]["nstd"] == m + n < got[0]["npiv"]
    assert (got[0]["npiv"], got[0]["nstd"]) == ((253, 238) if padded else (89, 24))


@pytest.mark.parametrize("padded", [False, True])
def test_stall_band_edges(padded):
    """test_stall_field's tolerance holds every pivot in the band, where an
    objective read one pivot late counts the same.  Here the band ends between
    the objectives after pivots m + n - 1 and m + n (and at each of the two):
    the counter is reset one short of the switch unless the tolerance is the
    later objective itself"""
    km = cc.km8_padded() if padded else gen.klee_minty(8)
    stack = np.stack([km, km])
    lo, mid, hi = tm.stall_edges(km)
    assert lo < mid < hi
    for stall in (lo, mid, hi):
        tol = dict(stall=stall)
        got = teamed_solve(stack, 3, tol=tol, log_cap=256, teams=[3, 3])
        check_stack(got, stack, tol=tol)
        switched = (253, 238) if padded else (89, 24)
        assert (got[0]["npiv"], got[0]["nstd"]) == (switched if stall == hi else (255, 255))


@pytest.mark.parametrize("down", [False, True], ids=["wide", "denormal"])
@pytest.mark.parametrize("m,ns", cc.SCALED_SHAPES)
def test_scaled_rows(m, ns, down):
    stack = cc.scaled_stack(m, ns, range(1, 5), down)
    got = teamed_solve(stack, 3, tol=cc.SCALE_TOL, log_cap=512, teams=[3] * 4)
    want = check_stack(got, stack, tol=cc.SCALE_TOL)
    assert all(w["status"] == cc.OPTIMAL and w["npiv"] >= 2 for w in want)


# ---------------------------------------------------------------------------
# G. calls not yet made on a teamed batch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES, ids=["standard", "min_index"])
def test_run_on_a_ragged_teamed_batch(rule):
    """lp_batch_run on test_ragged_mix_of_placements_and_teams' mix: run(3)
    brings the teamed LPs home from their second buffer, run(4) goes on from
    there, each against the oracle continued from the call before"""
    lps, teams = tm.ragged_mix()
    eng = _lib.RaggedEngine([rc.shape_of(T) for T in lps], log_cap=16, place="auto", team=teams)
    try:
        check_plan(eng, teams)
        eng.upload(lps)
        first = check_run(run_records(eng, rule, 3), lps, rule, 3)
        assert sum(w["npiv"] == 3 for w, g in zip(first, teams) if g > 1) >= 3
        second = check_run(run_records(eng, rule, 4), [w["T"] for w in first], rule, 4)
        assert sum(w["npiv"] == 4 for w, g in zip(second, teams) if g > 1) >= 3
    finally:
        eng.close()


def test_an_engine_without_a_log():
    stack = gen.mixed_stack(8, 10, range(1, 5))
    logged = teamed_solve(stack, 3, log_cap=16, teams=[3] * 4)
    check_stack(logged, stack)
    bare = teamed_solve(stack, 3, log_cap=0, teams=[3] * 4)
    for a, b in zip(bare, logged):
        assert a["log"] == [] and b["log"]
        check(a, dict(b, log=[]))
    for rule in RULES:
        logged = teamed_run(stack, 3, rule, 5, log_cap=16)
        check_run(logged, stack, rule, 5)
        for a, b in zip(teamed_run(stack, 3, rule, 5, log_cap=0), logged):
            assert a["log"] == [] and b["log"]
            check(a, dict(b, log=[]))


def test_a_capped_solve_continued():
    """solve(51) ends on an odd count, in the second buffer; the second solve
    goes on from the tableau that came home"""
    stack = tm.continued_stack()
    basis0 = canonical_basis(stack)
    eng = _lib.BatchEngine(2, 100, 200, log_cap=256, place="auto", team="auto")
    try:
        g = eng.team_of(0)
        assert g > 1
        check_plan(eng, [g, g])
        eng.upload(stack)
        eng.set_basis(basis0)
        capped = records(eng, *eng.solve(tm.CONTINUED_CAP), basis0)
        a = check_stack(capped, stack, cap=tm.CONTINUED_CAP, basis0=basis0)
        assert [(w["status"], w["npiv"]) for w in a] == [(cc.CAP_REACHED, tm.CONTINUED_CAP)] * 2
        mid = [w["T"] for w in a]
        basis1 = [c["basis"] for c in capped]
        b = check_stack(records(eng, *eng.solve(CAP), basis0), mid, basis0=basis1)
        assert [w["status"] for w in b] == [cc.OPTIMAL] * 2 and b[0]["npiv"] == 165
    finally:
        eng.close()
