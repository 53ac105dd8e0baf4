"""The inputs of test_gpu_batch_team_edges.py still reach what they are there
for (tests/_team_cases.py): the oracle alone puts each pivot row and column
where the case says, performs the pivots the case counts on, and ends each LP
after the count the case needs.  The contract stacks that file reuses are
checked in test_contract_cpu.py.  No GPU."""
import numpy as np
import pytest

import _contract_cases as cc
import _team_cases as tm
from lpsol_amd import _lib
from lpsol_amd import generators as gen

NT, STANDARD, MIN_INDEX = tm.NT, tm.STANDARD, tm.MIN_INDEX


def test_the_shapes_follow_the_knobs():
    assert tm.WAVES in (4, 8, 16) and NT == 64 * tm.WAVES and tm.TEAM_MAX >= 2 and tm.WINDOW > 1
    spots = tm.SPOTS
    assert len(spots) == tm.WAVES + 2 and spots == sorted(spots)
    assert [(s - 1) // 64 for s in spots[:tm.WAVES]] == list(range(tm.WAVES))       # thread s - 1: one spot per wave
    assert len({(s - 1) % 64 for s in spots[:tm.WAVES]}) == tm.WAVES                # at a lane of its own
    assert spots[-2:] == [NT + 1, tm.LONG] and tm.LONG < 2 * NT                     # the second pass, its ends
    hi, lo = tm.TIE
    assert lo < hi and (lo - 1) // 64 != (hi - 1) // 64 and {lo, hi} <= set(spots)
    if (tm.WAVES, tm.TEAM_MAX) == (8, 32):
        assert spots == [1, 72, 143, 214, 285, 356, 427, 498, 513, 576] and tm.TIE == (427, 143)


# ---------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------

def test_row_lps_leave_at_their_spot():
    stack = tm.row_stack()
    assert stack.shape == (len(tm.SPOTS) + 1, tm.LONG + 1, 5)
    for T, r in zip(stack, tm.SPOTS + [min(tm.TIE)]):
        w = tm.oracle_solve(T)
        assert (w["status"], w["log"], w["nstd"]) == (cc.OPTIMAL, [[r - 1, 0]], 1)
        for rule in tm.RULES:
            w = tm.oracle_run(T, rule, 3)
            assert (w["status"], w["log"]) == (cc.OPTIMAL, [[r - 1, 0]])


def test_column_lps_enter_at_their_spot():
    for rule in tm.RULES:
        stack = tm.col_stack(rule)
        assert stack.shape == (len(tm.SPOTS) + (rule == STANDARD), 4, tm.LONG + 1)
        for T, c in zip(stack, tm.SPOTS + [min(tm.TIE)]):
            w = tm.oracle_solve(T)                      # the solve starts with the standard rule; on the
            assert (w["status"], w["log"]) == (cc.OPTIMAL, [[0, c - 1]])    # min-index LPs its tie band is c..n
            w = tm.oracle_run(T, rule, 3)
            assert (w["status"], w["log"]) == (cc.OPTIMAL, [[0, c - 1]])
            other = tm.oracle_run(T, 1 - rule, 3)
            assert other["status"] == cc.OPTIMAL and other["log"][-1] == [0, c - 1]
    tie = tm.col_lp(STANDARD, *tm.TIE)
    assert tie[0, tm.TIE[0]] == tie[0, tm.TIE[1]] == -2.0 and np.count_nonzero(tie[0] == -2.0) == 2


def test_the_contract_cases_in_the_last_waves():
    m, n, row_at = tm.LONG_EMBEDDING
    assert [(r - 1) // 64 for r in row_at] == [tm.WAVES - 1, tm.WAVES - 1, tm.WAVES]
    if tm.WAVES == 8:
        assert (m, n, row_at) == (576, 40, (450, 500, 576))
    for c in cc.CASES:
        T = cc.embed(c, m, n, row_at)
        w = tm.oracle_solve(T, c["cap"], c["tol"])
        assert w["status"] == c["status"] and w["log"] == cc.mapped_log(c, row_at), c["name"]
        assert w["nstd"] == c["nstd"] and cc.same_values(w["T"], T) == c["untouched"], c["name"]


# ---------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------

def test_wide_rows_pivot_at_every_width():
    """the min-index rule makes every pivot asked for; the standard rule makes
    at least one and is optimal after the first at most inputs, so run(3) and
    run(4) of either rule end LPs in either buffer"""
    assert tm.WIDE_WIDTHS == [2 * NT - 1, 2 * NT, 2 * NT + 1, 2 * NT + 2]
    ends = set()
    for width in tm.WIDE_WIDTHS:
        stack = tm.wide_stack(width)
        assert stack.shape == (2, 3, width)
        assert tm.offsets(stack)[1] % 2 == width % 2            # E odd: LP 1 starts at an odd double
        for T in stack:
            assert tm.oracle_run(T, MIN_INDEX, 5)["npiv"] == 5
            for k in tm.WIDE_RUNS:
                assert tm.oracle_run(T, MIN_INDEX, k)["npiv"] == k
                assert 1 <= tm.oracle_run(T, STANDARD, k)["npiv"] <= k
                ends |= {tm.oracle_run(T, rule, k)["npiv"] % 2 for rule in tm.RULES}
    assert ends == {0, 1}
    assert {2 * NT // w for w in tm.WIDE_WIDTHS} == {0, 1} and 2 * NT % tm.WIDE_WIDTHS[1] == 0


def test_narrow_and_high():
    narrow = tm.narrow_stack()
    assert narrow.shape == (2, NT + 4, 2) and narrow[0].size % 2 == 0
    assert [tm.oracle_solve(T)["npiv"] for T in narrow] == [1, 1]
    high = tm.high_stack()
    assert high.shape == (2, NT + 3, 8)
    want = [tm.oracle_solve(T) for T in high]
    assert [w["status"] for w in want] == [cc.OPTIMAL] * 2
    if NT == 512:
        assert [w["npiv"] for w in want] == [5, 6]
    # leaving rows in the ratio test's first pass only: the second pass has to lose to them
    assert all(2 <= w["npiv"] and max(r for r, _ in w["log"]) < NT for w in want)


# ---------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------

def test_the_largest_teams_fit_their_lps():
    for stack, team in tm.pair_stacks():
        assert team == stack[0].size // 2 <= tm.TEAM_MAX
        assert all(tm.oracle_solve(T)["npiv"] >= 1 for T in stack)
    small = tm.pair_stacks()[0][0]
    assert small.shape == (3, 3, 3) and tm.offsets(small)[1] % 2 == 1
    for stack in tm.team_max_stacks():
        assert stack[0].size // 2 >= tm.TEAM_MAX
        want = [tm.oracle_solve(T) for T in stack]
        assert all(w["status"] == cc.OPTIMAL and w["npiv"] >= 2 for w in want)
    nine = tm.team_max_stacks()[0]
    assert nine.shape[1:] == (9, 19) and {tm.oracle_solve(T)["npiv"] % 2 for T in nine} == {0, 1}


# ---------------------------------------------------------------------------
# D
# ---------------------------------------------------------------------------

def test_the_big_row_is_above_64k_of_lds():
    stack = tm.big_row_stack()
    assert stack.shape == (2, 2, tm.BIG_ROW + 1)
    assert _lib.batch_device_lds_bytes(1, tm.BIG_ROW) == tm.BIG_LDS > 64 * 1024
    assert _lib.batch_device_lds_bytes(1, tm.BIG_ROW - 27) <= 64 * 1024     # m + n > 8174
    assert not _lib.placed_too_large(_lib.PLACE_DEVICE, 1, tm.BIG_ROW)
    assert [tm.oracle_run(T, MIN_INDEX, 5)["npiv"] for T in stack] == [5, 4]
    for T in stack:
        assert tm.oracle_run(T, MIN_INDEX, 3)["npiv"] == 3
        assert tm.oracle_run(T, STANDARD, 3)["npiv"] >= 1 and tm.oracle_solve(T, 64)["npiv"] >= 1


# ---------------------------------------------------------------------------
# E
# ---------------------------------------------------------------------------

def test_the_full_grid_ends_at_different_launches():
    stack = tm.full_stack()
    assert len(stack) * tm.TEAM_MAX > tm.RESIDENT and stack[0].size // 2 >= tm.TEAM_MAX
    want = [tm.oracle_solve(T) for T in stack]
    p = [w["npiv"] for w in want]
    assert {w["status"] for w in want} == {cc.OPTIMAL}
    assert (min(p), max(p), sum(x % 2 for x in p)) == (2, 12, 56)
    if (NT, tm.TEAM_MAX) == (512, 32):
        assert len(stack) * tm.TEAM_MAX == 3072 and tm.RESIDENT == 1024


# ---------------------------------------------------------------------------
# F
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("padded", [False, True])
def test_the_stall_band_decides_the_switch(padded):
    km = cc.km8_padded() if padded else gen.klee_minty(8)
    assert km[0, 0] == 0.0                                      # z0 = 0: the band is the tolerance itself
    lo, hi = tm.stall_band(km)
    assert (lo, hi) == ((374665.0, 374985.0) if padded else (19000.0, 21000.0))
    z = [abs(tm.oracle_solve(km, k)["z"]) for k in range(km.shape[0] + km.shape[1])]
    assert all(a < b for a, b in zip(z, z[1:]))                 # every pivot moves the objective
    switched = (253, 238) if padded else (89, 24)
    for stall in tm.stall_edges(km):
        w = tm.oracle_solve(km, tol=dict(stall=stall))
        assert (w["status"], w["npiv"], w["nstd"]) == (cc.OPTIMAL,) + (switched if stall == hi else (255, 255))


# ---------------------------------------------------------------------------
# G
# ---------------------------------------------------------------------------

def test_the_ragged_mix_runs_three_then_four():
    lps, teams = tm.ragged_mix()
    assert sorted(set(teams)) == [1, 2, 3, 5, 7] and len(lps) == len(teams)
    toff = tm.offsets(lps)
    assert {toff[i] % 2 for i, g in enumerate(teams) if g > 1} == {0, 1}
    for rule in tm.RULES:
        first = [tm.oracle_run(T, rule, 3) for T in lps]
        second = [tm.oracle_run(w["T"], rule, 4) for w in first]
        for g, a, b in zip(teams, first, second):
            if g > 1 and a["status"] == cc.PIVOTED:
                assert (a["npiv"], b["npiv"]) == (3, 4)         # home from the second buffer, then on from there
        assert sum(a["status"] == cc.PIVOTED for g, a in zip(teams, first) if g > 1) >= 3


def test_the_capped_solve_ends_in_the_second_buffer():
    stack = tm.continued_stack()
    assert all(cc.same_bits(T, gen.tableau("mixed", 100, 100, s)) for T, s in zip(stack, (1, 2)))
    assert tm.CONTINUED_CAP % 2 == 1
    more = []
    for T in stack:
        a = tm.oracle_solve(T, tm.CONTINUED_CAP)
        assert (a["status"], a["npiv"]) == (cc.CAP_REACHED, tm.CONTINUED_CAP)
        b = tm.oracle_solve(a["T"])
        assert b["status"] == cc.OPTIMAL and cc.same_bits(b["T"], tm.oracle_solve(T)["T"])
        more.append(b["npiv"])
    assert more == [165, 184]
