"""The inputs of the dual-rule and warm re-solve GPU tests do, on the oracle
alone, what their names say (tests/_dual_cases.py; no GPU, nothing from the
device): the perturbed right-hand sides need dual pivots, some end infeasible,
the warm optimum is the cold one, and each constructed tableau meets the clause
of the rule it was built for."""
import numpy as np
import pytest

import _dual_cases as dc
import _problem_cases as pc
import _twophase_cases as tc
import lpsol_amd
from lpsol_amd import _lib
from lpsol_amd import generators as gen
from lpsol_amd.problem import assemble_tableaux
from oracle import phase1
from oracle.f64 import F64Tableau

REL = 1e-9          # the project's objective tolerance (README)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def test_rule_value_is_exported():
    assert _lib.RULE_DUAL == dc.DUAL == 3 and lpsol_amd.RULE_DUAL == 3
    assert "RULE_DUAL" in lpsol_amd.__all__
    assert len({_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX, _lib.RULE_MAX_INCREASE, _lib.RULE_DUAL}) == 4


@pytest.mark.parametrize("shape,seeds,least", [(dc.SMALL, dc.SMALL_SEEDS, 16), (dc.LARGE, dc.LARGE_SEEDS, 16)],
                         ids=["8x10", "40x40"])
def test_scaled_right_hand_sides_need_dual_pivots_and_reach_the_cold_optimum(shape, seeds, least):
    """a quarter of the 64 small LPs, half of the 32 large ones"""
    need = 0
    for s in seeds:
        wm = dc.warm(*shape, s, "scale")
        assert (wm["b"] >= 0).all()
        assert not dc.dual_infeasible(wm["T"], dc.DEFAULT_TOL)          # row 0 did not change
        assert dc.same_bits(wm["T"][:, 1:], wm["opt"][:, 1:])
        w = dc.walk(wm["T"])
        assert w["status"] == _lib.OPTIMAL and w["npiv"] <= 68, s
        need += w["npiv"] > 0
        cold = F64Tableau(wm["T0"])
        st, log, _ = cold.solve()
        assert st == _lib.OPTIMAL
        assert rel(-w["T"][0, 0], cold.objective()) <= REL, s
    assert need >= least, need


@pytest.mark.parametrize("shape,seeds", [(dc.SMALL, dc.SMALL_SEEDS), (dc.LARGE, dc.LARGE_SEEDS)], ids=["8x10", "40x40"])
def test_shifted_right_hand_sides_agree_with_phase_1(shape, seeds):
    fates, most = [], 0
    for s in seeds:
        wm = dc.warm(*shape, s, "shift")
        w = dc.walk(wm["T"])
        cold = phase1.solve_lp(wm["T0"], report=True)
        assert w["status"] in (_lib.OPTIMAL, _lib.INFEASIBLE), s
        assert (w["status"] == _lib.INFEASIBLE) == (cold["status"] == phase1.INFEASIBLE), s
        if w["status"] == _lib.OPTIMAL:
            assert cold["status"] == _lib.OPTIMAL and rel(-w["T"][0, 0], cold["objective"]) <= REL, s
        fates.append(w["status"])
        most = max(most, w["npiv"])
    assert any((dc.warm(*shape, s, "shift")["b"] < 0).any() for s in seeds)
    assert _lib.INFEASIBLE in fates and _lib.OPTIMAL in fates and most >= 3


def test_the_original_right_hand_side_gives_back_the_optimal_column():
    for s in (1, 2, 3):
        T0 = gen.tableau("mixed", *dc.SMALL, s)
        o = F64Tableau(T0)
        o.solve()
        back = dc.set_rhs(o.T, dc.slack_table([_lib.SENSE_LE] * dc.SMALL[0], dc.SMALL[1]), T0[:, 0])
        assert np.allclose(back[:, 0], o.T[:, 0], rtol=0, atol=1e-12)       # M . b, summed in another order
        assert dc.walk(back)["npiv"] == 0


def first(name, tol=None):
    w = dc.walk(dc.CASES[name], dc.CAP, tol)
    return w["status"], w["log"]


def test_constructed_cases_do_what_their_names_say():
    assert first("row_tie") == first("row_tie", dict(cost_tie=0.0)) == (_lib.OPTIMAL, [[0, 0]])
    assert first("row_band")[1][0] == [0, 0] and first("row_band", dict(cost_tie=0.0))[1][0] == [1, 0]
    assert first("col_tie")[1][0] == [0, 0] and first("col_tie", dict(ratio_tie=0.0))[1][0] == [0, 0]
    assert first("col_band_in")[1][0] == [0, 0] and first("col_band_in", dict(ratio_tie=0.0))[1][0] == [0, 1]
    assert first("col_band_out")[1][0] == [0, 1]
    assert first("cost_clamp")[1][0] == [0, 0] and first("cost_clamp", dict(cost=0.0))[1][0] == [0, 1]
    assert first("a_small")[1][0] == [0, 1]
    assert first("b_small") == (_lib.OPTIMAL, [])
    assert first("infeasible") == (_lib.INFEASIBLE, [[1, 0]])
    assert first("infeasible_now") == (_lib.INFEASIBLE, [])
    assert first("neg_cost") == (_lib.BAD_ARG, []) and dc.same_bits(dc.walk(dc.NEG_COST)["T"], dc.NEG_COST)
    assert first("nan_cell")[1][0] == [0, 1] and np.isnan(dc.walk(dc.NAN_CELL)["T"][:, 1]).all()
    assert first("nan_ratio") == (_lib.BAD_PIVOT, []) and first("neg_inf_b") == (_lib.BAD_PIVOT, [])
    for name in ("infeasible_now", "nan_ratio", "neg_inf_b", "b_small"):       # no pivot applied
        assert dc.same_bits(dc.walk(dc.CASES[name])["T"], dc.CASES[name]), name


def test_caps():
    T = dc.warm(*dc.LARGE, 1, "scale")["T"]
    whole = dc.walk(T)
    assert whole["npiv"] >= 3
    assert (dc.walk(T, 0)["status"], dc.walk(T, 0)["npiv"]) == (_lib.PIVOTED, 0)
    two = dc.walk(T, 2)
    assert (two["status"], two["log"]) == (_lib.PIVOTED, whole["log"][:2])
    rest = dc.walk(two["T"])                     # a second call goes on where the first stopped
    assert two["log"] + rest["log"] == whole["log"] and dc.same_bits(rest["T"], whole["T"])
    assert dc.walk(dc.NEG_COST, 0)["status"] == _lib.BAD_ARG        # the start check comes before the cap


@pytest.mark.parametrize("m,n", dc.EDGE_ROWS + dc.EDGE_COLS)
def test_edge_lps_pivot_on_the_last_row_and_column(m, n):
    T = dc.edge_lp(m, n)
    assert not dc.dual_infeasible(T, dc.DEFAULT_TOL)
    assert [i for i in range(1, m + 1) if T[i, 0] < 0] == [m]
    assert [j for j in range(1, n + 1) if T[m, j] < 0] == [n]
    w = dc.walk(T)
    assert (w["status"], w["log"]) == (_lib.OPTIMAL, [[m - 1, n - 1]])
    assert (w["T"][:m, 0] != T[:m, 0]).all()           # the pivot changes every row


# ---------------------------------------------------------------------------
# the inputs of test_gpu_batch_dual_edges.py
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", dc.LATER_LDS + dc.LATER_DEV)
def test_later_trip_lps_pivot_on_the_last_row_and_column(m, n):
    """above the one-wave bound, and the last row or column is past the first trip of a lane: past 256
    for the LDS shapes, past 1024 for the device-placed ones"""
    T = dc.edge_lp(m, n)
    NT = 256 if (m, n) in dc.LATER_LDS else 1024
    assert dc.elems(T) > dc.ONE_WAVE_ELEMS and max(m, n) > NT
    assert not dc.dual_infeasible(T, dc.DEFAULT_TOL)
    assert [i for i in range(1, m + 1) if T[i, 0] < 0] == [m]
    assert [j for j in range(1, n + 1) if T[m, j] < 0] == [n]
    w = dc.walk(T)
    assert (w["status"], w["log"]) == (_lib.OPTIMAL, [[m - 1, n - 1]])
    assert (w["T"][:m, 0] != T[:m, 0]).all()


def test_later_trip_shapes_cover_both_loops_of_both_kernels():
    for shapes, NT in ((dc.LATER_LDS, 256), (dc.LATER_DEV, 1024)):
        assert any(n > NT and m < 64 for m, n in shapes) and any(m > NT and n < 64 for m, n in shapes)
        assert any(max(m, n) > 2 * NT for m, n in shapes)           # a third trip


@pytest.mark.parametrize("group", list(dc.LANE_GROUPS))
def test_lane_cases_put_two_candidates_into_one_lane(group):
    NT, place, cols, rows = dc.LANE_GROUPS[group]
    cases = dc.lane_cases(group)
    width = {"nt64": 1, "nt256_one_wave": 1, "nt256": 4}.get(group)         # the waves of the LDS kernel
    for name, (T, *want) in cases.items():
        assert dc.shape_of(T) == (cols if name.startswith("col") else rows)
        if place == "lds":
            assert (dc.elems(T) <= dc.ONE_WAVE_ELEMS) == (width == 1), name
        assert not dc.dual_infeasible(T, dc.DEFAULT_TOL)
        for tol, first in zip(dc.LANE_TOLS, want):
            one = dc.walk(T, 1, tol)
            assert (one["status"], one["log"]) == (_lib.PIVOTED, [first]), (name, tol)
            whole = dc.walk(T, dc.CAP, tol)
            assert whole["status"] == _lib.OPTIMAL and whole["log"][0] == first and whole["npiv"] <= 4, (name, tol)
    # what each pair is: the same lane of a kernel NT wide for tie and band, two lanes past their first trip else
    lo, hi = dc.LANE_LO, dc.LANE_LO + NT
    for kind in ("col", "row"):
        tie, band, lanes = (cases[f"{kind}_{k}"] for k in ("tie", "band", "lanes"))
        at = 1 if kind == "col" else 0
        assert tie[1][at] == band[1][at] == lo - 1 and (hi - lo) % NT == 0
        moved = band[2] if kind == "col" else band[3]
        assert moved[at] == hi - 1 and moved != band[1]           # the exact minimum is the later one
        assert tie[2] == tie[3] == tie[1]                           # a tie is a tie under either tolerance
        assert lanes[1][at] == NT + 5 and (NT + 10 - (NT + 5)) % NT != 0


def test_lane_bands_are_inside_the_default_tolerance_and_outside_zero():
    T = dc.lane_cases("nt64")["col_band"][0]
    lo, hi = T[0, dc.LANE_LO], T[0, dc.LANE_LO + 64]
    assert hi < lo <= hi + dc.DEFAULT_TOL["ratio_tie"] * hi and T[0, 1:].min() == hi
    T = dc.lane_cases("nt64")["row_band"][0]
    lo, hi = T[dc.LANE_LO, 0], T[dc.LANE_LO + 64, 0]
    assert hi < lo <= hi + dc.DEFAULT_TOL["cost_tie"] * abs(hi) and T[1:, 0].min() == hi


def test_each_tolerance_field_moves_an_outcome_in_both_directions():
    def got(name, **tol):
        w = dc.walk(dc.TOL_CASES[name], dc.CAP, tol or None)
        return w["status"], w["log"]
    # zero: b = -1e-10 takes part only at 0; b = -0.5 no longer at 1
    assert got("b_small") == (_lib.OPTIMAL, []) and got("b_small", zero=0.0) == (_lib.OPTIMAL, [[0, 0]])
    assert got("b_half") == (_lib.OPTIMAL, [[0, 0]]) and got("b_half", zero=1.0) == (_lib.OPTIMAL, [])
    # pivot: -1e-10 is eligible only at 0; -0.5 no longer at 1, -2 no longer at 4
    assert got("a_small")[1][0] == [0, 1] and got("a_small", pivot=0.0)[1][0] == [0, 0]
    assert got("pivot_steps") == (_lib.OPTIMAL, [[0, 0]])
    assert got("pivot_steps", pivot=1.0) == (_lib.OPTIMAL, [[0, 1]])
    assert got("pivot_steps", pivot=4.0) == (_lib.INFEASIBLE, [])
    # cost at the start: -1e-10 is dual feasible at the default alone; -1 from 1 up
    assert got("cost_small") == (_lib.OPTIMAL, [[0, 0]])
    assert got("cost_small", cost=0.0) == got("cost_small", cost=1e-11) == (_lib.BAD_ARG, [])
    assert dc.same_bits(dc.walk(dc.COST_SMALL, dc.CAP, dict(cost=0.0))["T"], dc.COST_SMALL)      # nothing applied
    assert got("neg_cost") == (_lib.BAD_ARG, []) and got("neg_cost", cost=2.0) == (_lib.OPTIMAL, [[0, 0]])


def test_the_tolerance_table_is_the_walk():
    """TOL_WANT states a case under the default and every set of its own field; the GPU test reads it"""
    for name, T in dc.TOL_CASES.items():
        stated = 0
        for tol in dc.FIELD_TOLS:
            want = dc.tol_want(name, tol)
            if want is not None:
                w = dc.walk(T, dc.CAP, tol)
                assert (w["status"], w["log"]) == want, (name, tol)
                stated += 1
        assert stated >= 3 and len(set(map(str, dc.TOL_WANT[name].values()))) >= 2, name
    assert len(dc.FIELD_TOLS) == len(dc.FIELD_TOL_IDS)
    for field in ("zero", "pivot", "cost"):
        values = [t[field] for t in dc.FIELD_TOLS if t and field in t]
        assert 0.0 in values and max(values) > dc.DEFAULT_TOL[field]


# ---------------------------------------------------------------------------
# the inputs of test_gpu_batch_rhs_edges.py
# ---------------------------------------------------------------------------

def assembled(items):
    blocks = [np.vstack([np.concatenate([[0.0], c]), np.c_[b, A]]) for c, A, b, _ in items]
    return assemble_tableaux(blocks, [s for *_, s in items])


def test_block_problems_cross_workgroups_where_they_say():
    items = dc.block_problems()
    assert len(items) == dc.BLOCK_WINDOWS[0][1] and len(items[dc.BLOCK_BIG][2]) == 260
    for first, count in dc.BLOCK_WINDOWS:
        assert 0 <= first and first + count <= len(items)
    whole = dc.lane_starts(items, 0, len(items))
    assert whole[-1] >= 600 and whole[-1] > 2 * dc.FLAT
    for first, edges in dc.BLOCK_EDGES.items():
        count = next(c for f, c in dc.BLOCK_WINDOWS if f == first)
        starts = dc.lane_starts(items, first, count)
        assert set(edges) <= set(starts) and starts[-1] > 2 * dc.FLAT, first
    big = whole[dc.BLOCK_BIG]
    assert big // dc.FLAT != (big + 260) // dc.FLAT                 # its rows lie in two workgroups
    assert dc.lane_starts(items, dc.BLOCK_BIG, 1)[-1] > dc.FLAT     # alone, too
    assert dc.FLAT <= whole[125] and whole[126] <= 2 * dc.FLAT      # LP 125 lies wholly in the second
    senses = np.concatenate([s for *_, s in items])
    assert (senses == _lib.SENSE_GE).sum() >= 30 and (senses == _lib.SENSE_LE).sum() >= 30
    assert not (senses == _lib.SENSE_EQ).any()


def test_block_problems_end_optimal_with_every_row_live():
    for i, T in enumerate(assembled(dc.block_problems())):
        o = tc.report(T, None, tc.PROBE_CAP)
        assert (o["status"], o["rows"]) == (tc.OPTIMAL, T.shape[0] - 1), i


def test_uniform_block_windows_cross_a_workgroup_with_first_above_zero():
    u = dc.UNIFORM_BLOCKS
    lanes = u["m"] + 1
    assert dc.FLAT % lanes != 0 and u["B"] * lanes > 2 * dc.FLAT
    first, count = u["windows"][1]
    assert first > 0 and count * lanes > dc.FLAT and first + count == u["B"]
    first, count = u["windows"][2]
    assert first * lanes < dc.FLAT < (first + count) * lanes        # the two LPs around lane 256 of the whole batch


def test_the_unbounded_lp_is_unbounded_and_keeps_a_negative_cost():
    c, A, b = dc.unbounded_parts()
    slack = dc.slack_table([_lib.SENSE_LE] * 3, 5)
    for i in range(len(c)):
        T = assemble_tableaux(np.vstack([np.concatenate([[0.0], c[i]]), np.c_[b[i], A[i]]])[None], ["<="] * 3)[0]
        o = F64Tableau(T)
        st, _, _ = o.solve()
        assert st == (_lib.UNBOUNDED if i == dc.UNBOUNDED_AT else _lib.OPTIMAL), i
        w = dc.walk(dc.set_rhs(o.T, slack, np.concatenate([[0.0], 0.5 * b[i]])))
        if i == dc.UNBOUNDED_AT:            # row 0 keeps a cost below -tol.cost: the dual rule is not defined
            assert (o.T[0, 1:] < -dc.DEFAULT_TOL["cost"]).any() and (w["status"], w["npiv"]) == (_lib.BAD_ARG, 0)
        else:
            assert w["status"] == _lib.OPTIMAL


def test_the_infeasible_block_ends_phase_1_with_every_row_live():
    for i, T in enumerate(assembled(dc.infeasible_problems())):
        o = tc.report(T, None, tc.PROBE_CAP)
        assert o["rows"] == T.shape[0] - 1, i
        assert o["status"] == (tc.INFEASIBLE if i == dc.INFEASIBLE_AT else tc.OPTIMAL), i


def test_only_the_dependent_lp_loses_a_row():
    assert (dc.DEPENDENT[2:, 3:] == 0).all() and dc.same_bits(dc.DEPENDENT[2], dc.DEPENDENT[3])
    for stack in (list(dc.short_uniform()), dc.short_ragged()):
        for i, T in enumerate(stack):
            m, n = dc.shape_of(T)
            assert n > m            # ns = n - m >= 1 under m senses that are all <=
            o = tc.report(T, None, tc.PROBE_CAP)
            assert o["status"] == tc.OPTIMAL and (o["rows"] == m - 1 if i == dc.SHORT_AT else o["rows"] == m), i
    assert len({T.shape for T in dc.short_ragged()}) == 3
    o = tc.report(dc.full_rank(), None, tc.PROBE_CAP)
    assert dc.full_rank().shape == dc.DEPENDENT.shape and (o["status"], o["rows"]) == (tc.OPTIMAL, 3)


# the status of run(RULE_DUAL) after each extreme right-hand side, LP by LP: +inf leaves no negative b on the
# small LP 0 and makes -inf cells on the large one; -inf is LP_BAD_PIVOT; a NaN takes no part
EXTREME_STATUS = dict(
    small=[_lib.OPTIMAL, _lib.BAD_PIVOT, _lib.OPTIMAL, _lib.OPTIMAL, _lib.OPTIMAL, _lib.OPTIMAL, _lib.OPTIMAL,
           _lib.OPTIMAL, _lib.BAD_PIVOT, _lib.OPTIMAL, _lib.OPTIMAL, _lib.OPTIMAL, _lib.BAD_PIVOT, _lib.OPTIMAL],
    large=[_lib.BAD_PIVOT, _lib.BAD_PIVOT, _lib.OPTIMAL, _lib.OPTIMAL, _lib.OPTIMAL, _lib.BAD_PIVOT, _lib.OPTIMAL])


@pytest.mark.parametrize("which", list(dc.EXTREME_BATCHES))
def test_extreme_right_hand_sides_on_the_oracle(which):
    (m, ns), B, _ = dc.EXTREME_BATCHES[which]
    assert B >= len(dc.EXTREME) and m >= 5
    got = dc.extreme_host(which)
    assert [dc.walk(T)["status"] for T, _ in got] == EXTREME_STATUS[which] == dc.EXTREME_STATUS[which]
    col = lambda k: [T[:, 0] for i, (T, _) in enumerate(got) if dc.EXTREME[i % 7] == k]
    assert all(np.isinf(c).any() for c in col("+inf")) and all(np.isnan(c).any() for c in col("nan"))
    assert all((c == -np.inf).any() or np.isnan(c).any() for c in col("-inf"))
    assert all(dc.walk(T)["status"] == _lib.BAD_PIVOT for i, (T, _) in enumerate(got) if dc.EXTREME[i % 7] == "-inf")
    assert any(np.isinf(c).any() for c in col("1e308 twice"))       # finite products, an infinite sum
    for i, (T, rhs) in enumerate(got):
        if dc.EXTREME[i % 7] == "1e308 twice":
            assert (rhs == 1e308).sum() == 2
        if dc.EXTREME[i % 7] == "-0.0":
            assert np.signbit(rhs[[0, 1, 4]]).all() and not rhs[[0, 1, 4]].any()
        if dc.EXTREME[i % 7] in ("5e-324", "1e-320"):
            assert ((rhs > 0) & (rhs < 2.3e-308)).sum() == 1        # a denormal went in


def test_the_ge_lps_of_the_log_test_take_phase_1_pivots():
    for seed in range(1, 17):
        T, _, _ = pc.lp("ge", 8, 10, seed)
        o = tc.report(T, None, tc.PROBE_CAP)
        assert o["status"] == tc.OPTIMAL and o["nart"] >= 1, seed


def test_the_field_tolerance_walks_fit_the_log():
    """under FIELD_CAP = LOG_CAP the whole log of every LP is kept; one walk reaches the cap: with every cost
    clamped to ratio 0 (cost = 2) the second 41 x 81 LP goes round, and ends 'pivoted' there"""
    assert dc.FIELD_CAP == dc.LOG_CAP
    capped = []
    for tol in dc.FIELD_TOLS:
        for i, T in enumerate(dc.field_lps()):
            w = dc.walk(T, dc.FIELD_CAP, tol)
            if w["status"] == _lib.PIVOTED:
                capped.append((dc.tol_key(tol), T.shape))
    assert capped == [((("cost", 2.0),), (41, 81))]
    for name, T in dc.TOL_CASES.items():            # the stated outcomes are far below the cap
        assert all(dc.walk(T, dc.FIELD_CAP, tol)["npiv"] <= 2 for tol in dc.FIELD_TOLS), name
