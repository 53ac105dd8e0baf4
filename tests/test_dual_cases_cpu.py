"""The inputs of the dual-rule and warm re-solve GPU tests do, on the oracle
alone, what their names say (tests/_dual_cases.py; no GPU, nothing from the
device): the perturbed right-hand sides need dual pivots, some end infeasible,
the warm optimum is the cold one, and each constructed tableau meets the clause
of the rule it was built for."""
import numpy as np
import pytest

import _dual_cases as dc
import lpsol_amd
from lpsol_amd import _lib
from lpsol_amd import generators as gen
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
