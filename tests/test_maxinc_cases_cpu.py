"""The inputs of test_gpu_batch_maxinc.py do on the oracle what their names
claim, so that no GPU test of the max-increase rule can pass vacuously; and the
front-end checks of the rule that need no device.  Every expected value below
is what oracle/lp_f64.c (lpf_find_max_increase, lpf_find, lpf_pivot) gives."""
import numpy as np
import pytest

import _maxinc_cases as mc
import lpsol_amd
from lpsol_amd import _lib, solve_batch, solve_ragged
from lpsol_amd import generators as gen
from oracle.f64 import F64Tableau


def find(T, tol=None):
    with np.errstate(all="ignore"):
        return F64Tableau(T, tol).find_max_increase()


def test_exact_tie_takes_the_first_column():
    # columns 0 and 2 both give 2 * 4 = 8, column 1 gives 4
    assert find(mc.TIE) == (0, 0)


def test_tie_band():
    assert find(mc.BAND_IN) == (0, 0)                           # 8 - 4e-12 is inside 8 - 1e-12 * 8
    assert find(mc.BAND_IN, dict(ratio_tie=0.0)) == (1, 2)
    assert find(mc.BAND_OUT) == (1, 2)                          # 8 - 4e-10 is not


def test_differs_from_the_standard_rule():
    assert F64Tableau(mc.NOT_STANDARD).find(0) == (0, 0)        # the most negative cost: 3 * 1
    assert find(mc.NOT_STANDARD) == (1, 1)                      # the largest increase: 2 * 9


def test_tol_cost_decides_who_takes_part():
    assert find(mc.TOL_COST) == (1, 1)                          # c_0 = -1e-10 is not negative
    assert find(mc.TOL_COST, dict(cost=0.0)) == (0, 0)          # now it is: 1e-10 * 1e12 = 100 against 2


def test_an_unbounded_column_wins_over_every_other():
    assert find(mc.UNBOUNDED_WINS) == "unbounded"
    assert F64Tableau(mc.UNBOUNDED_WINS).find(0) == (0, 0)


def test_an_overflowed_ratio_is_no_minimum():
    with np.errstate(over="ignore"):
        assert mc.OVERFLOW[1, 0] / mc.OVERFLOW[1, 1] == np.inf
    assert find(mc.OVERFLOW) == "unbounded"
    assert F64Tableau(mc.OVERFLOW).find(0) == (0, 0)


@pytest.mark.parametrize("tie", [1e-12, 0.0])
def test_an_infinite_maximum_leaves_no_column(tie):
    assert find(mc.NO_COLUMN, dict(ratio_tie=tie)) == (-1, -1)  # LP_PIVOTED with c = -1
    w = mc.walk(mc.NO_COLUMN, mc.CAP, dict(ratio_tie=tie))
    assert (w["status"], w["npiv"], w["log"]) == (_lib.BAD_PIVOT, 0, [])
    assert mc.same_bits(w["T"], mc.NO_COLUMN)


def test_nan_cost_and_nan_cell_are_skipped():
    assert find(mc.NAN_COST) == (1, 1)
    assert find(mc.NAN_CELL) == (0, 1)      # column 0: 6 / 2 = 3 (the NaN row skipped); column 1: 4
    T = mc.NAN_CELL.copy()
    T[1, 1] = 1.0                           # without the NaN column 0 still gives min(4, 3) = 3
    assert find(T) == (0, 1)
    assert np.isnan(mc.walk(mc.NAN_CELL)["T"]).any()


def test_walk_follows_the_statuses():
    for tol in mc.TOLS:
        got = {name: mc.walk(T, mc.CAP, tol) for name, T in mc.CASES.items()}
        assert got["unbounded_wins"]["status"] == got["overflow"]["status"] == _lib.UNBOUNDED
        assert got["no_column"]["status"] == _lib.BAD_PIVOT
        assert got["tie"]["log"] == [[0, 0], [1, 2]] and got["tie"]["status"] == _lib.OPTIMAL
        assert got["band_out"]["log"] == [[1, 2], [0, 0]]
        assert got["band_in"]["log"] == ([[1, 2], [0, 0]] if tol == dict(ratio_tie=0.0) else [[0, 0], [1, 2]])
        assert got["tol_cost"]["log"] == ([[0, 0], [1, 1]] if tol == dict(cost=0.0) else [[1, 1]])
    capped = mc.walk(mc.TIE, 1)
    assert (capped["status"], capped["log"]) == (_lib.PIVOTED, [[0, 0]])
    assert mc.walk(mc.TIE, 0)["status"] == _lib.PIVOTED and mc.walk(mc.TIE, 0)["npiv"] == 0


SMALL_PIVOTS = [7, 3, 3, 7, 5, 4, 5, 7, 5, 7, 7, 3, 6, 5, 8, 7, 4, 3, 6, 5, 5, 6, 6, 7, 5, 5, 4, 3, 4, 8, 6, 4,
                5, 7, 8, 4, 6, 5, 8, 6, 4, 5, 7, 5, 8, 5, 7, 6, 3, 5, 7, 4, 2, 8, 4, 5, 2, 5, 4, 5, 5, 5, 5, 8]
LARGE_PIVOTS = [54, 46, 26, 61, 36, 46, 56, 45]


def test_generator_walks_end_optimal():
    small = [mc.walk(T) for T in mc.small_stack()]
    assert [w["npiv"] for w in small] == SMALL_PIVOTS and all(w["status"] == _lib.OPTIMAL for w in small)
    large = [mc.walk(T) for T in mc.large_stack()]
    assert [w["npiv"] for w in large] == LARGE_PIVOTS and all(w["status"] == _lib.OPTIMAL for w in large)
    for T, npiv in ((gen.klee_minty(8), 1), (gen.klee_minty(8, degenerate=True), 20), (gen.beale(), 2)):
        w = mc.walk(T)
        assert (w["status"], w["npiv"]) == (_lib.OPTIMAL, npiv)


def test_edge_shapes_end_optimal_within_the_cap():
    shapes = {gen.tableau(kind, m, ns, 1).shape for kind, m, ns in mc.EDGES}
    assert {(65, 17), (2, 2), (2, 3), (64, 127), (32, 64), (32, 65), (4, 201), (9, 301), (2, 72), (63, 64)} == shapes
    most = 0
    for kind, m, ns in mc.EDGES:
        for seed in mc.EDGE_SEEDS:
            w = mc.walk(gen.tableau(kind, m, ns, seed))
            assert w["status"] == _lib.OPTIMAL, (kind, m, ns, seed)
            most = max(most, w["npiv"])
    assert most == 104 and most < mc.CAP


def test_the_rule_is_public_and_needs_steps():
    assert _lib.RULE_MAX_INCREASE == lpsol_amd.RULE_MAX_INCREASE == mc.MAXINC == 2
    assert {"RULE_STANDARD", "RULE_MIN_INDEX", "RULE_MAX_INCREASE"} <= set(lpsol_amd.__all__)
    with pytest.raises(ValueError, match="rule and steps go together"):
        solve_batch(mc.small_stack()[:2], rule=_lib.RULE_MAX_INCREASE)
    with pytest.raises(ValueError, match="rule and steps go together"):
        solve_ragged([mc.TIE, mc.OVERFLOW], rule=_lib.RULE_MAX_INCREASE)
