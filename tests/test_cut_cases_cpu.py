"""The inputs of the warm-cut tests on the host oracle alone (tests/_cut_cases.py):
the LPs the GPU tests extend, walked with the host dual rule and compared
with a cold solve of the LPs with the rows added.

Measured here on the oracle (le and lege, 8x10 seeds 1..64, 24x24 seeds 1..32,
40x40 seeds 1..16): every warm verdict equals the cold one; the optima agree
within 3.9e-15 relative (the bound asserted is 1e-12); the longest warm walk
takes 41 pivots against a cap of 10 * (m' + n') >= 300; set_rhs on D with the
joined slack table and right-hand sides gives D's column 0 back within 1.3e-15
of the largest entry of the column (the bound asserted is 1e-12)."""
import numpy as np
import pytest

import _cut_cases as cc
import _dual_cases as dc
from lpsol_amd import _lib
from lpsol_amd.problem import extend_tableau

REL = 1e-12
SHAPES = [cc.SMALL, cc.MID, cc.LARGE]


def cases(shape, workload):
    return [cc.case(*shape, seed, workload) for seed in cc.SEEDS[shape]]


@pytest.mark.parametrize("workload", cc.WORKLOADS)
@pytest.mark.parametrize("shape", SHAPES, ids=["8x10", "24x24", "40x40"])
def test_warm_verdicts_and_optima_equal_the_cold_ones(shape, workload):
    worst, most, verdicts = 0.0, 0, []
    for c in cases(shape, workload):
        st, npiv, _, z = cc.warm_answer(c)
        cst, cz, _ = cc.cold(c, workload)
        assert st == cst, (shape, workload, st, cst)
        assert st in (_lib.OPTIMAL, _lib.INFEASIBLE)
        assert npiv < c["cap"]
        most = max(most, npiv)
        verdicts.append(st)
        if st == _lib.OPTIMAL:
            worst = max(worst, abs(z - cz) / max(1.0, abs(cz)))
    print("%s %s: worst relative difference %.3g, most warm pivots %d, %d optimal, %d infeasible"
          % (shape, workload, worst, most, verdicts.count(_lib.OPTIMAL), verdicts.count(_lib.INFEASIBLE)))
    assert worst <= REL
    if workload == "le":
        assert verdicts == [_lib.OPTIMAL] * len(verdicts)
    else:
        assert _lib.OPTIMAL in verdicts and _lib.INFEASIBLE in verdicts


def test_warm_takes_fewer_pivots_than_cold_on_average():
    for shape in SHAPES:
        cs = cases(shape, "le")
        warm = np.mean([c["warm"]["npiv"] for c in cs])
        cold = np.mean([cc.cold(c, "le")[2] for c in cs])
        print("%s le: mean pivots warm %.1f, cold %.1f" % (shape, warm, cold))
        assert warm < cold


def test_the_inputs_are_no_no_ops():
    """a condition on the inputs: the cuts cut the optimum off, so the GPU tests are not about walks of no pivot"""
    idle = [c["warm"]["npiv"] == 0 for c in cases(cc.SMALL, "lege")]
    assert sum(idle) <= 2
    assert all(c["warm"]["npiv"] > 0 for c in cases(cc.SMALL, "le"))


@pytest.mark.parametrize("workload", cc.WORKLOADS)
def test_the_new_columns_hold_the_basis_inverse(workload):
    """the M-reading of DESIGN.md 4q holds on D: set_rhs with the joined slack table and right-hand sides
    reproduces D's column 0 up to the order of summation"""
    worst = 0.0
    for shape in SHAPES:
        m, ns = shape
        for c in cases(shape, workload):
            slack = dc.slack_table(c["joined"], ns)
            rhs = np.concatenate([[c["T0"][0, 0]], c["T0"][1:, 0], c["beta"]])
            back = dc.set_rhs(c["D"], slack, rhs)
            scale = max(1.0, np.abs(c["D"][:, 0]).max())
            worst = max(worst, np.abs(back[:, 0] - c["D"][:, 0]).max() / scale)
            assert dc.same_bits(back[:, 1:], c["D"][:, 1:])
    print("%s: column 0 comes back within %.3g" % (workload, worst))
    assert worst <= REL


def test_extend_is_the_package_statement():
    """lpsol_amd.problem.extend_tableau (columns side by side) gives the scalar loop's bits"""
    for shape, seed, workload, q in ((cc.SMALL, 3, "lege", 2), (cc.MID, 4, "le", 3), ((1, 1), 5, "lege", 1),
                                     (cc.SMALL, 6, "le", 0), (cc.SMALL, 7, "lege", 5)):
        c = cc.case(*shape, seed, workload, q)
        D, basis = extend_tableau(c["opt"], c["basis"], c["rows"], c["sense"])
        assert dc.same_bits(D, c["D"]) and np.array_equal(basis, c["basis2"]) and basis.dtype == np.int32
    T, basis, rows, sense = cc.odd_case()
    D, _ = extend_tableau(T, basis, rows, sense)
    want, _ = cc.extend(T, basis, rows, sense)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(D), nan) and dc.same_bits(D[~nan], want[~nan])
    assert dc.same_bits(D[:4, :5], T)                           # the NaN and the -0.0 of T are copied as bits
    assert np.signbit(D[5, 0]) and D[5, 0] == 0.0              # a >= cut whose priced cell is +0.0 stores -0.0
    assert nan[4:, :5].any() and np.isinf(D[4, :5]).any()
    with pytest.raises(ValueError, match='"=="'):
        extend_tableau(T, basis, rows[:1], ["=="])
    with pytest.raises(ValueError, match="rows must be"):
        extend_tableau(T, basis, rows[:, :4], sense)
    with pytest.raises(ValueError, match="sense must hold"):
        extend_tableau(T, basis, rows, sense[:2])
