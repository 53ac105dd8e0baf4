"""The host statements of the problem form (lpsol_amd.problem:
assemble_tableaux, problem_duals, pack_problems), without a GPU: the formula
gives back the generators' tableaux, and the duals it reads from the float64
oracle's final tableaux have the signs and the objective of LP duality."""
import numpy as np
import pytest

import _problem_cases as pc
from _problem_cases import same_bits
from lpsol_amd import assemble_tableaux, pack_problems, problem_columns, problem_duals
from oracle.f64 import DEFAULT_TOL, OPTIMAL
from oracle.phase1 import solve_lp

CASES = [(kind, m, ns, seed) for kind in pc.KINDS for m, ns in pc.CPU_SHAPES for seed in pc.CPU_SEEDS]


def test_assemble_reproduces_the_generators():
    assert len(CASES) == 96
    for kind, m, ns, seed in CASES:
        T, sense, nvars = pc.lp(kind, m, ns, seed)
        got = assemble_tableaux(pc.block(T, nvars)[None], sense)[0]
        assert problem_columns(sense, nvars) == T.shape[1] - 1
        if kind == "ge":        # the generator's -np.eye leaves -0.0 off the diagonal: by value
            assert np.array_equal(got, T), (kind, m, ns, seed)
            assert not np.signbit(got[:, nvars + 1:][got[:, nvars + 1:] == 0.0]).any()
        else:
            assert same_bits(got, T), (kind, m, ns, seed)
        # the per-LP form and pack_problems agree with the stacked one
        c, A, b = pc.parts(T, nvars)
        assert same_bits(pack_problems(c[None], A[None], b[None])[0], pc.block(T, nvars))
        assert same_bits(assemble_tableaux([pc.block(T, nvars)], [sense])[0], got)


@pytest.fixture(scope="module")
def solved():
    """the oracle's two-phase solve of every case, once"""
    out = []
    for kind, m, ns, seed in CASES:
        T, sense, nvars = pc.lp(kind, m, ns, seed)
        out.append((kind, T, sense, nvars, solve_lp(T, report=True)))
    return out


def test_duals_of_the_oracles_final_tableaux(solved):
    tol = DEFAULT_TOL["cost"]
    worst, checked = 0.0, 0
    for kind, T, sense, ns, o in solved:
        assert o["status"] == OPTIMAL, kind
        y = problem_duals(o["T"], sense, ns)
        le, ge, eq = sense == pc.LE, sense == pc.GE, sense == pc.EQ
        assert (y[le] <= tol).all() and (y[ge] >= -tol).all()
        assert (pc.bits(y[eq]) == pc.QNAN_BITS).all() and not np.isnan(y[~eq]).any()
        if kind == "eq":
            continue
        z = float(o["objective"])
        gap = abs(float(T[1:, 0] @ y) - z) / max(1.0, abs(z))
        worst = max(worst, gap)
        checked += 1
        assert gap <= 1e-12, (kind, T.shape, gap)
    assert checked == 72
    print("worst duality gap %.3g over %d LPs" % (worst, checked))


def test_hand_built_duals_by_value():
    for P, sense, x, z, y in pc.hand_lps():
        T = assemble_tableaux(P[None], sense)[0]
        o = solve_lp(T, report=True)
        assert o["status"] == OPTIMAL and float(o["objective"]) == z
        got = problem_duals(o["T"], sense, P.shape[1] - 1)
        want = np.array(y)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), (got, want)
        assert (pc.bits(got[np.isnan(want)]) == pc.QNAN_BITS).all()
        # x of the structural variables, from the oracle's basis
        xs = np.zeros(T.shape[1] - 1)
        for r, c in enumerate(o["bfs"][:o["rows"]]):
            if c >= 0:
                xs[c] = o["T"][1 + r, 0]
        assert xs[:P.shape[1] - 1].tolist() == x


def test_duals_flip_the_sign_bit_on_le_rows():
    T = np.zeros((3, 5))
    T[0, 3:] = [0.0, 2.5]
    y = problem_duals(T, [pc.LE, pc.LE], 2)
    assert np.signbit(y[0]) and y[0] == 0.0 and y[1] == -2.5
    y = problem_duals(T, [pc.GE, pc.GE], 2)
    assert not np.signbit(y[0]) and y[1] == 2.5
    with pytest.raises(ValueError, match="columns"):
        problem_duals(T, [pc.LE, pc.EQ], 2)


def test_special_cells_are_copied_by_their_bits():
    P, sense = pc.special_block()
    T = assemble_tableaux(P[None], sense)[0]
    assert T.shape == (3, 6)
    assert same_bits(T[:, :4], P)
    assert same_bits(T[:, 4:], np.array([[0.0, 0.0], [-1.0, 0.0], [0.0, 1.0]]))
