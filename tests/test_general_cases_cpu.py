"""General-form LPs on the host: the conversion to the standard form, the
recovery and the KKT conventions (lpsol_amd.problem.general_*), checked on the
f64 oracle alone.  No GPU.

Measured here on the 40 seeds of _general_cases.general_lp: 26 optimal under
min and 23 under max, the rest unbounded; 15 optima with a BOXED variable at
its ub, 14 with a FREE variable negative.  Worst values, each relative to
max(1, the magnitudes compared): |c - A^T y - r| 1.3e-15 (the share of the
equality row, which has no dual, projected out), |z - (c0 + c.x)| 5.6e-16, a
bound passed by 2.2e-16, a row by 7.8e-16."""
import numpy as np
import pytest

import _general_cases as gc
import _problem_cases as pc
from lpsol_amd import _lib, solve_problems, solve_problems_ragged
from lpsol_amd import problem as pr

TOL = 1e-9          # the project's relative tolerance
OPTIMAL = [k for k, v in _lib.STATUS_NAMES.items() if v == "optimal"][0]


@pytest.fixture(scope="module")
def solved():
    """(seed, maximise) -> the LP and the oracle's answer, computed once"""
    out = {}
    for mx in (False, True):
        for seed in gc.SEEDS:
            lp = gc.general_lp(seed)
            out[seed, mx] = (lp, gc.oracle_solve(*lp, mx))
    return out


def test_the_cases_cover_what_they_should(solved):
    at_ub = free_neg = 0
    for mx in (False, True):
        opt = [(lp, o) for (seed, d), (lp, o) in solved.items() if d == mx and o["status"] == OPTIMAL]
        assert 2 * len(opt) >= len(gc.SEEDS), (mx, len(opt))
        for (P, s, kind, lb, ub), o in opt:
            at_ub += any(kind[j] == gc.BOXED and o["x"][j] == ub[j] for j in range(gc.NS))
            free_neg += any(kind[j] == gc.FREE and o["x"][j] < 0.0 for j in range(gc.NS))
    assert at_ub >= 1 and free_neg >= 1


def test_kkt_objective_bounds_and_rows_at_the_optima(solved):
    worst = dict(kkt=0.0, z=0.0, bound=0.0, row=0.0)
    for (seed, mx), ((P, s, kind, lb, ub), o) in solved.items():
        if o["status"] != OPTIMAL:
            continue
        c, A, b = P[0, 1:], P[1:, 1:], P[1:, 0]
        x, y, r = o["x"], o["y"], o["r"]
        has = ~np.isnan(y)
        assert (has == (s != pc.EQ)).all()
        # c - A^T y = r over the rows with a dual; an equality row has none, and r holds its share, a
        # multiple of that row: it is projected out of the residual
        resid = c - A[has].T @ y[has] - r
        if (~has).any():
            E = A[~has]
            resid = resid - E.T @ np.linalg.lstsq(E.T, resid, rcond=None)[0]
        scale = max(1.0, np.abs(c).max(), np.abs(r).max())
        worst["kkt"] = max(worst["kkt"], np.abs(resid).max() / scale)
        z = -P[0, 0] + c @ x
        worst["z"] = max(worst["z"], abs(o["z"] - z) / max(1.0, abs(z)))
        worst["bound"] = max(worst["bound"], (lb - x).max(), (x - ub).max(), 0.0)
        ax = A @ x
        viol = np.where(s == pc.LE, ax - b, np.where(s == pc.GE, b - ax, np.abs(ax - b)))
        worst["row"] = max(worst["row"], viol.max() / max(1.0, np.abs(b).max()))
        # the sign conventions: at a lower bound r >= 0 under min, <= 0 under max; reversed at an upper one
        sgn = -1.0 if mx else 1.0
        for j in range(gc.NS):
            if kind[j] == gc.FREE:
                assert abs(r[j]) <= TOL
            elif x[j] > lb[j] + TOL and x[j] < ub[j] - TOL:
                assert abs(r[j]) <= TOL, (seed, mx, j)
            elif x[j] <= lb[j] + TOL:
                assert sgn * r[j] >= -TOL, (seed, mx, j)
            else:
                assert sgn * r[j] <= TOL, (seed, mx, j)
    print("worst:", worst)
    assert all(v <= TOL for v in worst.values()), worst


def test_hand_lps_are_exact_on_the_oracle():
    for h in gc.hand_lps():
        P, s, kind, lb, ub = gc.hand_block(h)
        o = gc.oracle_solve(P, s, kind, lb, ub, h["maximize"])
        assert _lib.STATUS_NAMES[o["status"]] == h["status"]
        if h["status"] != "optimal":
            continue
        entries, T = gc.pivot_entries(o["T0"], o["rep"])
        assert np.array_equal(T, o["rep"]["T"])             # the replay is the oracle's run
        assert entries and all(abs(e) == 1.0 for e in entries)
        assert o["x"].tolist() == h["x"] and o["z"] == h["z"]
        assert o["y"].tolist() == h["y"] and (o["r"] == np.array(h["r"])).all()


def test_hand_lps_cover_the_kinds():
    kinds = [gc.hand_block(h)[2].tolist() for h in gc.hand_lps()]
    assert [gc.BOXED, gc.BOXED] in kinds and [gc.FREE, gc.LOWER] in kinds and [gc.UPPER, gc.PLAIN] in kinds
    h = gc.hand_lps()[3]
    assert h["lb"][0] > h["ub"][0] and h["status"] == "infeasible"


def test_default_form_is_the_problem_form_bit_for_bit():
    blocks = [pc.mixed_sense_block(seed, 5) for seed in range(1, 9)] + [pc.special_block()]
    for P, s in blocks:
        ns = P.shape[1] - 1
        kinds = np.zeros(ns, dtype=np.int8)
        want = pr.assemble_tableaux(P[None], s)[0]
        got = pr.general_standard_form(P, None, None, s, kinds, False)
        assert pc.same_bits(got, want)
        assert pr.general_shape(s, kinds) == (want.shape[0] - 1, want.shape[1] - 1)
        # under maximise only the sign bits of row 0 differ: every cell of it, the slack zeros excepted
        mx = pr.general_standard_form(P, None, None, s, kinds, True)
        diff = pc.bits(mx) ^ pc.bits(want)
        assert not diff[1:].any()
        assert (diff[0, :ns + 1] == 1 << 63).all() and not diff[0, ns + 1:].any()
    # a stack goes through the same loop
    P3 = np.stack([pc.mixed_sense_block(seed, 5)[0] for seed in range(1, 5)])
    s = pc.mixed_sense_block(1, 5)[1]
    assert pc.same_bits(pr.general_standard_form(P3, None, None, s, np.zeros(5, dtype=np.int8)),
                        pr.assemble_tableaux(P3, s))


def test_standard_form_layout_of_all_five_kinds():
    P, s, kind, lb, ub = gc.general_lp(5)           # kinds 0, 1, 2, 3, 4
    assert kind.tolist() == [0, 1, 2, 3, 4]
    T = pr.general_standard_form(P, lb, ub, s, kind, True)
    m, ns = 5, 5
    assert T.shape == (m + 1 + 1, 1 + ns + 1 + 4 + 1) and pr.general_shape(s, kind) == (6, 11)
    c, A, b = P[0, 1:], P[1:, 1:], P[1:, 0]
    assert (T[0, 1:6] == [-c[0], -c[1], -c[2], c[3], -c[4]]).all() and T[0, 6] == c[4]
    assert (T[1:6, 4] == -A[:, 3]).all() and (T[1:6, 6] == -A[:, 4]).all() and (T[1:6, 5] == A[:, 4]).all()
    rhs = b.copy()
    for j, sj in ((1, lb[1]), (2, lb[2]), (3, ub[3])):
        rhs = rhs - A[:, j] * sj
    assert (T[1:6, 0] == rhs).all()
    assert T[6, 0] == ub[2] - lb[2] and T[6, 3] == 1.0 and T[6, 11] == 1.0 and np.count_nonzero(T[6]) == 3
    # the oracle's answer survives the round trip: general_recover undoes the substitution
    o = gc.oracle_solve(P, s, kind, lb, ub, True)
    xs = o["xstd"]
    assert o["x"][0] == xs[0] and o["x"][1] == lb[1] + xs[1] and o["x"][3] == ub[3] - xs[3]
    assert o["x"][4] == xs[4] - xs[5]


def test_kinds_from_bounds():
    inf = gc.INF
    assert pr.general_kinds([0, 1, -1, -inf, -inf, -0.0], [inf, inf, 2, 3, inf, inf]).tolist() == [0, 1, 2, 3, 4, 0]
    # PLAIN needs lb == 0 in every LP of the stack
    assert pr.general_kinds([[0, 0], [0, 1]], None).tolist() == [gc.PLAIN, gc.LOWER]
    assert pr.general_kinds(None, [[1, inf], [2, inf]]).tolist() == [gc.BOXED, gc.PLAIN]
    with pytest.raises(ValueError, match="solve_problems_ragged"):
        pr.general_kinds([[0, 0], [0, -inf]], None)
    with pytest.raises(ValueError, match="solve_problems_ragged"):
        pr.general_kinds(None, [[1, inf], [inf, inf]])
    for lb, ub, what in (([np.nan], [1], "NaN"), ([0], [np.nan], "NaN"), ([inf], [inf], r"\+inf"),
                         ([0], [-inf], "-inf")):
        with pytest.raises(ValueError, match=what):
            pr.general_kinds(lb, ub)


def test_argument_errors_come_before_any_device_call():
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2))
    c, A, b = pc.parts(T, ns)
    far = dict(device=1 << 20)
    with pytest.raises(ValueError, match="NaN"):
        solve_problems(c, A, b, lb=[0, 0, np.nan, 0, 0], **far)
    with pytest.raises(ValueError, match=r"\+inf"):
        solve_problems(c, A, b, lb=[0, 0, np.inf, 0, 0], **far)
    with pytest.raises(ValueError, match="-inf"):
        solve_problems(c, A, b, ub=[1, 1, -np.inf, 1, 1], maximize=True, **far)
    with pytest.raises(ValueError, match="solve_problems_ragged"):
        solve_problems(c, A, b, ub=[[1] * 5, [1, 1, np.inf, 1, 1]], **far)
    with pytest.raises(ValueError):
        solve_problems(c, A, b, lb=[0, 0, 0], **far)           # not ns entries
    one = (c[0], A[0], b[0], None)
    with pytest.raises(ValueError, match="LP 1: a bound is NaN"):
        solve_problems_ragged([one, (c[1], A[1], b[1], None, [np.nan] * 5, None, False)], **far)
    with pytest.raises(ValueError, match="LP 0 must be"):
        solve_problems_ragged([(c[0], A[0], b[0], None, None)], maximize=True, **far)
    with pytest.raises(ValueError, match="lb must hold one entry per LP"):
        solve_problems_ragged([one, one], lb=[[0] * 5], **far)


def test_general_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2))
    c, A, b = pc.parts(T, ns)
    with pytest.raises(_lib.EngineUnavailable):
        solve_problems(c, A, b, maximize=True)
    with pytest.raises(_lib.EngineUnavailable):
        solve_problems_ragged([(c[0], A[0], b[0], None, None, [1.0] * 5, False)])
