"""lp_reopt_set_costs, lp_reopt_set_general and ProblemResult.reoptimize on the
GPU (csrc/batch.hip: k_cost, k_general_restage).

set_costs is compared bit for bit with the host loop of tests/_reopt_cases.py
applied to the tableau and basis downloaded just before the call; set_general
with general_standard_form's column 0 pushed through the host set_rhs;
reoptimize with those followed by lpf_solve (the primal side) or the host dual
walk (the dual side), and with a cold solve of the same LPs within the
project's objective tolerance of 1e-9 relative (README)."""
import numpy as np
import pytest

import _dual_cases as dc
import _general_cases as gc
import _problem_cases as pc
import _reopt_cases as rc
from lpsol_amd import _lib, solve_problems, solve_problems_ragged
from lpsol_amd import generators as gen
from lpsol_amd import problem as pr

pytestmark = pytest.mark.gpu

REL = 1e-9
snapshot, assert_untouched, same_bits = dc.snapshot, dc.assert_untouched, dc.same_bits


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


assert_set_costs = rc.assert_set_costs


def some_rows(eng, seed0):
    shapes = eng.shapes if hasattr(eng, "shapes") else [(eng.m, eng.n)] * eng.count
    return [rc.some_costs(n, seed0 + i) for i, (_, n) in enumerate(shapes)]


# ---------------------------------------------------------------------------
# set_costs after the plain path and after the two-phase path, whole batch and windows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,ns,B,place", [(8, 10, 64, "lds"), (40, 40, 8, "lds"), (40, 40, 4, "device")],
                         ids=["8x10", "40x40", "40x40-device"])
def test_set_costs_after_the_plain_path(m, ns, B, place):
    T, sense, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=8, place=place)
    assert res.path == "plain" and res.status == ["optimal"] * B
    eng = res._engine
    rows = np.stack(some_rows(eng, 1))
    before, after = assert_set_costs(eng, rows)
    assert any((t[0, 1:] < 0).any() for t in after["T"])
    # the re-priced cost of a basic column is exactly 0.0
    assert all((after["T"][i][0, 1 + before["basis"][i]] == 0.0).all() for i in range(B))
    # windows: the LPs outside them stay bit for bit
    assert_set_costs(eng, np.stack(some_rows(eng, 100))[2:B - 1], first=2)
    assert_set_costs(eng, np.stack(some_rows(eng, 200))[B - 1:], first=B - 1)
    snap = snapshot(eng)
    eng.set_costs(np.empty((0, m + ns + 1)), first=B)          # count 0: a no-op, at the end of the batch too
    eng.set_costs(np.empty((0, m + ns + 1)), first=1)
    assert_untouched(snapshot(eng), snap, range(B))
    # the original costs bring the optimal row back, up to the order of summation
    eng.set_costs(np.concatenate([np.zeros((B, 1)), c, np.zeros((B, m))], axis=1))
    back = eng.download()
    assert np.allclose(back[:, 0], np.stack(before["T"])[:, 0], rtol=0, atol=1e-9)
    # a NaN and an infinity among the costs arrive bit for bit, as the loop has them
    odd = np.stack(some_rows(eng, 300))
    odd[0, 3], odd[1, 0], odd[2, m + ns], odd[3, 1 + int(before["basis"][3][0])] = np.nan, np.inf, -np.inf, np.nan
    _, after = assert_set_costs(eng, odd)
    assert np.isnan(after["T"][0][0, 3]) and np.isnan(after["T"][3][0]).all() and after["T"][1][0, 0] == np.inf
    # a basis entry of -1 is skipped, and so is one of n
    basis = eng.get_basis()
    basis[0, 0], basis[1, m - 1], basis[2, :] = -1, m + ns, -1
    eng.set_basis(basis)
    _, after = assert_set_costs(eng, rows)
    assert same_bits(after["T"][2][0], rows[2])


@pytest.mark.parametrize("kind,B", [("ge", 32), ("neg", 32)])
def test_set_costs_after_the_two_phase_path(kind, B):
    T, sense, ns = pc.stack(kind, 8, 10, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, sense, log_cap=8)
    assert res.path == "twophase" and res.status == ["optimal"] * B and (res.rows == len(sense)).all()
    assert_set_costs(res._engine, np.stack(some_rows(res._engine, 1)))
    assert_set_costs(res._engine, np.stack(some_rows(res._engine, 50))[1:B - 2], first=1)


def test_set_costs_with_equality_rows():
    blocks = [pc.mixed_sense_block(s) for s in range(1, 9)]
    P = np.stack([p for p, _ in blocks])
    res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], blocks[0][1], log_cap=8)
    assert res.path == "twophase" and (res.rows == 5).all() and "optimal" in res.status
    assert (blocks[0][1] == pc.EQ).any()            # == rows are no obstacle here
    assert_set_costs(res._engine, np.stack(some_rows(res._engine, 1)))
    assert_set_costs(res._engine, np.stack(some_rows(res._engine, 9))[3:6], first=3)


@pytest.mark.parametrize("place", ["lds", "device"])
def test_set_costs_on_a_ragged_batch(place):
    tabs = rc.ragged_tableaux()
    items = [(*pc.parts(t, ns), None) for t, (_, ns) in zip(tabs, rc.RAGGED_SHAPES)]
    res = solve_problems_ragged(items, log_cap=8, place=place)
    assert res.status == ["optimal"] * len(items)
    eng, B = res._engine, len(items)
    assert_set_costs(eng, some_rows(eng, 1))
    assert_set_costs(eng, some_rows(eng, 20)[2:B - 1], first=2)
    assert_set_costs(eng, some_rows(eng, 30)[B - 1:], first=B - 1)
    assert_set_costs(eng, some_rows(eng, 40)[3:4], first=3)
    snap = snapshot(eng)
    eng.set_costs([], first=B)
    assert_untouched(snapshot(eng), snap, range(B))


def test_set_costs_refusals_change_nothing():
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2, 3))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=4)
    eng = res._engine
    before = snapshot(eng)
    rows = np.stack(some_rows(eng, 1))
    for first, k in ((-1, 1), (3, 1), (1, 3), (4, 0)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.set_costs(rows[:k], first)
    assert eng.lib.lp_reopt_set_costs(eng.h, 0, 2, None) == _lib.BAD_ARG
    basis = eng.get_basis()
    eng.set_basis(None)
    with pytest.raises(ValueError, match="no basis"):
        eng.set_costs(rows)
    eng.set_basis(basis)
    assert_untouched(snapshot(eng), before, range(3))
    # an LP whose last two-phase call left fewer than m live rows: the wording of set_rhs
    P, s = pc.dependent_block(3)
    P2, _ = pc.dependent_block(4)
    short = solve_problems(np.stack([P[0, 1:], P2[0, 1:]]), np.stack([P[1:, 1:], P2[1:, 1:]]),
                           np.stack([P[1:, 0], P2[1:, 0]]), s, log_cap=4)
    assert (short.rows < len(s)).all()
    before = snapshot(short._engine)
    with pytest.raises(ValueError, match=r"LP 0, row 3: its last two-phase call left 3 of 4 rows live"):
        short._engine.set_costs(np.zeros((2, short._engine.n + 1)))
    with pytest.raises(ValueError, match=r"LP 1, row 3"):
        short._engine.set_costs(np.zeros((1, short._engine.n + 1)), first=1)
    assert_untouched(snapshot(short._engine), before, range(2))


# ---------------------------------------------------------------------------
# the primal side of reoptimize
# ---------------------------------------------------------------------------

def assert_primal(new, before, rows, nss, cap=-1, held=()):
    for i in range(len(new)):
        if i in held:
            assert new.status[i] == "infeasible" and new.npiv[i] == 0, i
            continue
        st, npiv, nstd, log, x, z, _ = rc.host_primal(before["T"][i], before["basis"][i], rows[i], cap)
        assert (new.status_code[i], new.npiv[i], new.nstd[i]) == (st, npiv, nstd), i
        assert new.log(i).tolist() == log[:dc.LOG_CAP], i
        assert same_bits(new.x[i], x[:nss[i]]) and same_bits(new.objective[i], z), i
    assert new.path == "primal" and not new.ninit.any() and not new.stage.any()


@pytest.mark.parametrize("m,ns,B,how", [(8, 10, 64, "tilt"), (8, 10, 64, "swing"), (40, 40, 16, "tilt"),
                                         (40, 40, 16, "swing")])
def test_reoptimize_costs_is_the_host_loop_and_lpf_solve_and_agrees_with_a_cold_solve(m, ns, B, how):
    T, sense, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=dc.LOG_CAP)
    before = snapshot(res._engine)
    old = dict(x=res.x.copy(), objective=res.objective.copy(), status=list(res.status))
    c2 = np.stack([rc.PERTURB[how](c[i], 1 + i) for i in range(B)])
    assert all(same_bits(c2[i], rc.cost_case(m, ns, 1 + i, how)["c"]) for i in range(B))       # the vetted inputs
    new = res.reoptimize(c=c2)
    rows = np.concatenate([np.zeros((B, 1)), c2, np.zeros((B, m))], axis=1)
    assert_primal(new, before, rows, [ns] * B)
    assert new.status == ["optimal"] * B and 2 * np.count_nonzero(new.npiv) >= B
    # the old result keeps what it holds, and y was fetched for it
    assert res._y is not None and same_bits(res.x, old["x"]) and res.status == old["status"]
    for use in (lambda: res.reduced_costs, lambda: res.tableau(0), lambda: res.reoptimize(c=c)):
        with pytest.raises(RuntimeError, match="resolve"):
            use()
    cold = solve_problems(c2, A, b)
    assert cold.status == ["optimal"] * B
    assert all(rel(new.objective[i], cold.objective[i]) <= REL for i in range(B))
    assert new.npiv.sum() < cold.npiv.sum()
    # back to the original costs, on the new result: row 0 and the optimum come back
    mid = snapshot(new._engine)
    again = new.reoptimize(c=c, max_pivots=500)
    assert_primal(again, mid, np.concatenate([np.zeros((B, 1)), c, np.zeros((B, m))], axis=1), [ns] * B, 500)
    assert again.status == ["optimal"] * B
    assert all(rel(again.objective[i], old["objective"][i]) <= REL for i in range(B))


def test_reoptimize_costs_on_a_ragged_result():
    shapes = [rc.SMALL] * 6 + [rc.LARGE] * 3 + [(1, 1), (3, 5)]
    tabs = [gen.tableau("mixed", m, ns, 1 + i) for i, (m, ns) in enumerate(shapes)]
    items = [(*pc.parts(t, ns), None) for t, (_, ns) in zip(tabs, shapes)]
    res = solve_problems_ragged(items, log_cap=dc.LOG_CAP, place="auto")
    before = snapshot(res._engine)
    c2 = [rc.PERTURB[("tilt", "swing")[i % 2]](it[0], 1 + i) for i, it in enumerate(items)]
    new = res.reoptimize(c=c2, c0=-2.0)
    rows = [np.concatenate([[2.0], c2[i], np.zeros(m)]) for i, (m, _) in enumerate(shapes)]
    assert_primal(new, before, rows, [ns for _, ns in shapes])
    assert type(new) is type(res)
    cold = solve_problems_ragged([(c2[i], it[1], it[2], None) for i, it in enumerate(items)], c0=[-2.0] * len(items))
    assert all(rel(new.objective[i], cold.objective[i]) <= REL for i in range(len(items)))


def test_the_hand_lp():
    for c2, status, z, x in rc.HAND_NEW:
        res = solve_problems(rc.HAND_C[None], rc.HAND_A[None], rc.HAND_B[None])
        assert res.status == ["optimal"] and res.objective[0] == 0.0
        new = res.reoptimize(c=c2[None])
        assert new.status == [status]
        if z is not None:
            assert new.objective[0] == z and new.x[0].tolist() == x and new.npiv[0] == 1


def test_an_infeasible_lp_keeps_its_status_and_a_chain_of_both_sides():
    items = dc.infeasible_problems()
    res = solve_problems_ragged(items, log_cap=dc.LOG_CAP)
    assert res.status[dc.INFEASIBLE_AT] == "infeasible" and res.status.count("optimal") == len(items) - 1
    before = snapshot(res._engine)
    c2 = [rc.tilt(it[0], 5 + i) for i, it in enumerate(items)]
    new = res.reoptimize(c=c2)
    shapes = res._engine.shapes
    rows = [np.concatenate([[0.0], c2[i], np.zeros(n - len(c2[i]))]) for i, (_, n) in enumerate(shapes)]
    assert_primal(new, before, rows, [len(v) for v in c2], held=(dc.INFEASIBLE_AT,))
    # its tableau holds its own costs re-priced, not the +0.0 row it was solved under
    i = dc.INFEASIBLE_AT
    assert same_bits(new._engine.download(i, 1)[0], rc.reprice(before["T"][i], before["basis"][i], rows[i]))
    # a chain: new right-hand sides, then new costs, each against the host from the state before it
    T, sense, ns = pc.stack("mixed", 8, 10, range(1, 17))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=dc.LOG_CAP)
    b2 = np.stack([dc.scale(b[k], 1 + k) for k in range(16)])
    c3 = np.stack([rc.swing(c[k], 1 + k) for k in range(16)])
    one = res.reoptimize(b=b2)
    assert one.path == "dual"
    mid = snapshot(one._engine)
    two = one.reoptimize(c=c3)
    assert_primal(two, mid, np.concatenate([np.zeros((16, 1)), c3, np.zeros((16, 8))], axis=1), [ns] * 16,
                  held=[k for k in range(16) if one.status[k] == "infeasible"])
    cold = solve_problems(c3, A, b2)
    for k in range(16):
        assert (two.status[k] == "infeasible") == (cold.status[k] == "infeasible")
        if two.status[k] == cold.status[k] == "optimal":
            assert rel(two.objective[k], cold.objective[k]) <= REL, k


# ---------------------------------------------------------------------------
# set_general and the dual side of reoptimize on general-form results
# ---------------------------------------------------------------------------

border_of, assert_set_general = rc.border_of, rc.assert_set_general


assert_dual = rc.assert_dual


@pytest.mark.parametrize("m,ns,B,way", [(8, 10, 64, "down"), (8, 10, 64, "up"), (24, 24, 16, "down"),
                                         (24, 24, 16, "up")])
def test_branching_on_boxed_lps(m, ns, B, way):
    lps = [(*rc.boxed_lp(m, ns, 1 + i), False) for i in range(B)]
    P = np.stack([lp[0] for lp in lps])
    lb, ub = np.zeros((B, ns)), np.full((B, ns), 2.0)
    res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], lb=lb, ub=ub, log_cap=dc.LOG_CAP)
    assert res.path == "plain" and res.status == ["optimal"] * B and (res.kind == gc.BOXED).all()
    vetted = [rc.branch_case(m, ns, 1 + i, way) for i in range(B)]
    got = [rc.branch_bounds(res.x[i], lb[i], ub[i], way) for i in range(B)]
    assert all(g[0] == v["j"] and same_bits(g[1], v["lb"]) and same_bits(g[2], v["ub"]) for g, v in zip(got, vetted))
    lb2, ub2 = np.stack([g[1] for g in got]), np.stack([g[2] for g in got])
    before = snapshot(res._engine)
    new = res.reoptimize(ub=ub2) if way == "down" else res.reoptimize(lb=lb2)
    cap = 10 * (res._engine.m + res._engine.n)
    assert_dual(new, before, lps, list(zip(lb2, ub2)), cap)
    assert [new.status_code[i] for i in range(B)] == [v["cold"]["status"] for v in vetted]
    for i, v in enumerate(vetted):
        if new.status[i] == "optimal":
            assert rel(new.objective[i], v["cold"]["z"]) <= REL, i
        if v["j"] is None:
            assert new.npiv[i] == 0
    if way == "up":
        assert "infeasible" in new.status
    with pytest.raises(RuntimeError, match="resolve"):
        res.tableau(0)
    if (m, way) == (8, "down"):
        # lb > ub on a BOXED variable: its range row turns negative and the LP ends infeasible
        ub3 = ub2.copy()
        ub3[0, 3] = -1.0
        mid = snapshot(new._engine)
        bad = new.reoptimize(ub=ub3)
        assert_dual(bad, mid, lps, list(zip(lb2, ub3)), cap)
        assert bad.status[0] == "infeasible" and bad.status[1:] == new.status[1:]


def cycled(B, m=8, ns=10):
    return [(*rc.cycled_lp(m, ns, 1 + i), True) for i in range(B)]


def test_set_general_on_kinds_cycling_under_maximise():
    B = 16
    lps = cycled(B)
    P = np.stack([lp[0] for lp in lps])
    lb, ub = np.stack([lp[3] for lp in lps]), np.stack([lp[4] for lp in lps])
    res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], lb=lb, ub=ub, maximize=True, log_cap=dc.LOG_CAP)
    assert res.kind.tolist() == lps[0][2].tolist() and "optimal" in res.status
    assert (res.rows == res._engine.m).all()
    eng = res._engine
    tight = [rc.tighten(lps[i][2], lb[i], ub[i], 1 + i) for i in range(B)]
    borders = [border_of(P[i], *tight[i]) for i in range(B)]
    assert_set_general(eng, lps, borders, tight)
    # windows, a new b and c0 among them; the LPs outside stay bit for bit
    for first, last in ((2, B - 1), (B - 1, B), (5, 6)):
        more = [rc.tighten(lps[i][2], *tight[i], 40 + i) for i in range(first, last)]
        Pw = [P[i].copy() for i in range(first, last)]
        for k, p in enumerate(Pw):
            p[0, 0], p[1:, 0] = 0.5 + k, dc.scale(p[1:, 0], 7 + k)
        assert_set_general(eng, [(Pw[i - first], *lps[i][1:]) if first <= i < last else lps[i] for i in range(B)],
                           [border_of(p, *bd) for p, bd in zip(Pw, more)], more, first=first)
    snap = snapshot(eng)
    eng.set_general(np.empty((0, len(borders[0]))), first=B)
    assert_untouched(snapshot(eng), snap, range(B))


def test_reoptimize_bounds_and_costs_under_maximise():
    B = 16
    lps = cycled(B)
    P = np.stack([lp[0] for lp in lps])
    lb, ub = np.stack([lp[3] for lp in lps]), np.stack([lp[4] for lp in lps])
    c, A, b = P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0]
    res = solve_problems(c, A, b, lb=lb, ub=ub, maximize=True, c0=1.5, log_cap=dc.LOG_CAP)
    lps = [(pr.pack_problems(c[i:i + 1], A[i:i + 1], b[i:i + 1], np.array([-1.5]))[0], *lps[i][1:]) for i in range(B)]
    tight = [rc.tighten(lps[i][2], lb[i], ub[i], 1 + i) for i in range(B)]
    lb2, ub2 = np.stack([t[0] for t in tight]), np.stack([t[1] for t in tight])
    before = snapshot(res._engine)
    new = res.reoptimize(lb=lb2, ub=ub2)
    cap = 10 * (res._engine.m + res._engine.n)
    assert_dual(new, before, lps, tight, cap)
    assert "optimal" in new.status
    cold = solve_problems(c, A, b, lb=lb2, ub=ub2, maximize=True, c0=1.5)
    for i in range(B):
        if res.status[i] == "optimal":          # (an unbounded start is no dual start: the walk says so)
            assert new.status[i] == cold.status[i], i
            if new.status[i] == "optimal":
                assert rel(new.objective[i], cold.objective[i]) <= REL, i
    # new costs on the general-form result: general_cost_row, the host loop, lpf_solve, general_recover
    mid = snapshot(new._engine)
    c2 = np.stack([rc.tilt(c[i], 1 + i) for i in range(B)])
    n = new._engine.n
    rows = pr.general_cost_row(np.concatenate([np.full((B, 1), -1.5), c2], axis=1), lb2, ub2, lps[0][2], True, n)
    last = new.reoptimize(c=c2, max_pivots=500)       # (a cap: an LP that was unbounded is no primal start)
    held = [i for i in range(B) if new.status[i] == "infeasible"]
    for i in range(B):
        if i in held:
            assert last.status[i] == "infeasible" and last.npiv[i] == 0
            continue
        Pn = lps[i][0].copy()                   # set_general stores the new c and rewrites column 0 first
        Pn[0, 1:] = c2[i]
        T1 = rc.host_general_rhs(mid["T"][i], Pn, lps[i][1], lps[i][2], lb2[i], ub2[i], True)
        st, npiv, nstd, log, xs, _, Tf = rc.host_primal(T1, mid["basis"][i], rows[i], 500)
        x, z = pr.general_recover(xs, Tf[0, 0], lb2[i], ub2[i], lps[i][2], True)
        assert (last.status_code[i], last.npiv[i], last.nstd[i]) == (st, npiv, nstd), i
        assert same_bits(last.x[i], x) and same_bits(last.objective[i], z), i
    assert last.path == "primal" and last.maximize is True
    cold = solve_problems(c2, A, b, lb=lb2, ub=ub2, maximize=True, c0=1.5)
    for i in range(B):
        if last.status[i] == cold.status[i] == "optimal":
            assert rel(last.objective[i], cold.objective[i]) <= REL, i
    assert any(last.status[i] == cold.status[i] == "optimal" for i in range(B))


def test_reoptimize_bounds_on_a_ragged_general_result():
    shapes = [(8, 10), (1, 1), (3, 5), (24, 24), (5, 4), (2, 1)]
    lps = []
    for i, (m, ns) in enumerate(shapes):
        P, sense, kind, lb, ub = rc.cycled_lp(m, ns, 60 + i) if i % 2 else rc.boxed_lp(m, ns, 60 + i)
        lps.append((P, sense, kind, lb, ub, bool(i % 2)))
    items = [(p[0, 1:], p[1:, 1:], p[1:, 0], s, lb, ub, mx) for p, s, _, lb, ub, mx in lps]
    res = solve_problems_ragged(items, log_cap=dc.LOG_CAP, place="auto")
    assert all(np.array_equal(k, lp[2]) for k, lp in zip(res.kind, lps))
    tight = [rc.tighten(lp[2], lp[3], lp[4], 9 + i) for i, lp in enumerate(lps)]
    before = snapshot(res._engine)
    new = res.reoptimize(lb=[t[0] for t in tight], ub=[t[1] for t in tight])
    assert_dual(new, before, lps, tight, max(10 * (m + n) for m, n in res._engine.shapes))
    assert type(new) is type(res) and "optimal" in new.status
    # and a window of borders through the engine
    more = [rc.tighten(lps[i][2], *tight[i], 80 + i) for i in range(1, 4)]
    assert_set_general(new._engine, lps, [border_of(lps[i][0], *more[i - 1]) for i in range(1, 4)], more, first=1)


def test_set_general_refusals_change_nothing():
    B = 3
    lps = [(*gc.general_lp(s, kinds=[0, 1, 2, 3, 4]), False) for s in (1, 2, 3)]
    sense = np.array([pc.GE, pc.LE, pc.LE, pc.LE, pc.GE], dtype=np.int8)       # general_lp's, the == row a <= row
    P = np.stack([lp[0] for lp in lps])
    lb, ub = np.stack([lp[3] for lp in lps]), np.stack([lp[4] for lp in lps])
    res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], sense, lb=lb, ub=ub, log_cap=4)
    eng = res._engine
    lps = [(P[i], sense, res.kind, lb[i], ub[i], False) for i in range(B)]
    before, x0 = snapshot(eng), eng.general_solution()[0].copy()
    good =np.stack([border_of(P[i], lb[i], ub[i]) for i in range(B)])
    m, ns = 5, 5
    for first, k in ((-1, 1), (3, 1), (1, 3), (4, 0)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.set_general(good[:k], first)
    assert eng.lib.lp_reopt_set_general(eng.h, 0, 2, None) == _lib.BAD_ARG
    at_lb, at_ub = ns + 1 + m, 2 * ns + 1 + m
    inf = np.inf
    for j, at, value in ((0, at_lb, 1.0), (0, at_ub, 5.0), (1, at_lb, -inf), (1, at_ub, 5.0), (2, at_lb, -inf),
                         (2, at_ub, inf), (3, at_lb, 0.0), (3, at_ub, inf), (4, at_lb, 0.0), (4, at_ub, 5.0),
                         (2, at_lb, np.nan), (3, at_ub, np.nan)):
        bad = good.copy()
        bad[1, at + j] = value
        with pytest.raises(ValueError, match="LP 1, variable %d" % j):
            eng.set_general(bad)
        with pytest.raises(ValueError, match="LP 1, variable %d" % j):
            eng.set_general(bad[1:], first=1)
    assert_untouched(snapshot(eng), before, range(B))
    assert same_bits(eng.general_solution()[0], x0)                 # the stored bounds are the old ones
    # a window without the bad LP is fine: the same border gives column 0 again, up to the order of summation
    assert_set_general(eng, lps, [good[0]], [(lb[0], ub[0])])
    assert np.allclose(eng.download()[0][:, 0], before["T"][0][:, 0], rtol=0, atol=1e-9)
    # reoptimize finds the same on the host, and the result stays live
    bad_ub = ub.copy()
    bad_ub[2, 1] = 3.0
    with pytest.raises(ValueError, match="LP 2, variable 1"):
        res.reoptimize(ub=bad_ub)
    assert not res._stale and res.reduced_costs is not None
    # an equality among the m rows: the message names the LP and the row
    eqs = [gc.general_lp(s, kinds=[0, 1, 2, 3, 0]) for s in (1, 2)]
    Pe = np.stack([e[0] for e in eqs])
    eq = solve_problems(Pe[:, 0, 1:], Pe[:, 1:, 1:], Pe[:, 1:, 0], eqs[0][1], lb=np.stack([e[3] for e in eqs]),
                        ub=np.stack([e[4] for e in eqs]), log_cap=4)
    before = snapshot(eq._engine)
    with pytest.raises(ValueError, match="LP 0, row 1 is an equality"):
        eq._engine.set_general(np.stack([border_of(e[0], e[3], e[4]) for e in eqs]))
    with pytest.raises(ValueError, match='"==" row'):
        eq.reoptimize(ub=np.stack([e[4] for e in eqs]))
    assert_untouched(snapshot(eq._engine), before, range(2))
    # short rows, under a general form
    Pd, s = pc.dependent_block(3)
    short = solve_problems(Pd[None, 0, 1:], Pd[None, 1:, 1:], Pd[None, 1:, 0], s, c0=0.0, log_cap=4)
    assert short.kind is not None and short.rows[0] < len(s)
    before = snapshot(short._engine)
    with pytest.raises(ValueError, match="rows live"):
        short._engine.set_general(border_of(Pd, np.zeros(4), np.full(4, inf))[None])
    assert_untouched(snapshot(short._engine), before, range(1))
    # no form attached
    T, _, ns = pc.stack("mixed", 3, 5, (1, 2))
    plain = solve_problems(*pc.parts(T, ns))
    a = np.zeros(64)
    assert plain._engine.lib.lp_reopt_set_general(plain._engine.h, 0, 1, _lib._ptr(a)) == _lib.BAD_ARG
    assert "no form attached" in plain._engine._err(plain._engine.h)
