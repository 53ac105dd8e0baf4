"""lp_reopt_set_costs and lp_reopt_set_general on the GPU, where the first tests
do not look (csrc/batch.hip: k_cost, k_general_restage, k_general_shift and the
k_rhs that follows): windows of more than one workgroup, ragged and
uniform, beginning above LP 0; a device-placed general-form batch re-optimised on
the dual side; costs and borders near overflow and in the subnormal range.

set_costs is compared bit for bit (a NaN matching a NaN) with the host loop of
tests/_reopt_cases.py applied to the tableau and basis downloaded just before the
call, set_general with general_standard_form's column 0 pushed through the host
set_rhs, run(RULE_DUAL) with those followed by the host walk and general_recover.
The inputs, and where their lanes fall, are vetted by tests/test_reopt_cases_cpu.py."""
import numpy as np
import pytest

import _dual_cases as dc
import _general_cases as gc
import _problem_cases as pc
import _reopt_cases as rc
from lpsol_amd import _lib, solve_problems, solve_problems_ragged

pytestmark = pytest.mark.gpu

REL = 1e-9          # the project's tolerance on an optimum (README): warm against cold only
same_bits = dc.same_bits


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


# ---------------------------------------------------------------------------
# 1, 2. k_cost on windows of more than one workgroup
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("place", ["auto", "device"])
def test_k_cost_on_ragged_windows_across_workgroups(place):
    tabs = rc.cost_block_tableaux()
    items = [(*pc.parts(t, ns), None) for t, (_, ns) in zip(tabs, rc.COST_SHAPES)]
    res = solve_problems_ragged(items, place=place)
    assert res.path == "plain" and res.status == ["optimal"] * len(items)
    eng = res._engine
    assert eng.placement(rc.COST_BIG) == ("lds" if place == "auto" else "device")
    for k, (first, count) in enumerate(rc.COST_WINDOWS):
        rows = [rc.some_costs(n, 100 * k + i) for i, (_, n) in enumerate(eng.shapes)]
        before, after = rc.assert_set_costs(eng, rows[first:first + count], first=first)
        assert any(not same_bits(after["T"][i][0], before["T"][i][0]) for i in range(first, first + count))


@pytest.mark.parametrize("place", ["lds", "device"])
def test_k_cost_on_uniform_windows_across_workgroups_with_first_above_zero(place):
    u = rc.COST_UNIFORM
    T, _, ns = pc.stack("mixed", u["m"], u["ns"], range(1, u["B"] + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, place=place)
    assert res.path == "plain" and res.status == ["optimal"] * u["B"]
    eng = res._engine
    for k, (first, count) in enumerate(u["windows"]):
        rows = np.stack([rc.some_costs(eng.n, 100 * k + i) for i in range(u["B"])])
        before, after = rc.assert_set_costs(eng, rows[first:first + count], first=first)
        assert all(not same_bits(after["T"][i][0], before["T"][i][0]) for i in range(first, first + count))


# ---------------------------------------------------------------------------
# 3. set_general on windows of more than one workgroup, then the dual walk
# ---------------------------------------------------------------------------

def test_set_general_on_ragged_windows_across_workgroups_then_the_dual_walk():
    lps = rc.general_block_lps()
    items = [(p[0, 1:], p[1:, 1:], p[1:, 0], s, lb, ub, mx) for p, s, _, lb, ub, mx in lps]
    res = solve_problems_ragged(items, log_cap=dc.LOG_CAP, place="auto")
    assert all(np.array_equal(k, lp[2]) for k, lp in zip(res.kind, lps))
    assert res.status == ["optimal"] * len(lps)
    eng = res._engine
    assert [int(r) for r in res.rows] == [m for m, _ in eng.shapes]                # every row live
    assert eng.placement(rc.GENERAL_BIG) == "device" and eng.placement(0) == "lds"
    borders = lambda tight, w: [rc.border_of(lps[i][0], *tight[i]) for i in w]
    for k, (first, count) in enumerate(rc.GENERAL_WINDOWS):
        tight, w = rc.general_tight(lps, k), range(first, first + count)
        before, after = rc.assert_set_general(eng, lps, borders(tight, w), [tight[i] for i in w], first=first)
        assert any(not same_bits(after["T"][i][:, 0], before["T"][i][:, 0]) for i in w)
    # the window that spans the boundaries once more, under bounds that cut each LP's optimum off, then the
    # walk of its LPs against the host chain
    first, count = rc.GENERAL_WALKED
    tight, w = rc.general_squeezed(lps), range(first, first + count)
    before, _ = rc.assert_set_general(eng, lps, borders(tight, w), [tight[i] for i in w], first=first)
    # but for column 0 the stored tableaux are the oracle's optima, so what the host test found of these walks holds
    for i, (T, basis) in enumerate(rc.general_block_optima()):
        assert same_bits(before["T"][i][:, 1:], T[:, 1:]) and np.array_equal(before["basis"][i], basis), i
    cap = max(10 * (m + n) for m, n in eng.shapes)
    status, done = eng.run(_lib.RULE_DUAL, cap)
    xg, zg = eng.general_solution()
    verdicts = set()
    for i in w:
        P, sense, kind, _, _, mx = lps[i]
        h = rc.host_general_dual(before["T"][i], before["basis"][i], P, sense, kind, *tight[i], mx, cap)
        assert (int(status[i]), int(done[i])) == (h["status"], h["npiv"]), i
        assert eng.log(i).tolist() == h["log"][:dc.LOG_CAP], i
        assert same_bits(np.asarray(xg[i]), h["x"]) and same_bits(zg[i], np.float64(h["z"])), i
        verdicts.add(h["status"])
    assert verdicts == {_lib.OPTIMAL, _lib.INFEASIBLE}
    assert int(done[first:first + count].sum()) > 0 and int(done[rc.GENERAL_BIG]) > 0


# ---------------------------------------------------------------------------
# 4. a device-placed general-form batch on the dual side
# ---------------------------------------------------------------------------

def test_a_device_placed_general_batch_reoptimises_as_the_host_walk_and_as_the_lds_placed_one():
    m, ns, B, way = 24, 24, 16, "down"
    lps = [(*rc.boxed_lp(m, ns, 1 + i), False) for i in range(B)]
    P = np.stack([lp[0] for lp in lps])
    lb, ub = np.zeros((B, ns)), np.full((B, ns), 2.0)
    got = {}
    for place in ("device", "lds"):
        res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], lb=lb, ub=ub, log_cap=dc.LOG_CAP, place=place)
        assert res.path == "plain" and res.status == ["optimal"] * B and (res.kind == gc.BOXED).all()
        assert all(res._engine.placement(i) == place for i in (0, B - 1))
        vetted = [rc.branch_case(m, ns, 1 + i, way) for i in range(B)]
        new_bounds = [rc.branch_bounds(res.x[i], lb[i], ub[i], way) for i in range(B)]
        assert all(g[0] == v["j"] and same_bits(g[2], v["ub"]) for g, v in zip(new_bounds, vetted))
        ub2 = np.stack([g[2] for g in new_bounds])
        before = dc.snapshot(res._engine)
        new = res.reoptimize(ub=ub2)
        cap = 10 * (res._engine.m + res._engine.n)
        rc.assert_dual(new, before, lps, list(zip(lb, ub2)), cap)
        assert [new.status_code[i] for i in range(B)] == [v["cold"]["status"] for v in vetted]
        assert all(rel(new.objective[i], v["cold"]["z"]) <= REL for i, v in enumerate(vetted) if new.status[i] == "optimal")
        assert new.npiv.sum() > 0
        got[place] = dict(before=before, T=new._engine.download(), basis=new._engine.get_basis(), x=np.array(new.x),
                          z=np.array(new.objective), npiv=np.array(new.npiv), status=list(new.status))
    dev, lds = got["device"], got["lds"]
    assert all(same_bits(a, b) for a, b in zip(dev["before"]["T"], lds["before"]["T"]))
    assert same_bits(dev["T"], lds["T"]) and np.array_equal(dev["basis"], lds["basis"])
    assert same_bits(dev["x"], lds["x"]) and same_bits(dev["z"], lds["z"])
    assert np.array_equal(dev["npiv"], lds["npiv"]) and dev["status"] == lds["status"]


# ---------------------------------------------------------------------------
# 5. costs and borders near overflow and in the subnormal range
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("place", ["lds", "device"])
def test_extreme_costs_are_the_host_loop_bit_for_bit(place):
    m, ns = rc.SMALL
    B = 2 * len(rc.EXTREME_COSTS)
    T, _, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, place=place)
    assert res.status == ["optimal"] * B
    eng = res._engine
    # the stored optimum is the oracle's, so the host test's findings about the expected rows hold here
    assert all(same_bits(t, rc.cost_case(m, ns, 1 + i, "tilt")["opt"]) for i, t in enumerate(eng.download()))
    rows = np.stack([rc.extreme_costs(m + ns, i, 1 + i) for i in range(B)])
    assert np.isfinite(rows).all()
    _, after = rc.assert_set_costs(eng, rows)
    row0 = np.stack([t[0] for t in after["T"]])
    assert np.isinf(row0).any() and np.isnan(row0).any() and rc.is_subnormal(row0).any()
    # a window of them on top of that state: the LPs outside keep their infinities and NaNs bit for bit
    rc.assert_set_costs(eng, rows[::-1][2:B - 3], first=2)


@pytest.mark.parametrize("place", ["lds", "device"])
def test_extreme_borders_are_the_host_statement_bit_for_bit(place):
    m, ns, B = *rc.SMALL, 8
    lps = [(*rc.boxed_lp(m, ns, 1 + i), False) for i in range(B)]
    P = np.stack([lp[0] for lp in lps])
    res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], lb=np.zeros((B, ns)), ub=np.full((B, ns), 2.0),
                         place=place)
    assert res.status == ["optimal"] * B
    eng = res._engine
    assert all(same_bits(t, rc.branch_case(m, ns, 1 + i, "down")["opt"]) for i, t in enumerate(eng.download()))
    new = [rc.extreme_bounds(lps[i][0], lps[i][3], lps[i][4], i) for i in range(B)]
    stated = [(p, *lps[i][1:]) for i, (p, _, _) in enumerate(new)]
    with np.errstate(all="ignore"):
        _, after = rc.assert_set_general(eng, stated, [rc.border_of(p, lo, hi) for p, lo, hi in new],
                                         [(lo, hi) for _, lo, hi in new])
        col0 = np.concatenate([t[:, 0] for t in after["T"]])
        assert np.isinf(col0).any() and np.isnan(col0).any() and rc.is_subnormal(col0).any()
        rc.assert_set_general(eng, stated, [rc.border_of(p, lo, hi) for p, lo, hi in new][3:6],
                              [(lo, hi) for _, lo, hi in new][3:6], first=3)
