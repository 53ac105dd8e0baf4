"""The inputs of the warm re-optimisation tests on the oracle alone: what a GPU
test compares the device with must itself be right, and must not be trivial --
a batch in which no LP pivots would let a kernel that does nothing pass."""
import numpy as np
import pytest

import _general_cases as gc
import _reopt_cases as rc
from lpsol_amd import _lib
from lpsol_amd import problem as pr
from oracle.f64 import F64Tableau

COST_BATCHES = [(how, shape) for how in ("tilt", "swing") for shape in (rc.SMALL, rc.MID, rc.LARGE)]
BRANCH_BATCHES = [(way, shape) for way in ("down", "up") for shape in (rc.SMALL, rc.MID)]
REL = 1e-9          # the project's tolerance on an optimum


def close(a, b):
    return abs(a - b) <= REL * max(1.0, abs(b))


@pytest.mark.parametrize("how,shape", COST_BATCHES, ids=lambda v: str(v))
def test_new_costs_warm_equals_cold(how, shape):
    cases = [rc.cost_case(*shape, s, how) for s in rc.SEEDS[shape]]
    for s, c in zip(rc.SEEDS[shape], cases):
        assert c["warm"]["status"] == c["cold"]["status"] == _lib.OPTIMAL, s
        assert close(c["warm"]["objective"], c["cold"]["objective"]), s
        # lpf_pivot leaves exact unit columns: the re-priced cost of a basic column is exactly 0.0
        assert (c["T"][0, 1 + c["basis"]] == 0.0).all(), s
        # rows 1..m are the optimal tableau's
        assert rc.same_bits(c["T"][1:], c["opt"][1:]), s
    moved = sum(len(c["warm"]["log"]) > 0 for c in cases)
    assert 2 * moved >= len(cases), (moved, len(cases))


def test_the_library_loop_is_the_test_modules_loop():
    for shape, seed, how in ((rc.SMALL, 3, "tilt"), (rc.MID, 5, "swing"), ((1, 1), 2, "tilt")):
        c = rc.cost_case(*shape, seed, how)
        assert rc.same_bits(pr.reprice_costs(c["opt"], c["basis"], c["row"]), c["T"])
    # an entry outside [0, n) is skipped; a NaN and an infinity go through as the loop has them
    T = np.array([[0.0, 1.0, 2.0, 3.0], [4.0, 1.0, 5.0, 6.0], [7.0, 0.0, 8.0, 9.0]])
    for basis in ([0, -1], [3, 0], [-1, -1]):
        for row in ([1.0, 2.0, np.nan, 4.0], [np.inf, -2.0, 0.5, -0.0]):
            assert rc.same_bits(pr.reprice_costs(T, basis, row), rc.reprice(T, basis, row))
    assert rc.same_bits(pr.reprice_costs(T, [-1, -1], [1.0, 2.0, 3.0, 4.0])[0], np.array([1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(ValueError, match="costs must hold"):
        pr.reprice_costs(T, [0, 1], [1.0, 2.0])
    with pytest.raises(ValueError, match="basis must hold"):
        pr.reprice_costs(T, [0], [1.0, 2.0, 3.0, 4.0])


@pytest.mark.parametrize("way,shape", BRANCH_BATCHES, ids=lambda v: str(v))
def test_branch_warm_equals_cold(way, shape):
    cases = [rc.branch_case(*shape, s, way) for s in rc.SEEDS[shape]]
    for s, c in zip(rc.SEEDS[shape], cases):
        assert c["warm"]["status"] == c["cold"]["status"], s
        assert c["warm"]["status"] in (_lib.OPTIMAL, _lib.INFEASIBLE), s
        if c["warm"]["status"] == _lib.OPTIMAL:
            assert close(c["warm"]["z"], c["cold"]["z"]), s
        if c["j"] is None:
            assert c["warm"]["npiv"] == 0 and c["warm"]["status"] == _lib.OPTIMAL, s
        elif way == "down":
            assert c["warm"]["npiv"] > 0, s          # the old optimum violates the new bound
    statuses = [c["warm"]["status"] for c in cases]
    if way == "up":
        assert statuses.count(_lib.INFEASIBLE) >= 1
        assert 4 * statuses.count(_lib.OPTIMAL) >= 3 * len(cases)
    else:
        assert statuses.count(_lib.OPTIMAL) == len(cases)
    assert sum(c["j"] is None for c in cases) <= 1


def test_general_cost_row_is_row_0_of_the_standard_form():
    for seed in gc.SEEDS:
        P, sense, kind, lb, ub = gc.general_lp(seed)
        for mx in (False, True):
            T = pr.general_standard_form(P, lb, ub, sense, kind, mx)
            row = pr.general_cost_row(P[0], lb, ub, kind, mx, T.shape[1] - 1)
            assert rc.same_bits(row, T[0]), (seed, mx)
            nf = int((kind == gc.FREE).sum())
            assert rc.same_bits(pr.general_cost_row(P[0], lb, ub, kind, mx), T[0, :1 + len(kind) + nf])
    for h in gc.hand_lps():
        P, sense, kind, lb, ub = gc.hand_block(h)
        T = pr.general_standard_form(P, lb, ub, sense, kind, h["maximize"])
        assert rc.same_bits(pr.general_cost_row(P[0], lb, ub, kind, h["maximize"], T.shape[1] - 1), T[0])
    # a stack at once
    Ps = [gc.general_lp(s, kinds=[0, 1, 2, 3, 4]) for s in (1, 2, 3)]
    P = np.stack([p[0] for p in Ps])
    lb, ub = np.stack([p[3] for p in Ps]), np.stack([p[4] for p in Ps])
    T = pr.general_standard_form(P, lb, ub, Ps[0][1], Ps[0][2], True)
    assert rc.same_bits(pr.general_cost_row(P[:, 0], lb, ub, Ps[0][2], True, T.shape[2] - 1), T[:, 0])
    with pytest.raises(ValueError, match="below ns"):
        pr.general_cost_row(P[0, 0], lb[0], ub[0], Ps[0][2], False, 3)


def test_the_hand_lp():
    T0 = np.array([[0.0, 1.0, 1.0, 0.0], [1.0, 1.0, -1.0, 1.0]])
    for c, status, z, x in rc.HAND_NEW:
        st, npiv, _, _, xs, obj, _ = rc.host_primal(T0, [2], np.concatenate([[0.0], c, [0.0]]))
        assert _lib.STATUS_NAMES[st] == status
        if z is not None:
            assert obj == z and xs[:2].tolist() == x and npiv == 1


# ---------------------------------------------------------------------------
# the inputs of test_gpu_batch_reopt_edges.py: where the lanes of the flat kernels fall
# ---------------------------------------------------------------------------

def assert_lane_edges(lanes, windows, edges, big, inside, tag):
    """the conditions on a ragged batch and its windows, from the lanes per LP alone"""
    B, F = len(lanes), rc.FLAT
    assert all(0 <= first and count >= 1 and first + count <= B for first, count in windows), tag
    assert any(first > 0 and rc.starts(lanes, first, count)[-1] > 2 * F for first, count in windows), tag
    seen = set()
    for first, at in edges.items():
        count = next(c for f, c in windows if f == first)
        s = rc.starts(lanes, first, count)
        assert set(at) <= set(s[:-1]), (tag, first)
        seen |= set(at)
    assert {F - 1, F, F + 1} <= seen and seen & {2 * F - 1, 2 * F, 2 * F + 1}, (tag, seen)
    whole = rc.starts(lanes, 0, B)
    assert lanes[big] > F and (big, 1) in windows, tag                                  # alone, more than a workgroup
    assert whole[big] // F != (whole[big + 1] - 1) // F, tag                            # and in two of the whole batch
    assert F <= whole[inside] and whole[inside + 1] <= 2 * F and (inside, 1) in windows, tag


def test_the_cost_block_crosses_workgroups_where_it_says():
    assert len(rc.COST_SHAPES) == rc.COST_WINDOWS[0][1] and rc.COST_SHAPES[rc.COST_BIG] == (2, 520)
    assert_lane_edges(rc.cost_lanes(), rc.COST_WINDOWS, rc.COST_EDGES, rc.COST_BIG, rc.COST_INSIDE, "k_cost")
    u = rc.COST_UNIFORM
    lanes = u["m"] + u["ns"] + 1
    assert rc.FLAT % lanes != 0 and u["B"] * lanes > 2 * rc.FLAT
    first, count = u["windows"][1]
    assert first > 0 and count * lanes > 2 * rc.FLAT and first + count == u["B"]
    first, count = u["windows"][2]
    assert first > 0 and first * lanes < rc.FLAT < (first + count) * lanes      # the two LPs around lane 256


def test_the_cost_block_ends_optimal_and_its_new_costs_move_row_0():
    tabs = rc.cost_block_tableaux()
    opt = []
    for i, (T, (m, ns)) in enumerate(zip(tabs, rc.COST_SHAPES)):
        o = F64Tableau(T)
        st, log, _ = o.solve()
        assert st == _lib.OPTIMAL, i
        opt.append((o.T, rc.basis_of(np.arange(ns, ns + m), log)))
    for k, (first, count) in enumerate(rc.COST_WINDOWS):
        moved = 0
        for i in range(first, first + count):
            T, basis = opt[i]
            moved += not rc.same_bits(rc.reprice(T, basis, rc.some_costs(T.shape[1] - 1, 100 * k + i))[0], T[0])
        assert moved >= 1, (first, count)


def test_the_general_block_crosses_workgroups_where_it_says():
    lps = rc.general_block_lps()
    assert len(lps) == rc.GENERAL_WINDOWS[0][1] and rc.GENERAL_FORMS[rc.GENERAL_BIG] == ("boxed", 258, 2)
    assert_lane_edges(rc.restage_lanes(lps), rc.GENERAL_WINDOWS, rc.RESTAGE_EDGES, rc.GENERAL_BIG, rc.RESTAGE_INSIDE,
                      "k_general_restage")
    assert_lane_edges(rc.shift_lanes(lps), rc.GENERAL_WINDOWS, rc.SHIFT_EDGES, rc.GENERAL_BIG, rc.SHIFT_INSIDE,
                      "k_general_shift, k_rhs")
    assert rc.GENERAL_WALKED in rc.GENERAL_WINDOWS and rc.GENERAL_WALKED[0] > 0
    assert rc.starts(rc.shift_lanes(lps), *rc.GENERAL_WALKED)[-1] > 2 * rc.FLAT
    # both kinds and both directions, LP by LP
    assert sum(lp[5] for lp in lps) >= 40 and sum(not lp[5] for lp in lps) >= 40
    assert {int(k) for lp in lps for k in lp[2]} == {gc.LOWER, gc.BOXED, gc.UPPER}


def test_the_general_block_ends_optimal_and_walks_to_a_verdict_under_every_window():
    lps, optima = rc.general_block_lps(), rc.general_block_optima()
    for k, (first, count) in enumerate(rc.GENERAL_WINDOWS):
        tight = rc.general_tight(lps, k)
        moved = 0
        for i in range(first, first + count):
            P, sense, kind, lb, ub, mx = lps[i]
            T, basis = optima[i]
            lb2, ub2 = tight[i]
            # the kinds stay: a finite bound stays finite, an infinite one stays
            assert np.array_equal(np.isfinite(lb2), np.isfinite(lb)) and np.array_equal(np.isfinite(ub2), np.isfinite(ub))
            assert (lb2 <= ub2).all(), i
            cap = 10 * (T.shape[0] - 1 + T.shape[1] - 1)
            w = rc.host_general_dual(T, basis, P, sense, kind, lb2, ub2, mx, cap)
            assert w["status"] in (_lib.OPTIMAL, _lib.INFEASIBLE) and 2 * w["npiv"] < cap, (k, i)
            moved += not rc.same_bits(rc.host_general_rhs(T, P, sense, kind, lb2, ub2, mx)[:, 0], T[:, 0])
        assert moved >= 1, (first, count)


def test_the_walked_general_window_pivots_in_every_workgroup_and_ends_both_ways():
    """the bounds of the walk cut optima off: LPs that pivot begin in each of the three workgroups of the row
    map, the large LP among them, and both verdicts occur"""
    lps, optima = rc.general_block_lps(), rc.general_block_optima()
    bounds = rc.general_squeezed(lps)
    first, count = rc.GENERAL_WALKED
    at = rc.starts(rc.shift_lanes(lps), first, count)
    pivoted, verdicts = {}, set()
    for k, i in enumerate(range(first, first + count)):
        P, sense, kind, lb, ub, mx = lps[i]
        T, basis = optima[i]
        lb2, ub2 = bounds[i]
        assert np.array_equal(np.isfinite(lb2), np.isfinite(lb)) and np.array_equal(np.isfinite(ub2), np.isfinite(ub))
        assert (lb2 <= ub2).all(), i
        cap = 10 * (T.shape[0] - 1 + T.shape[1] - 1)
        w = rc.host_general_dual(T, basis, P, sense, kind, lb2, ub2, mx, cap)
        assert w["status"] in (_lib.OPTIMAL, _lib.INFEASIBLE) and 2 * w["npiv"] < cap, i
        assert w["npiv"] <= 128, i                                  # the GPU test keeps the whole log
        verdicts.add(w["status"])
        if w["npiv"] > 0:
            pivoted[i] = at[k] // rc.FLAT
    assert at[-1] > 2 * rc.FLAT and set(pivoted.values()) == {0, 1, 2}
    assert rc.GENERAL_BIG in pivoted and 2 * len(pivoted) >= count
    assert verdicts == {_lib.OPTIMAL, _lib.INFEASIBLE}


def test_the_extreme_costs_and_borders_hold_what_they_say():
    """the expected arrays of the GPU test hold an infinity, a NaN the loop itself made and a subnormal"""
    m, ns = rc.SMALL
    rows, borders = [], []
    for i in range(2 * len(rc.EXTREME_COSTS)):
        c = rc.cost_case(m, ns, 1 + i, "tilt")
        row = rc.extreme_costs(m + ns, i, 1 + i)
        assert np.isfinite(row).all()
        rows.append(rc.reprice(c["opt"], c["basis"], row)[0])
    got = np.concatenate(rows)
    assert np.isinf(got).any() and np.isnan(got).any() and rc.is_subnormal(got).any()
    for i in range(8):
        b = rc.branch_case(m, ns, 1 + i, "down")
        P, lb, ub = rc.extreme_bounds(b["P"], np.zeros(ns), np.full(ns, 2.0), i)
        assert np.isfinite(P).all() and np.isfinite(lb).all() and np.isfinite(ub).all()
        with np.errstate(all="ignore"):
            borders.append(rc.host_general_rhs(b["opt"], P, b["sense"], b["kind"], lb, ub)[:, 0])
    got = np.concatenate(borders)
    assert np.isinf(got).any() and np.isnan(got).any() and rc.is_subnormal(got).any()
