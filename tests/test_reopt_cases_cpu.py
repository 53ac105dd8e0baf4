"""The inputs of the warm re-optimisation tests on the oracle alone: what a GPU
test compares the device with must itself be right, and must not be trivial --
a batch in which no LP pivots would let a kernel that does nothing pass."""
import numpy as np
import pytest

import _general_cases as gc
import _reopt_cases as rc
from lpsol_amd import _lib
from lpsol_amd import problem as pr

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
