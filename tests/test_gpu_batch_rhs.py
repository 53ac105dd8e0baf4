"""lp_resolve_set_rhs, ProblemResult.resolve and solve_problems(method="dual") on
the GPU (csrc/batch.hip: k_rhs, bdual).

set_rhs is compared bit for bit with the host loop of tests/_dual_cases.py
applied to the tableau downloaded just before the call; resolve with that loop
followed by the host walk, and with a cold solve of the same LPs within the
project's objective tolerance of 1e-9 relative (README)."""
import numpy as np
import pytest

import _dual_cases as dc
import _problem_cases as pc
from lpsol_amd import _lib, solution_x, solve_problems, solve_problems_ragged
from lpsol_amd import generators as gen
from lpsol_amd.problem import assemble_tableaux

pytestmark = pytest.mark.gpu

REL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def new_rhs(b, seed0, how="scale", z=0.0):
    """[B, m+1]: each LP's b perturbed on its own seed, under the stored _z cell z"""
    return np.stack([np.concatenate([[z], dc.PERTURB[how](b[i], seed0 + i)]) for i in range(len(b))])


snapshot, assert_untouched, assert_set_rhs = dc.snapshot, dc.assert_untouched, dc.assert_set_rhs
host_resolve = dc.host_resolve


# ---------------------------------------------------------------------------
# 1, 2, 3. set_rhs after the plain path and after the two-phase path, whole batch and window
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,ns,B,place", [(8, 10, 64, "lds"), (40, 40, 8, "lds"), (40, 40, 4, "device")],
                         ids=["8x10", "40x40", "40x40-device"])
def test_after_the_plain_path(m, ns, B, place):
    T, sense, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=8, place=place)
    assert res.path == "plain" and res.status == ["optimal"] * B
    slack = dc.slack_table(sense, ns)
    before, after = assert_set_rhs(res._engine, [slack] * B, new_rhs(b, 1, "shift", 0.25))
    assert any((t[1:, 0] < 0).any() for t in after["T"])
    # a window: the LPs outside it stay bit for bit
    assert_set_rhs(res._engine, [slack] * B, new_rhs(b, 100)[2:B - 1], first=2)
    assert_set_rhs(res._engine, [slack] * B, new_rhs(b, 200)[B - 1:], first=B - 1)
    res._engine.set_rhs(np.empty((0, m + 1)), first=B)          # count 0: a no-op, at the end of the batch too
    # the original right-hand sides bring the optimal column back, up to the order of summation
    res._engine.set_rhs(np.concatenate([np.zeros((B, 1)), b], axis=1))
    back = res._engine.download()
    assert np.allclose(back[:, :, 0], np.stack(before["T"])[:, :, 0], rtol=0, atol=1e-9)


@pytest.mark.parametrize("kind,m,ns,B", [("ge", 8, 10, 32), ("neg", 8, 10, 32), ("ge", 24, 24, 8)])
def test_after_the_two_phase_path(kind, m, ns, B):
    T, sense, _ = pc.stack(kind, m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    assert (b < 0).any()                    # rows that phase 1 negates
    res = solve_problems(c, A, b, sense, log_cap=8)
    assert res.path == "twophase" and res.status == ["optimal"] * B and (res.rows == len(sense)).all()
    slack = dc.slack_table(sense, ns)
    assert_set_rhs(res._engine, [slack] * B, new_rhs(b, 1, "shift", -1.5))
    assert_set_rhs(res._engine, [slack] * B, new_rhs(b, 50)[1:B - 2], first=1)


# ---------------------------------------------------------------------------
# 4. a ragged batch
# ---------------------------------------------------------------------------

def ragged_problems():
    """LPs of many shapes under <= and >= senses, m = 1 and 1 x 1 blocks among them"""
    shapes = [(8, 10), (1, 1), (3, 5), (40, 40), (1, 6), (5, 4), (8, 10), (24, 24), (2, 1)]
    items = []
    for i, (m, ns) in enumerate(shapes):
        kind = ("mixed", "ge", "neg")[i % 3] if m > 2 else "mixed"
        T, sense, _ = pc.lp(kind, m, ns, 40 + i)
        items.append((*pc.parts(T, ns), sense))
    return items


@pytest.mark.parametrize("place", ["lds", "device"])
def test_on_a_ragged_batch(place):
    items = ragged_problems()
    res = solve_problems_ragged(items, log_cap=8, place=place)
    assert res.path == "twophase" and res.status == ["optimal"] * len(items)
    slacks = [dc.slack_table(s, len(c)) for c, _, _, s in items]
    rhs = [np.concatenate([[0.5 * i], dc.shift(b, 7 + i)]) for i, (_, _, b, _) in enumerate(items)]
    assert_set_rhs(res._engine, slacks, rhs)
    rhs = [np.concatenate([[-1.0], dc.scale(b, 70 + i)]) for i, (_, _, b, _) in enumerate(items)]
    assert_set_rhs(res._engine, slacks, rhs[3:7], first=3)
    assert_set_rhs(res._engine, slacks, rhs[8:], first=8)
    assert_set_rhs(res._engine, slacks, rhs[:2], first=0)


# ---------------------------------------------------------------------------
# 5. refusals change nothing
# ---------------------------------------------------------------------------

def test_refusals_change_nothing():
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2, 3))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=4)
    eng = res._engine
    before = snapshot(eng)
    rhs = new_rhs(b, 1)
    for first, k in ((-1, 1), (3, 1), (1, 3), (4, 0)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.set_rhs(rhs[:k], first)
    assert eng.lib.lp_resolve_set_rhs(eng.h, 0, 2, None) == _lib.BAD_ARG
    eng.set_senses(None)
    with pytest.raises(ValueError, match="no senses"):
        eng.set_rhs(rhs)
    eng.set_senses(sense)
    assert_untouched(snapshot(eng), before, range(3))
    # an == row owns no column: the message names the LP and the row
    P, s = pc.mixed_sense_block(3)
    eq = solve_problems(P[None, 0, 1:], P[None, 1:, 1:], P[None, 1:, 0], s, log_cap=4)
    before = snapshot(eq._engine)
    with pytest.raises(ValueError, match="LP 0, row 1 is an equality"):
        eq._engine.set_rhs(np.zeros((1, len(s) + 1)))
    assert_untouched(snapshot(eq._engine), before, range(1))
    with pytest.raises(ValueError, match='"==" row'):
        eq.resolve(P[None, 1:, 0])
    assert eq.y is not None and not eq._stale
    # ragged: the first LP with an equality is named
    blocks = [(c[0], A[0], b[0], None), (P[0, 1:], P[1:, 1:], P[1:, 0], s)]
    rag = solve_problems_ragged(blocks, log_cap=4)
    before = snapshot(rag._engine)
    with pytest.raises(ValueError, match="LP 1, row 1 is an equality"):
        rag._engine.set_rhs([np.zeros(4), np.zeros(len(s) + 1)])
    rag._engine.set_rhs([np.zeros(4)])              # a window without it is fine
    after = snapshot(rag._engine)
    assert dc.same_bits(after["T"][1], before["T"][1])


# ---------------------------------------------------------------------------
# 6. resolve
# ---------------------------------------------------------------------------

def assert_resolve(new, before, slack, rhs, ns, cap):
    for i in range(len(new)):
        st, npiv, x, z = host_resolve(before["T"][i], before["basis"][i], slack, rhs[i], cap)
        assert (new.status_code[i], new.npiv[i]) == (st, npiv), i
        assert dc.same_bits(new.x[i], x[:ns]) and dc.same_bits(new.objective[i], z), i
        rows = [r for r in range(len(slack))]
        assert dc.same_bits(new.slack[i], x[[abs(slack[r]) - 1 for r in rows]]), i
    assert new.path == "dual" and not new.nstd.any() and not new.ninit.any() and not new.stage.any()


@pytest.mark.parametrize("m,ns,B,how", [(8, 10, 64, "scale"), (8, 10, 64, "shift"), (40, 40, 16, "scale"),
                                         (40, 40, 16, "shift")])
def test_resolve_is_the_host_loop_and_walk_and_agrees_with_a_cold_solve(m, ns, B, how):
    T, sense, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=dc.LOG_CAP)
    slack = dc.slack_table(sense, ns)
    before = snapshot(res._engine)
    old = dict(x=res.x.copy(), objective=res.objective.copy(), status=list(res.status))
    b2 = np.stack([dc.PERTURB[how](b[i], 1 + i) for i in range(B)])
    assert all(dc.same_bits(b2[i], dc.warm(m, ns, 1 + i, how)["b"]) for i in range(B))      # the vetted inputs
    new = res.resolve(b2)
    cap = 10 * (m + ns + m)
    assert_resolve(new, before, slack, np.concatenate([np.zeros((B, 1)), b2], axis=1), ns, cap)
    assert set(new.status) <= {"optimal", "infeasible"}
    assert new.log(1).tolist() == dc.walk(dc.set_rhs(before["T"][1], slack, np.concatenate([[0.0], b2[1]])), cap)["log"]
    # the old result keeps what it holds, and y was fetched for it
    assert res._y is not None and dc.same_bits(res.x, old["x"]) and res.status == old["status"]
    for use in (lambda: res.reduced_costs, lambda: res.tableau(0), lambda: res.log(0), lambda: res.resolve(b)):
        with pytest.raises(RuntimeError, match="resolve"):
            use()
    # against the cold call
    cold = solve_problems(c, A, b2)
    assert cold.path == ("plain" if how == "scale" else "twophase")
    assert [s == "infeasible" for s in new.status] == [s == "infeasible" for s in cold.status]
    if how == "shift":
        assert "infeasible" in new.status
    for i in range(B):
        if new.status[i] == cold.status[i] == "optimal":
            assert rel(new.objective[i], cold.objective[i]) <= REL, i
    # a second resolve, on the new result: back to the original right-hand sides
    mid = snapshot(new._engine)
    again = new.resolve(b, max_pivots=200)
    assert_resolve(again, mid, slack, np.concatenate([np.zeros((B, 1)), b], axis=1), ns, 200)
    assert again.status == ["optimal"] * B
    assert all(rel(again.objective[i], old["objective"][i]) <= REL for i in range(B))
    with pytest.raises(RuntimeError, match="resolve"):
        new.basis


def test_resolve_with_the_original_b_takes_no_pivot():
    T, sense, ns = pc.stack("mixed", 8, 10, range(1, 33))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b)
    new = res.resolve(b)
    assert new.status == ["optimal"] * 32 and not new.npiv.any()
    assert np.allclose(new.x, res.x, rtol=0, atol=1e-9) and np.allclose(new.objective, res.objective, rtol=0, atol=1e-9)
    assert np.array_equal(new.basis, res.basis)         # fetched on first use, from the live engine
    capped = new.resolve(np.stack([dc.shift(b[i], 1 + i) for i in range(32)]), max_pivots=1, c0=2.5)
    assert {"pivoted", "optimal"} <= set(capped.status) and capped.npiv.max() == 1
    zero = capped.resolve(b, max_pivots=0)
    assert zero.status == ["pivoted"] * 32 and not zero.npiv.any()
    assert np.allclose(zero.resolve(b).objective, res.objective + 2.5, rtol=0, atol=1e-9)     # c0 is kept


def test_resolve_after_the_two_phase_path():
    B, m, ns = 32, 8, 10
    T, sense, _ = pc.stack("ge", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, sense)
    assert res.path == "twophase" and res.status == ["optimal"] * B
    slack = dc.slack_table(sense, ns)
    before = snapshot(res._engine)
    b2 = np.stack([dc.scale(b[i], 1 + i) for i in range(B)])
    new = res.resolve(b2)
    assert_resolve(new, before, slack, np.concatenate([np.zeros((B, 1)), b2], axis=1), ns, 10 * (m + 1 + ns + m + 1))
    cold = solve_problems(c, A, b2, sense)
    assert [s == "infeasible" for s in new.status] == [s == "infeasible" for s in cold.status]
    assert "infeasible" in new.status and "optimal" in new.status
    for i in range(B):
        if new.status[i] == cold.status[i] == "optimal":
            assert rel(new.objective[i], cold.objective[i]) <= REL, i


def test_resolve_on_a_ragged_result():
    items = ragged_problems()
    res = solve_problems_ragged(items)
    before = snapshot(res._engine)
    b2 = [dc.scale(b, 90 + i) for i, (_, _, b, _) in enumerate(items)]
    new = res.resolve(b2, c0=1.0)
    cap = max(10 * (m + n) for m, n in res._engine.shapes)
    for i, (c, _, _, s) in enumerate(items):
        slack = dc.slack_table(s, len(c))
        st, npiv, x, z = host_resolve(before["T"][i], before["basis"][i], slack, np.concatenate([[-1.0], b2[i]]), cap)
        assert (new.status_code[i], new.npiv[i]) == (st, npiv), i
        assert dc.same_bits(new.x[i], x[:len(c)]) and dc.same_bits(new.objective[i], z), i
    assert type(new) is type(res) and new.path == "dual"
    cold = solve_problems_ragged([(c, A, b2[i], s) for i, (c, A, _, s) in enumerate(items)], c0=[1.0] * len(items))
    for i in range(len(items)):
        assert (new.status[i] == "infeasible") == (cold.status[i] == "infeasible"), i
        if new.status[i] == cold.status[i] == "optimal":
            assert rel(new.objective[i], cold.objective[i]) <= REL, i
    with pytest.raises(RuntimeError, match="resolve"):
        res.tableau(0)


def test_resolve_refuses_a_general_form_result():
    T, sense, ns = pc.stack("mixed", 3, 5, (1, 2))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, c0=1.0)
    with pytest.raises(ValueError, match="general-form"):
        res.resolve(b)
    assert res.reduced_costs is not None            # still live


# ---------------------------------------------------------------------------
# 7. method="dual": the cold start from the slack basis
# ---------------------------------------------------------------------------

def test_method_dual_on_covering_lps():
    B, m, ns = 64, 8, 10
    lps = [dc.covering(m, ns, s) for s in range(1, B + 1)]
    c, A, b = (np.stack([lp[k] for lp in lps]) for k in range(3))
    res = solve_problems(c, -A, -b, method="dual", log_cap=32)
    assert res.path == "dual" and res.status == ["optimal"] * B and res.npiv.max() <= 8 and res.npiv.min() >= 1
    for i in range(B):
        T = dc.covering_tableau(m, ns, 1 + i)
        assert dc.same_bits(T, assemble_tableaux(np.concatenate([[[0.0, *c[i]]], np.c_[-b[i], -A[i]]])[None],
                                                 ["<="] * m)[0])
        w = dc.walk(T, 10 * (m + ns + m))
        basis = np.arange(ns, ns + m)
        for r, col in w["log"]:
            basis[r] = col
        x = solution_x(w["T"], basis)
        assert (res.status_code[i], res.npiv[i], res.log(i).tolist()) == (w["status"], w["npiv"], w["log"]), i
        assert dc.same_bits(res.x[i], x[:ns]) and dc.same_bits(res.slack[i], x[ns:]), i
        assert dc.same_bits(res.objective[i], -w["T"][0, 0]) and res.basis[i].tolist() == basis.tolist(), i
    two = solve_problems(c, A, b, [">="] * m)
    assert two.path == "twophase" and two.status == ["optimal"] * B
    assert all(rel(res.objective[i], two.objective[i]) <= REL for i in range(B))
    assert not res.nstd.any() and not res.ninit.any() and (res.rows == m).all()
    # the result resolves like any other
    new = res.resolve(-b * 0.5)
    assert new.status == ["optimal"] * B and all(rel(new.objective[i], 0.5 * res.objective[i]) <= REL for i in range(B))


def test_method_dual_ragged_and_a_negative_cost():
    lps = [dc.covering(m, ns, 5 + m) for m, ns in ((8, 10), (3, 5), (1, 1), (24, 24))]
    items = [(c, -A, -b, None) for c, A, b in lps]
    bad = (np.array([1.0, -0.5]), -np.ones((1, 2)), -np.ones(1), None)          # a negative cost: not dual feasible
    res = solve_problems_ragged(items + [bad], method="dual")
    assert res.path == "dual" and res.status == ["optimal"] * 4 + ["bad_arg"] and res.npiv[4] == 0
    two = solve_problems_ragged([(c, A, b, [">="] * len(b)) for c, A, b in lps])
    cap = 10 * max(m + n for m, n in res._engine.shapes)        # the default: of the largest LP
    assert cap == 10 * (24 + 48)
    for i in range(4):
        m, ns = lps[i][1].shape
        w = dc.walk(dc.covering_tableau(m, ns, 5 + m), cap)
        assert (res.status_code[i], res.npiv[i]) == (w["status"], w["npiv"]), i
        assert dc.same_bits(res.objective[i], -w["T"][0, 0]), i
        assert rel(res.objective[i], two.objective[i]) <= REL, i
