"""The inputs of test_gpu_twophase_contract.py still reach what they are there
for (tests/_twophase_cases.py), and the reporting mode of oracle/phase1.py
equals the asserting one wherever that one does not assert.  No GPU.

Of test_gpu_twophase.py's inputs only degenerate(5, 8) is left out of the
comparison of the two modes: the strict oracle asserts on it, after 2^20
pivots."""
import numpy as np
import pytest

from conftest import fixture_input, load_golden

import _twophase_cases as tc
import test_gpu_twophase as tg
from lpsol_amd import _lib
from lpsol_amd import generators as gen
from oracle import phase1

SMALL = load_golden("small.json")


# ---------------------------------------------------------------------------
# report mode equals strict mode
# ---------------------------------------------------------------------------

def same_as_strict(T, tol=None):
    """-> False where the strict oracle asserts, else compares field for field"""
    T0 = np.array(T, copy=True)
    try:
        s = phase1.solve_lp(T, tol)
    except AssertionError:
        return False
    r = phase1.solve_lp(T, tol, report=True)
    assert tc.same_bits(np.asarray(T), T0)              # neither touches its input
    assert r["init_seq"] == s["init_seq"]
    if "error" in s:
        assert (r["status"], r["stage"]) == (tc.INFEASIBLE, tc.ARTIFICIAL)
        assert tc.same_bits(r["T"], np.asarray(T, dtype=np.float64)) and r["seq"] == []
        return True
    assert (r["status"], r["stage"], r["canonical"]) == (tc.OPTIMAL, tc.PHASE2, True)
    m, rows = T.shape[0] - 1, s["T"].shape[0] - 1
    assert r["rows"] == rows and r["bfs"] == s["bfs"] + [-1] * (m - rows)
    assert tc.same_bits(r["T"], s["T"])
    assert tc.same_bits(np.array([r["objective"]]), np.array([s["objective"]]))
    assert (r["seq"], r["init_bfs"], r["init_size"]) == (s["seq"], s["init_bfs"], s["init_size"])
    assert 0 <= r["nart"] <= len(r["init_seq"]) and 0 <= r["nstd"] <= len(r["seq"])
    return True


def strict_keys_unchanged(T):
    """the default call gives the keys it always gave"""
    s = phase1.solve_lp(T)
    if "error" in s:
        assert set(s) == {"error", "init_seq"}
    else:
        assert set(s) == {"T", "bfs", "init_seq", "init_bfs", "init_size", "seq", "objective"}
    f = phase1.find_bfs(T)
    assert set(f) in ({"error", "init_seq"}, {"T", "bfs", "init_seq"})


@pytest.mark.parametrize("fx", SMALL["phase1"], ids=[fx["name"] for fx in SMALL["phase1"]])
def test_report_mode_on_the_goldens(fx):
    T = fixture_input(fx)
    strict_keys_unchanged(T)
    assert same_as_strict(T)


def test_report_mode_on_the_batches_of_test_gpu_twophase():
    stacks = [tg.batch1(), tg.batch2(),
              np.stack([gen.phase1_lp("eq", 1, 8, 1), gen.phase1_lp("infeasible", 2, 8, 1),
                        gen.phase1_lp("eq", 1, 8, 2), gen.phase1_lp("eq", 1, 8, 3)]),
              np.stack([gen.phase1_lp("eq", 30, 72, s) for s in range(1, 5)] +
                       [gen.phase1_lp("dep", 29, 72, s) for s in range(1, 5)]),
              np.stack([gen.phase1_lp("ge", 32, 32, s) for s in range(1, 4)] +
                       [gen.phase1_lp("neg", 32, 32, s) for s in range(1, 4)] +
                       [gen.tableau("mixed", 33, 32, 1)]),
              np.stack([tg.degenerate(s, 16) for s in range(1, 9)]),
              np.stack([tg.degenerate(s, 8) for s in range(1, 5)])]
    for stack in stacks:
        for T in stack:
            assert same_as_strict(T)
    tol = dict(zero=1e-7, pivot=1e-7)                   # test_tolerances_reach_every_stage
    for T in tg.batch2():
        assert same_as_strict(T, tol)


@pytest.mark.parametrize("kind", ["ge", "neg", "eq", "dep"])
def test_report_mode_on_generated_lps(kind):
    seen = set()
    for m, ns in ((5, 6), (5, 8)):
        for s in range(1, 65):
            T = gen.phase1_lp(kind, m, ns, s)
            assert same_as_strict(T)                    # the strict oracle asserts on none of them
            r = phase1.solve_lp(T, report=True)
            seen.add((r["status"], r["stage"]))
    assert seen <= {(tc.OPTIMAL, tc.PHASE2), (tc.INFEASIBLE, tc.ARTIFICIAL)}


def test_a_cap_caps_each_solve_and_not_the_drive_out():
    T = gen.phase1_lp("eq", 5, 8, 228)                  # two drive-out pivots (test_gpu_twophase)
    full = phase1.solve_lp(T, report=True)
    nart, ndrive = full["nart"], len(full["init_seq"]) - full["nart"]
    assert ndrive == 2 and nart >= 2
    r = phase1.solve_lp(T, cap=nart, report=True)       # cap == pivots needed: the cap is met first
    assert (r["status"], r["stage"]) == (tc.CAP_REACHED, tc.ARTIFICIAL)
    assert r["init_seq"] == full["init_seq"][:nart] and tc.same_bits(r["T"], T)
    assert r["bfs"] != full["bfs"] and r["rows"] == 6 and r["seq"] == []
    r = phase1.solve_lp(T, cap=nart + 1, report=True)   # fewer than nart + ndrive: not capped
    for k in ("status", "stage", "init_seq", "seq", "bfs", "rows", "nstd"):
        assert r[k] == full[k], k
    assert tc.same_bits(r["T"], full["T"])
    with pytest.raises(AssertionError):                 # the strict mode asserts under a cap too
        phase1.solve_lp(T, cap=1)
    T = gen.phase1_lp("ge", 5, 6, 1)                    # 3 artificial pivots, 8 of phase 2
    full = phase1.solve_lp(T, report=True)
    assert (full["nart"], len(full["init_seq"]), len(full["seq"])) == (3, 3, 8)
    r = phase1.solve_lp(T, cap=5, report=True)          # each solve has the cap to itself
    assert (r["status"], r["stage"]) == (tc.CAP_REACHED, tc.PHASE2)
    assert r["init_seq"] == full["init_seq"] and r["seq"] == full["seq"][:5] and r["nstd"] == 5
    assert r["T"].shape == full["T"].shape and not tc.same_bits(r["T"], full["T"])


# ---------------------------------------------------------------------------
# coverage: the outcome batches
# ---------------------------------------------------------------------------

def reached(batches, waves):
    pairs, not_canonical = set(), 0
    for b in batches:
        stack = b["stack"]
        m, n = stack.shape[1] - 1, stack.shape[2] - 1
        assert _lib.twophase_waves(m, n) == waves, b["name"]
        recs, cap = tc.oracle_batch(stack, b["tol"], b["cap"])
        assert cap <= tc.LOG_CAP and all(len(o["init_seq"]) + len(o["seq"]) <= tc.LOG_CAP for o in recs)
        for i, o in enumerate(recs):
            got = (o["status"], o["stage"])
            if i in b["want"]:
                assert got == b["want"][i], (b["name"], i)
                pairs.add(got)
            elif b["optimal_neighbours"]:
                assert got == (tc.OPTIMAL, tc.PHASE2), (b["name"], i)
            assert (o["canonical"] is False) == (i in b["canon"]), (b["name"], i)
            not_canonical += o["canonical"] is False
        # a target sits between two neighbours
        marked = set(b["want"]) | b["canon"]
        assert 0 not in marked or not b["optimal_neighbours"]
        assert len(stack) - 1 not in marked or not b["optimal_neighbours"]
    return pairs, not_canonical


def test_one_wave_batches_reach_every_outcome():
    pairs, not_canonical = reached(tc.outcome_batches(), 1)
    assert pairs == set(tc.ONE_WAVE_PAIRS)              # both non-optimal artificial endings are found
    assert not_canonical >= 6


def test_four_wave_batches_reach_their_outcomes():
    pairs, _ = reached(tc.four_wave_batches(), 4)
    assert (tc.UNBOUNDED, tc.PHASE2) in pairs
    assert {(tc.CAP_REACHED, tc.ARTIFICIAL), (tc.UNBOUNDED, tc.ARTIFICIAL),
            (tc.OBJ_INCREASED, tc.ARTIFICIAL)} <= pairs


def test_unbounded_phase2_with_and_without_phase1_pivots():
    b = tc.outcome_batches()[0]
    recs, _ = tc.oracle_batch(b["stack"], b["tol"], b["cap"])
    assert b["name"] == "unbounded_phase2"
    assert [len(recs[i]["init_seq"]) for i in (1, 3, 4, 6)] == [3, 5, 0, 4]
    assert [len(recs[i]["seq"]) for i in (1, 3, 4, 6)] == [2, 1, 2, 0]


def test_phase1_failed_after_drive_out_pivots():
    """dep(3, 4, 168) makes a drive-out pivot before the row that fails"""
    b = next(x for x in tc.outcome_batches() if x["name"] == "phase1_failed_pivot")
    o = tc.report(b["stack"][3], b["tol"], tc.PROBE_CAP)
    assert (o["nart"], len(o["init_seq"])) == (8, 9)


# ---------------------------------------------------------------------------
# pinned cases: the scan and the set-up
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("waves", [1, 4])
def test_scan_cases_are_what_their_docstrings_say(waves):
    n = tc.SCAN_N[waves]
    assert _lib.twophase_waves(tc.SCAN_M, n) == waves
    assert _lib.twophase_lds_bytes(tc.SCAN_M, n) <= _lib.BATCH_LDS_MAX
    assert tc.SCAN_HIGH[waves] >= 64 * waves > 20 and tc.SCAN_HIGH[waves] < n
    pins = tc.scan_pins(waves)
    assert list(pins) == tc.SCAN_NAMES
    stack, rev = tc.scan_stack(waves), tc.scan_stack(waves, reverse=True)
    plain = np.where(stack == 5e-324, 0.0, stack)
    assert np.all(plain * 4 == np.round(plain * 4))     # dyadic, but for the one denormal
    for name, T, R in zip(tc.SCAN_NAMES, stack, rev):
        p = pins[name]
        basis, k = tc.scan_basis(T)
        assert (k, basis) == (p["k"], p["basis"]), name
        rb, rk = tc.scan_basis(R)
        assert rk == k and sorted(j for j in rb if j < n) == sorted(j for j in basis if j < n), name
        for X, b0 in ((T, basis), (R, rb)):
            o = tc.report(X, None, tc.PROBE_CAP)
            assert (o["status"], o["stage"], o["rows"]) == (p["status"], p["stage"], p["rows"]), name
            assert o["canonical"] and (len(o["init_seq"]) > 0) == (k > 0), name
            z = tc.report(X, None, 0)                   # a cap of 0 shows the set-up alone
            assert z["status"] == tc.CAP_REACHED and z["bfs"] == b0, name
            assert z["stage"] == (tc.ARTIFICIAL if k else tc.PHASE2), name
    by = dict(zip(tc.SCAN_NAMES, stack))
    # signed zeros: b = -0.0 keeps its bits through the set-up, and the flipped
    # row's zeros come out as -0.0
    z = tc.report(by["b_negzero"], None, 0)
    assert np.signbit(z["T"][3, 0]) and z["T"][3, 0] == 0.0
    z = tc.report(by["flip_makes_unit"], None, 0)
    assert z["stage"] == tc.PHASE2 and z["T"][5, 0] == 2.0
    assert np.signbit(z["T"][5, 20]) and z["T"][5, 20] == 0.0 and z["T"][5, 9] == -1.0


def test_tiny_shapes_need_phase_1():
    for m, n in tc.TINY_SHAPES:
        T = tc.tiny_lp(m, n)
        assert T.shape == (m + 1, n + 1) and np.all(T * 4 == np.round(T * 4))
        basis, k = tc.scan_basis(T)
        assert k == m and basis == [n + i for i in range(m)]
        o = tc.report(T, None, tc.PROBE_CAP)
        assert (o["status"], o["stage"], o["rows"]) == (tc.OPTIMAL, tc.PHASE2, min(m, n)), (m, n)


# ---------------------------------------------------------------------------
# shapes at the kernel's own boundaries
# ---------------------------------------------------------------------------

def test_wave_boundary_shapes():
    a, b = gen.phase1_lp("eq", 30, 32, 1), gen.phase1_lp("eq", 30, 33, 1)
    assert a.shape == (32, 33) and 32 * (33 + 31) == 2048 and _lib.twophase_waves(31, 32) == 1
    assert b.shape == (32, 34) and 32 * (34 + 31) == 2080 and _lib.twophase_waves(31, 33) == 4


def test_largest_shapes_sit_on_the_lds_boundary():
    wide, tall = tc.wide_stack(), tc.tall_stack()
    assert wide.shape[1:] == (_lib.twophase_max_m(tc.WIDE_N) + 1, tc.WIDE_N + 1) == (91, 129)
    assert tall.shape[1:] == (_lib.twophase_max_m(tc.TALL_N) + 1, tc.TALL_N + 1) == (137, 9)
    assert _lib.twophase_lds_bytes(90, 128) == 162400 and _lib.twophase_lds_bytes(136, 8) == 161848
    assert _lib.twophase_waves(90, 128) == 4 and _lib.twophase_waves(136, 8) == 4
    recs, cap = tc.oracle_batch(wide)
    assert [o["rows"] for o in recs] == [90, 90, 89, 89] and cap <= tc.LOG_CAP
    assert all(o["status"] == tc.OPTIMAL and o["nart"] >= 136 and len(o["seq"]) >= 40 for o in recs)
    recs, _ = tc.oracle_batch(tall)
    assert [o["rows"] for o in recs] == [8, 8, 8]       # 128 rows dropped
    assert all(o["status"] == tc.OPTIMAL for o in recs)
    assert any(len(o["init_seq"]) > o["nart"] for o in recs)    # a drive-out pivot among them


def test_the_two_special_lps_of_the_large_batch():
    inf, canon = tc.wide_infeasible(), gen.tableau("mixed", 90, tc.WIDE_N - 90, 1)
    assert inf.shape == canon.shape == (91, tc.WIDE_N + 1)
    assert min(tc.WIDE_INFEASIBLE_AT, tc.WIDE_CANONICAL_AT) > 256
    o = tc.report(inf, None, tc.PROBE_CAP)
    assert (o["status"], o["stage"]) == (tc.INFEASIBLE, tc.ARTIFICIAL)
    o = tc.report(canon, None, tc.PROBE_CAP)
    assert (o["status"], o["stage"], o["init_seq"]) == (tc.OPTIMAL, tc.PHASE2, []) and o["seq"]


def test_nonfinite_cases_run_through_the_oracle():
    """the reporting oracle raises on none of them, and the cells are where
    their names say"""
    labels, stack = tc.nonfinite_stack()
    assert len(labels) == 14 and _lib.twophase_waves(4, 8) == 1
    basis, k = tc.scan_basis(stack[-1])
    assert (basis, k) == ([8, 5, 9, 7], 2)              # rows 0 and 2 need an artificial
    seen = set()
    for T in stack:
        o = tc.report(T, None, tc.NONFINITE_CAP)
        seen.add((o["status"], o["stage"]))
    assert len(seen) >= 3
