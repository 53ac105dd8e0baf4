"""lp_batch_run with LP_RULE_MAX_INCREASE on the GPU (csrc/batch.hip: bmaxinc in
front of bstep's ratio test).

Every comparison is status, done, the whole log, the basis and the final
tableau bit for bit (a NaN matching a NaN) against the host walk of
tests/_maxinc_cases.py over oracle/lp_f64.c's lpf_find_max_increase and
lpf_pivot.  tests/test_maxinc_cases_cpu.py shows that each input does on the
oracle what its name claims."""
import numpy as np
import pytest

import _maxinc_cases as mc
from lpsol_amd import _lib, solve_batch, solve_ragged
from lpsol_amd import generators as gen
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu

MAXINC = _lib.RULE_MAX_INCREASE


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def edge_lps():
    return [gen.tableau(kind, m, ns, seed) for kind, m, ns in mc.EDGES for seed in mc.EDGE_SEEDS]


# ---------------------------------------------------------------------------
# 1, 2. one wave and four waves, the tableau in LDS
# ---------------------------------------------------------------------------

def test_one_wave_in_lds():
    stack = mc.small_stack()                # 9 x 19
    recs = mc.device_run(stack, 64, log_cap=64)
    assert all(r["status"] == _lib.OPTIMAL for r in recs)
    mc.assert_records(recs, stack, 64)


def test_four_waves_in_lds():
    stack = mc.large_stack()                # 41 x 81
    assert stack.shape[1] * stack.shape[2] > 2048       # above the one-wave bound
    recs = mc.device_run(stack, 128)
    assert all(r["status"] == _lib.OPTIMAL for r in recs)
    mc.assert_records(recs, stack, 128)


# ---------------------------------------------------------------------------
# 3. caps, chunks and a second run
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stack_of", [mc.small_stack, mc.large_stack], ids=["8x10", "40x40"])
def test_caps_and_chunks(stack_of):
    stack = stack_of()[:8]
    for recs in (mc.device_run(stack, 0), mc.device_run(stack, 0, chunk=1)):
        assert all((r["status"], r["npiv"], r["log"]) == (_lib.PIVOTED, 0, []) for r in recs)
        mc.assert_records(recs, stack, 0)
    capped = mc.device_run(stack, 3)        # every LP here needs at least 3 pivots
    assert all((r["status"], r["npiv"]) == (_lib.PIVOTED, 3) for r in capped)
    mc.assert_records(capped, stack, 3)
    whole = mc.device_run(stack)
    mc.assert_records(whole, stack)
    for chunk in (1, 2):
        got = mc.device_run(stack, chunk=chunk)
        for a, b in zip(got, whole):
            assert (a["status"], a["npiv"], a["log"], a["basis"]) == (b["status"], b["npiv"], b["log"], b["basis"])
            assert mc.same_bits(a["T"], b["T"])


def test_a_second_run_continues_from_the_current_tableau():
    stack = mc.small_stack()[:16]
    eng = mc.make_engine(stack)
    try:
        mc.load(eng, stack)
        first = mc.records(eng, *eng.run(MAXINC, 2))
        mc.assert_records(first, stack, 2)
        second = mc.records(eng, *eng.run(MAXINC, mc.CAP))
    finally:
        eng.close()
    for i, (a, b) in enumerate(zip(first, second)):
        w = mc.walk(a["T"])                 # the oracle, started where the first run stopped
        assert (b["status"], b["npiv"], b["log"]) == (w["status"], w["npiv"], w["log"]), i
        assert mc.same_bits(b["T"], w["T"]), i
        whole = mc.walk(stack[i])
        assert a["log"] + b["log"] == whole["log"] and mc.same_bits(b["T"], whole["T"]), i


# ---------------------------------------------------------------------------
# 4. the constructed cases, mixed fates side by side in one ragged batch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tol", mc.TOLS, ids=["default", "ratio_tie=0", "cost=0"])
@pytest.mark.parametrize("place", ["lds", "device"])
def test_constructed_cases(tol, place):
    names = list(mc.CASES)
    lps = [mc.CASES[k] for k in names]
    recs = mc.device_run(lps, tol=tol, place=place)
    for name, rec, T in zip(names, recs, lps):
        mc.assert_record(rec, T, mc.CAP, tol, tag=name)
    by = dict(zip(names, recs))
    assert by["unbounded_wins"]["status"] == by["overflow"]["status"] == _lib.UNBOUNDED
    assert (by["no_column"]["status"], by["no_column"]["npiv"]) == (_lib.BAD_PIVOT, 0)
    assert mc.same_bits(by["no_column"]["T"], mc.NO_COLUMN)      # no pivot applied
    assert by["tie"]["status"] == _lib.OPTIMAL and by["tie"]["log"][0] == [0, 0]
    assert by["band_in"]["log"][0] == ([1, 2] if tol == dict(ratio_tie=0.0) else [0, 0])
    assert by["tol_cost"]["log"][0] == ([0, 0] if tol == dict(cost=0.0) else [1, 1])
    assert np.isnan(by["nan_cell"]["T"]).any()


# ---------------------------------------------------------------------------
# 5. the edges of the lane mapping
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,m,ns", mc.EDGES, ids=["%s_%dx%d" % e for e in mc.EDGES])
def test_lane_mapping_edges(kind, m, ns):
    stack = np.stack([gen.tableau(kind, m, ns, seed) for seed in mc.EDGE_SEEDS])
    recs = mc.device_run(stack)
    assert all(r["status"] == _lib.OPTIMAL for r in recs)
    mc.assert_records(recs, stack)


# ---------------------------------------------------------------------------
# 6. Klee-Minty
# ---------------------------------------------------------------------------

def test_klee_minty():
    stack = np.stack([gen.klee_minty(8), gen.klee_minty(8, degenerate=True)])
    recs = mc.device_run(stack)
    assert [(r["status"], r["npiv"]) for r in recs] == [(_lib.OPTIMAL, 1), (_lib.OPTIMAL, 20)]
    mc.assert_records(recs, stack)
    assert len(F64Tableau(stack[0]).solve(cap=4096, logcap=4096)[1]) == 255     # the standard solve's walk


# ---------------------------------------------------------------------------
# 7. ragged
# ---------------------------------------------------------------------------

def ragged_lps():
    lps = list(mc.small_stack()[:4]) + list(mc.large_stack()[:2]) + edge_lps() + list(mc.small_stack()[4:8])
    assert len(lps) == 40
    return lps


def test_ragged():
    lps = ragged_lps()
    res = solve_ragged(lps, rule=MAXINC, steps=128, log_cap=128, basis=[mc.start_basis(T.shape[0] - 1) for T in lps])
    waves = {b["waves"] for b in res.plan()}
    assert {1, 4} <= waves
    assert not res.nstd.any()
    for i, T in enumerate(lps):
        w = mc.walk(T, 128)
        assert (res.status_code[i], res.npiv[i], res.log(i).tolist()) == (w["status"], w["npiv"], w["log"]), i
        assert res.status[i] == "optimal", i
        assert mc.same_bits(res.tableaux[i], w["T"]), i
        assert res.basis[i].tolist() == mc.basis_after(T.shape[0] - 1, w["log"]), i
        assert res.objective[i] == -w["T"][0, 0], i


# ---------------------------------------------------------------------------
# 8. device-placed LPs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stack_of,k", [(mc.small_stack, 64), (mc.large_stack, 128)], ids=["8x10", "40x40"])
def test_device_placed_gives_the_bits_of_lds(stack_of, k):
    stack = stack_of()
    dev, lds = mc.device_run(stack, k, place="device"), mc.device_run(stack, k, place="lds")
    mc.assert_records(dev, stack, k)
    for a, b in zip(dev, lds):
        assert (a["status"], a["npiv"], a["log"], a["basis"]) == (b["status"], b["npiv"], b["log"], b["basis"])
        assert mc.same_bits(a["T"], b["T"])


def test_auto_places_a_large_lp_on_the_device():
    stack = gen.mixed_stack(100, 100, (1, 2, 3))
    eng = mc.make_engine(stack, place="auto", log_cap=256)
    try:
        assert [eng.placement(i) for i in range(3)] == ["device"] * 3
        mc.load(eng, stack)
        recs = mc.records(eng, *eng.run(MAXINC, 256))
    finally:
        eng.close()
    assert all(r["status"] == _lib.OPTIMAL for r in recs)
    mc.assert_records(recs, stack, 256)


def test_device_placed_ragged_slots_at_odd_doubles():
    # odd-sized tableaux (9 x 19, 41 x 81, 65 x 17) in front of even-sized ones: the LPs after an odd
    # running total start at an odd double
    lps = [mc.small_stack()[0], gen.tableau("mixed", 31, 32, 1), mc.large_stack()[0], gen.tableau("mixed", 3, 197, 1),
           gen.tableau("tall", 64, 16, 1), gen.tableau("mixed", 62, 1, 1), mc.small_stack()[1],
           gen.tableau("mixed", 1, 70, 1), gen.tableau("mixed", 8, 292, 1)]
    starts = np.cumsum([0] + [T.size for T in lps[:-1]])
    assert (starts % 2 == 1).sum() >= 3 and (starts % 2 == 0).sum() >= 3
    recs = mc.device_run(lps, place="device")
    mc.assert_records(recs, lps)


# ---------------------------------------------------------------------------
# 9. teams
# ---------------------------------------------------------------------------

def test_a_teamed_batch_refuses_the_rule_and_keeps_the_others():
    stack = mc.large_stack()[:3]
    eng = mc.make_engine(stack, place="device", team=2, log_cap=8)
    try:
        assert eng.team_of(0) == 2
        mc.load(eng, stack)
        with pytest.raises(ValueError, match="team"):
            eng.run(MAXINC, 5)
        assert all(mc.same_bits(a, b) for a, b in zip(eng.download(), stack))       # before any launch
        recs = mc.records(eng, *eng.run(_lib.RULE_STANDARD, 5))
    finally:
        eng.close()
    for rec, T in zip(recs, stack):
        o = F64Tableau(T)
        st, log = o.run(_lib.RULE_STANDARD, 5)
        assert (rec["status"], rec["log"]) == (st, log.tolist()) and mc.same_bits(rec["T"], o.T)


def test_team_one_and_auto_teams_of_one_run_the_rule():
    stack = mc.small_stack()
    mc.assert_records(mc.device_run(stack, place="device", team=1), stack)
    big = gen.mixed_stack(8, 10, range(1, 2049))        # more device-placed LPs than the chip has room for teams
    eng = mc.make_engine(big, place="device", team="auto", log_cap=16)
    try:
        assert {eng.team_of(i) for i in range(0, 2048, 97)} == {1} and eng.team_plan() == []
        mc.load(eng, big)
        recs = mc.records(eng, *eng.run(MAXINC, 64))
    finally:
        eng.close()
    mc.assert_records(recs, big, 64)


# ---------------------------------------------------------------------------
# 10. result="solution"
# ---------------------------------------------------------------------------

def test_solution_result_uniform():
    stack = mc.small_stack()
    full = solve_batch(stack, rule=MAXINC, steps=64, log_cap=64)
    slim = solve_batch(stack, rule=MAXINC, steps=64, log_cap=64, result="solution")
    assert slim.tableaux is None and full.status == slim.status == ["optimal"] * 64
    assert np.array_equal(full.npiv, slim.npiv) and not full.nstd.any() and not slim.nstd.any()
    assert np.array_equal(full.basis, slim.basis)
    assert mc.same_bits(full.x, slim.x) and mc.same_bits(full.objective, slim.objective)
    for i in (0, 17, 63):
        w = mc.walk(stack[i], 64)
        assert full.log(i).tolist() == slim.log(i).tolist() == w["log"]
        assert mc.same_bits(full.tableaux[i], w["T"])


def test_solution_result_ragged():
    lps = [T for T in ragged_lps() if T.shape[1] > T.shape[0]]        # the canonical ones ("tall" has no unit columns)
    full = solve_ragged(lps, rule=MAXINC, steps=128)
    slim = solve_ragged(lps, rule=MAXINC, steps=128, result="solution", place="auto")
    assert full.status == slim.status == ["optimal"] * len(lps)
    assert np.array_equal(full.npiv, slim.npiv) and mc.same_bits(full.objective, slim.objective)
    for i in range(len(lps)):
        assert full.basis[i].tolist() == slim.basis[i].tolist() and mc.same_bits(full.x[i], slim.x[i]), i
        assert full.npiv[i] == mc.walk(lps[i], 128)["npiv"], i


# ---------------------------------------------------------------------------
# 11. more LPs than resident workgroups
# ---------------------------------------------------------------------------

def test_more_lps_than_resident_workgroups():
    stack = gen.mixed_stack(8, 10, range(1, 4097))
    recs = mc.device_run(stack, 64, log_cap=16)
    for i, rec in enumerate(recs):
        w = mc.walk(stack[i], 64)
        assert (rec["status"], rec["npiv"], rec["log"]) == (w["status"], w["npiv"], w["log"][:16]), i
        assert mc.same_bits(rec["T"], w["T"]), i


# ---------------------------------------------------------------------------
# 12. the other rules on the same engine
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("place", ["lds", "device"])
def test_the_other_rules_are_untouched(place):
    stack = mc.large_stack()[:4]
    eng = mc.make_engine(stack, place=place)
    try:
        for rule in (_lib.RULE_STANDARD, MAXINC, _lib.RULE_MIN_INDEX):
            mc.load(eng, stack)
            recs = mc.records(eng, *eng.run(rule, 7))
            if rule == MAXINC:
                mc.assert_records(recs, stack, 7)
                continue
            for rec, T in zip(recs, stack):
                o = F64Tableau(T)
                st, log = o.run(rule, 7)
                assert (rec["status"], rec["npiv"], rec["log"]) == (st, len(log), log.tolist())
                assert rec["basis"] == mc.basis_after(T.shape[0] - 1, log.tolist()) and mc.same_bits(rec["T"], o.T)
    finally:
        eng.close()
