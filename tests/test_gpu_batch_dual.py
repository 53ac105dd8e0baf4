"""lp_batch_run with LP_RULE_DUAL on the GPU (csrc/batch.hip: bdual in front of
bstep's pivot).

Every comparison is status, done, the whole log, the basis and the final
tableau bit for bit (a NaN matching a NaN) against the host walk of
tests/_dual_cases.py.  The inputs are warm tableaux the host built from oracle
optima -- nothing from the device -- and the constructed tableaux;
tests/test_dual_cases_cpu.py shows that each does on the oracle what its name
claims."""
import numpy as np
import pytest

import _dual_cases as dc
import _maxinc_cases as mc
from lpsol_amd import _lib
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu

DUAL = _lib.RULE_DUAL


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def small(how="scale"):
    return dc.warm_stack(dc.SMALL, dc.SMALL_SEEDS, how)             # 9 x 19, 64 LPs


def large(how="scale"):
    return dc.warm_stack(dc.LARGE, dc.LARGE_GPU_SEEDS, how)         # 41 x 81, 16 LPs


# ---------------------------------------------------------------------------
# 1, 2. one wave and four waves, the tableau in LDS
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["scale", "shift"])
def test_one_wave_in_lds(how):
    stack = small(how)
    recs = dc.device_run(stack)
    dc.assert_records(recs, stack)
    fates = {r["status"] for r in recs}
    assert fates == ({_lib.OPTIMAL} if how == "scale" else {_lib.OPTIMAL, _lib.INFEASIBLE})
    assert sum(r["npiv"] > 0 for r in recs) >= 16


@pytest.mark.parametrize("how", ["scale", "shift"])
def test_four_waves_in_lds(how):
    stack = large(how)
    assert stack.shape[1] * stack.shape[2] > 2048       # above the one-wave bound
    recs = dc.device_run(stack)
    dc.assert_records(recs, stack)
    assert sum(r["npiv"] >= 3 for r in recs) >= 4


# ---------------------------------------------------------------------------
# 3. device-placed: odd element counts, so every second LP starts at an odd double and the pair walk peels a head
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stack_of", [small, large], ids=["9x19", "41x81"])
def test_device_placed_gives_the_bits_of_lds(stack_of):
    stack = np.concatenate([stack_of("scale")[:8], stack_of("shift")[:8]])
    assert stack[0].size % 2 == 1
    dev, lds = dc.device_run(stack, place="device"), dc.device_run(stack, place="lds")
    dc.assert_records(dev, stack)
    for a, b in zip(dev, lds):
        assert (a["status"], a["npiv"], a["log"], a["basis"]) == (b["status"], b["npiv"], b["log"], b["basis"])
        assert dc.same_bits(a["T"], b["T"])


def test_device_placed_even_element_count():
    stack = dc.warm_stack((7, 10), range(1, 9), "shift")        # 8 x 18
    assert stack[0].size % 2 == 0
    dc.assert_records(dc.device_run(stack, place="device"), stack)


# ---------------------------------------------------------------------------
# 4. a ragged batch of all of these and the constructed cases, under each tolerance set
# ---------------------------------------------------------------------------

def ragged_lps():
    names = list(dc.CASES)
    lps = [dc.CASES[k] for k in names]
    lps[3:3] = list(small("shift")[:3])
    lps[9:9] = list(large("scale")[:2])
    lps += [dc.edge_lp(65, 4), dc.edge_lp(3, 256)] + list(small("scale")[8:11]) + [large("shift")[2]]
    return lps


@pytest.mark.parametrize("tol", dc.TOLS, ids=dc.TOL_IDS)
@pytest.mark.parametrize("place", ["lds", "device"])
def test_ragged_mix_with_the_constructed_cases(tol, place):
    lps = ragged_lps()
    starts = np.cumsum([0] + [T.size for T in lps[:-1]])
    assert (starts % 2 == 1).any() and (starts % 2 == 0).any()
    recs = dc.device_run(lps, tol=tol, place=place)
    for i, (rec, T) in enumerate(zip(recs, lps)):
        dc.assert_record(rec, T, dc.CAP, tol, tag=i)
    by = {name: next(r for r, T in zip(recs, lps) if T is dc.CASES[name]) for name in dc.CASES}
    assert by["row_tie"]["log"][0] == [0, 0]
    assert by["row_band"]["log"][0] == ([1, 0] if tol == dict(cost_tie=0.0) else [0, 0])
    assert by["col_tie"]["log"][0] == [0, 0]
    assert by["col_band_in"]["log"][0] == ([0, 1] if tol == dict(ratio_tie=0.0) else [0, 0])
    assert by["col_band_out"]["log"][0] == by["a_small"]["log"][0] == [0, 1]
    assert by["cost_clamp"]["log"][0] == ([0, 1] if tol == dict(cost=0.0) else [0, 0])
    assert (by["b_small"]["status"], by["b_small"]["npiv"]) == (_lib.OPTIMAL, 0)
    assert (by["infeasible"]["status"], by["infeasible"]["log"]) == (_lib.INFEASIBLE, [[1, 0]])
    assert (by["infeasible_now"]["status"], by["infeasible_now"]["npiv"]) == (_lib.INFEASIBLE, 0)
    assert (by["neg_cost"]["status"], by["neg_cost"]["npiv"]) == (_lib.BAD_ARG, 0)
    assert dc.same_bits(by["neg_cost"]["T"], dc.NEG_COST)            # the tableau untouched
    assert by["nan_ratio"]["status"] == by["neg_inf_b"]["status"] == _lib.BAD_PIVOT
    assert dc.same_bits(by["nan_ratio"]["T"], dc.NAN_RATIO) and dc.same_bits(by["neg_inf_b"]["T"], dc.NEG_INF_B)
    assert np.isnan(by["nan_cell"]["T"][:, 1]).all()


def test_ragged_plan_has_both_widths():
    lps = ragged_lps()
    eng = mc.make_engine(lps)
    try:
        assert {1, 4} <= {b["waves"] for b in eng.plan()}
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 5. caps, chunks and a second run
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stack_of,place", [(small, "lds"), (large, "lds"), (large, "device")],
                         ids=["9x19", "41x81", "41x81-device"])
def test_caps_and_chunks(stack_of, place):
    stack = np.concatenate([stack_of("scale")[:6], stack_of("shift")[:6], [stack_of("scale")[0]]])
    stack[-1, 0, 3] = -1.0                              # not dual feasible: LP_BAD_ARG whatever k is
    for recs in (dc.device_run(stack, 0, place=place), dc.device_run(stack, 0, chunk=1, place=place)):
        assert [r["status"] for r in recs] == [_lib.PIVOTED] * 12 + [_lib.BAD_ARG]
        assert all(r["npiv"] == 0 and r["log"] == [] for r in recs)
        dc.assert_records(recs, stack, 0)
    one = dc.device_run(stack, 1, chunk=1, place=place)
    dc.assert_records(one, stack, 1)
    assert {r["status"] for r in one} >= {_lib.PIVOTED, _lib.OPTIMAL, _lib.BAD_ARG}
    whole = dc.device_run(stack, place=place)
    dc.assert_records(whole, stack)
    for chunk in (1, 2):
        got = dc.device_run(stack, chunk=chunk, place=place)
        for a, b in zip(got, whole):
            assert (a["status"], a["npiv"], a["log"], a["basis"]) == (b["status"], b["npiv"], b["log"], b["basis"])
            assert dc.same_bits(a["T"], b["T"])


def test_a_second_run_continues_from_the_current_tableau():
    stack = large("scale")
    eng = mc.make_engine(stack, log_cap=dc.LOG_CAP)
    try:
        mc.load(eng, stack)
        first = mc.records(eng, *eng.run(DUAL, 2))
        dc.assert_records(first, stack, 2)
        second = mc.records(eng, *eng.run(DUAL, dc.CAP))
    finally:
        eng.close()
    assert sum(r["status"] == _lib.PIVOTED for r in first) >= 4
    for i, (a, b) in enumerate(zip(first, second)):
        w = dc.walk(a["T"])                 # the walk, started where the first run stopped
        assert (b["status"], b["npiv"], b["log"]) == (w["status"], w["npiv"], w["log"]), i
        assert dc.same_bits(b["T"], w["T"]), i
        whole = dc.walk(stack[i])
        assert a["log"] + b["log"] == whole["log"] and dc.same_bits(b["T"], whole["T"]), i


# ---------------------------------------------------------------------------
# 6. the edges of the lane mapping: the only negative b in the last row, the only eligible column last
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", dc.EDGE_ROWS + dc.EDGE_COLS)
@pytest.mark.parametrize("place", ["lds", "device"])
def test_lane_mapping_edges(m, n, place):
    stack = np.stack([dc.edge_lp(m, n)] * 3)
    recs = dc.device_run(stack, place=place)
    assert all((r["status"], r["log"]) == (_lib.OPTIMAL, [[m - 1, n - 1]]) for r in recs)
    dc.assert_records(recs, stack)


# ---------------------------------------------------------------------------
# 7. teams
# ---------------------------------------------------------------------------

def test_a_teamed_batch_refuses_the_rule_and_keeps_the_others():
    stack = mc.large_stack()[:3]
    eng = mc.make_engine(stack, place="device", team=2, log_cap=8)
    try:
        assert eng.team_of(0) == 2
        mc.load(eng, stack)
        with pytest.raises(ValueError, match="team"):
            eng.run(DUAL, 5)
        assert all(dc.same_bits(a, b) for a, b in zip(eng.download(), stack))       # before any launch
        for rule in (_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX):
            mc.load(eng, stack)
            recs = mc.records(eng, *eng.run(rule, 5))
            for rec, T in zip(recs, stack):
                o = F64Tableau(T)
                st, log = o.run(rule, 5)
                assert (rec["status"], rec["log"]) == (st, log.tolist()) and dc.same_bits(rec["T"], o.T)
    finally:
        eng.close()


def test_team_one_runs_the_rule():
    stack = small("shift")[:16]
    dc.assert_records(dc.device_run(stack, place="device", team=1), stack)


# ---------------------------------------------------------------------------
# 8. the other rules on the same engine
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("place", ["lds", "device"])
def test_the_other_rules_are_untouched(place):
    stack = mc.large_stack()[:4]
    eng = mc.make_engine(stack, place=place)
    try:
        for rule in (_lib.RULE_STANDARD, DUAL, _lib.RULE_MAX_INCREASE, _lib.RULE_MIN_INDEX):
            mc.load(eng, stack)
            recs = mc.records(eng, *eng.run(rule, 7))
            if rule == DUAL:                    # the generator's LPs start with negative costs
                assert all((r["status"], r["npiv"]) == (_lib.BAD_ARG, 0) for r in recs)
                assert all(dc.same_bits(r["T"], T) for r, T in zip(recs, stack))
                continue
            if rule == _lib.RULE_MAX_INCREASE:
                mc.assert_records(recs, stack, 7)
                continue
            for rec, T in zip(recs, stack):
                o = F64Tableau(T)
                st, log = o.run(rule, 7)
                assert (rec["status"], rec["npiv"], rec["log"]) == (st, len(log), log.tolist())
                assert rec["basis"] == mc.basis_after(T.shape[0] - 1, log.tolist()) and dc.same_bits(rec["T"], o.T)
    finally:
        eng.close()
