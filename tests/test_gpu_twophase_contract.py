"""lp_twophase_solve (csrc/batch.hip k_twophase) where test_gpu_twophase.py does
not go: every (status, stage) the call can report, the basic-column scan and
the set-up of the artificial problem on hand-built inputs, the shapes at the
wave threshold and at the LDS limit, more LPs than compute units, logs shorter
than the pivot count, non-finite cells, and the handle after a call that ended
early.

Every LP of every batch is compared with the reporting mode of
oracle/phase1.py (solve_lp(..., report=True)): == on integers, bytes on the
tableau, the objective and the basis; where the oracle's own tableau holds a
non-finite cell, NaN in the same cells and bytes elsewhere.  The inputs, and
the CPU test that they reach what they are there for, are in
tests/_twophase_cases.py and tests/test_twophase_cases_cpu.py.

Every call passes a finite max_pivots: the case's own cap where the cap is the
point, else the largest per-solve pivot count the oracle needed over the batch
plus 8 (tc.oracle_batch).  A kernel that matches the oracle never reaches the
second; one that does not ends with LP_CAP_REACHED and a failing assertion.

Non-finite cells (group f): the reporting oracle raises on none of the twelve
inputs, so none is left out."""
import ctypes as C

import numpy as np
import pytest

import _twophase_cases as tc
from test_gpu_twophase import run
from lpsol_amd import _lib
from lpsol_amd import generators as gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def check_batch(res, stack, recs, where=""):
    for i, (T, o) in enumerate(zip(stack, recs)):
        tc.check_lp(res, i, T, o, finite=bool(np.isfinite(o["T"]).all()), where=where)


def solve_and_check(stack, tol=None, cap=None, where="", **kw):
    """one device call under the case's cap or the safety cap, every LP checked"""
    recs, max_pivots = tc.oracle_batch(stack, tol, cap)
    res = run(stack, tol=tol, max_pivots=max_pivots, **kw)
    check_batch(res, stack, recs, where)
    return res, recs, max_pivots


# ---------------------------------------------------------------------------
# a. outcomes
# ---------------------------------------------------------------------------

BATCHES = tc.outcome_batches() + tc.four_wave_batches()


@pytest.mark.parametrize("b", BATCHES, ids=[b["name"] for b in BATCHES])
def test_every_outcome_between_its_neighbours(b):
    stack = b["stack"]
    res, recs, max_pivots = solve_and_check(stack, b["tol"], b["cap"], b["name"])
    for i, want in b["want"].items():
        assert (res["status"][i], res["stage"][i]) == want, (b["name"], i)
    for i in b["canon"]:                        # phase 2 ran where the reference would assert
        assert recs[i]["canonical"] is False and res["stage"][i] == tc.PHASE2, (b["name"], i)
    # a relaunch at every pivot: the state goes through global memory each time
    one = run(stack, tol=b["tol"], max_pivots=max_pivots, chunk=1)
    tc.same_result(one, res)


# ---------------------------------------------------------------------------
# b. the scan and the set-up
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True], ids=["rows_in_order", "rows_reversed"])
@pytest.mark.parametrize("waves", [1, 4], ids=["one_wave", "four_waves"])
def test_scan_and_set_up(waves, reverse):
    stack = tc.scan_stack(waves, reverse)
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    assert _lib.twophase_waves(m, n) == waves
    pins = tc.scan_pins(waves)
    # max_pivots = 0 stops every LP before its first pivot: the basis is the
    # set-up's, the tableau the flipped one where no artificial is needed
    zero, recs, _ = solve_and_check(stack, cap=0, where="cap 0")
    for i, name in enumerate(tc.SCAN_NAMES):
        p = pins[name]
        want, k = tc.scan_basis(stack[i])
        assert k == p["k"] and (reverse or want == p["basis"]), name
        assert zero["basis"][i] == want, name
        assert zero["status"][i] == tc.CAP_REACHED, name
        assert zero["stage"][i] == (tc.ARTIFICIAL if k else tc.PHASE2), name
        assert (zero["ninit"][i], zero["npiv"][i]) == (0, 0), name
    full, recs, _ = solve_and_check(stack, where="full")
    for i, name in enumerate(tc.SCAN_NAMES):
        p = pins[name]
        assert (full["status"][i], full["stage"][i], full["rows"][i]) == \
            (p["status"], p["stage"], p["rows"]), name
        assert (full["ninit"][i] > 0) == (p["k"] > 0), name
    tc.same_result(run(stack, max_pivots=0, chunk=1), zero)


# ---------------------------------------------------------------------------
# c. shapes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ns,waves", [(32, 1), (33, 4)], ids=["last_one_wave", "first_four_waves"])
def test_wave_boundary(ns, waves):
    stack = np.stack([gen.phase1_lp("eq", 30, ns, s) for s in range(1, 5)])
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    assert (m, n) == (31, ns) and (m + 1) * (n + 1 + m) == (2048 if waves == 1 else 2080)
    assert _lib.twophase_waves(m, n) == waves
    res, recs, _ = solve_and_check(stack)
    assert all(o["stage"] == tc.PHASE2 and o["init_seq"] for o in recs)


def test_largest_wide_shape():
    stack = tc.wide_stack()
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    assert n == tc.WIDE_N and m == _lib.twophase_max_m(n)
    assert _lib.twophase_lds_bytes(m, n) <= _lib.BATCH_LDS_MAX < _lib.twophase_lds_bytes(m + 1, n)
    res, recs, _ = solve_and_check(stack, where="wide")
    assert res["status"] == [tc.OPTIMAL] * 4 and res["rows"] == [m, m, m - 1, m - 1]


def test_largest_tall_shape():
    stack = tc.tall_stack()
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    assert n == tc.TALL_N and m == _lib.twophase_max_m(n)
    assert _lib.twophase_lds_bytes(m, n) <= _lib.BATCH_LDS_MAX < _lib.twophase_lds_bytes(m + 1, n)
    res, recs, max_pivots = solve_and_check(stack, where="tall")
    assert res["status"] == [tc.OPTIMAL] * 3 and res["rows"] == [n] * 3     # m - n rows dropped
    tc.same_result(run(stack, max_pivots=max_pivots, chunk=7), res)


def test_tiny_shapes():
    for m, n in tc.TINY_SHAPES:
        T = tc.tiny_lp(m, n)
        stack = np.stack([T, np.concatenate([T[:1], T[:0:-1]])])
        res, recs, _ = solve_and_check(stack, where=f"{m}x{n}")
        assert res["stage"] == [tc.PHASE2] * 2 and min(res["ninit"]) >= 1, (m, n)


# ---------------------------------------------------------------------------
# d. more LPs than compute units
# ---------------------------------------------------------------------------

def test_more_wide_lps_than_compute_units():
    """one workgroup of the widest shape fits a compute unit, so 300 of them
    do not run at once"""
    stack = tc.many_wide()
    assert len(stack) == 300 > 256
    res, recs, _ = solve_and_check(stack, where="300 wide")
    i, c = tc.WIDE_INFEASIBLE_AT, tc.WIDE_CANONICAL_AT
    assert (res["status"][i], res["stage"][i]) == (tc.INFEASIBLE, tc.ARTIFICIAL)
    assert (res["status"][c], res["ninit"][c]) == (tc.OPTIMAL, 0) and res["npiv"][c] > 0


def test_2048_small_lps():
    stack = tc.many_small()
    assert len(stack) == 2048
    res, recs, _ = solve_and_check(stack, where="2048 small")
    assert set(res["status"]) == {tc.OPTIMAL}


# ---------------------------------------------------------------------------
# e. the log
# ---------------------------------------------------------------------------

def test_log_shorter_than_the_pivot_count():
    stack = np.stack([gen.phase1_lp("ge", 5, 6, s) for s in range(1, 9)])
    want, recs, max_pivots = solve_and_check(stack)
    ninit, npiv = want["ninit"][0], want["npiv"][0]
    assert (ninit, npiv) == (3, 8)                      # phase-1 and phase-2 pivots
    B, m, n = len(stack), stack.shape[1] - 1, stack.shape[2] - 1
    for log_cap in (0, 1, ninit - 1, ninit, ninit + 1, ninit + npiv - 1):
        eng = _lib.BatchEngine(B, m, n, log_cap=log_cap)
        try:
            eng.upload(stack)
            status, stage, rows, ni, npv, nstd = eng.solve_lp(max_pivots)
            got = dict(status=status.tolist(), stage=stage.tolist(), rows=rows.tolist(),
                       ninit=ni.tolist(), npiv=npv.tolist(), nstd=nstd.tolist(), T=eng.download(),
                       z=eng.objective(), basis=eng.get_basis().tolist(), log=want["log"])
            tc.same_result(got, want)                   # everything but the log
            for i in range(B):
                full = want["log"][i]
                assert eng.log(i).tolist() == full[:log_cap], (log_cap, i)
                # the raw call, into a poisoned buffer longer than the log kept
                buf = np.full((log_cap + 4, 2), -7, dtype=np.int64)
                cnt = C.c_int64()
                eng._check(eng.lib.lp_batch_log(eng.h, i, buf.ctypes.data_as(_lib._P64),
                                                log_cap + 4, C.byref(cnt)), eng.h)
                assert cnt.value == want["ninit"][i] + want["npiv"][i] == len(full), (log_cap, i)
                take = min(log_cap, len(full))
                assert buf[:take].tolist() == full[:take] and (buf[take:] == -7).all(), (log_cap, i)
        finally:
            eng.close()


# ---------------------------------------------------------------------------
# f. non-finite cells
# ---------------------------------------------------------------------------

def test_nonfinite_cells():
    labels, stack = tc.nonfinite_stack()
    recs = [tc.report(T, None, tc.NONFINITE_CAP) for T in stack]
    for chunk in (None, 1):
        res = run(stack, max_pivots=tc.NONFINITE_CAP, chunk=chunk)
        for i, (T, o) in enumerate(zip(stack, recs)):
            tc.check_lp(res, i, T, o, finite=False, where=labels[i])


# ---------------------------------------------------------------------------
# g. the handle afterwards
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,early", [("cap_in_either_solve", (tc.CAP_REACHED, tc.ARTIFICIAL)),
                                        ("phase1_failed_zero", (tc.PHASE1_FAILED, tc.DRIVE_OUT))])
def test_a_second_call_after_lps_that_ended_early(name, early):
    b = next(x for x in BATCHES if x["name"] == name)
    stack, tol = b["stack"], b["tol"]
    B, m, n = len(stack), stack.shape[1] - 1, stack.shape[2] - 1
    recs, safety = tc.oracle_batch(stack, tol)          # no cap of the case's own
    first_cap = b["cap"] if b["cap"] is not None else safety
    eng = _lib.BatchEngine(B, m, n, log_cap=tc.LOG_CAP)
    try:
        first = run(stack, tol=tol, max_pivots=first_cap, eng=eng)
        assert early in set(zip(first["status"], first["stage"]))
        second = run(stack, tol=tol, max_pivots=safety, eng=eng)
    finally:
        eng.close()
    tc.same_result(second, run(stack, tol=tol, max_pivots=safety))
    check_batch(second, stack, recs, name)
