"""lp_batch_run with LP_RULE_DUAL on the GPU, where the first tests do not look
(csrc/batch.hip: bdual, bdual_start): the later trips of the lane
loops in the four-wave and the device-placed kernel, two candidates in one
lane, and tol.zero, tol.pivot and tol.cost at the start moved in both
directions.

Every comparison is status, done, the whole log, the basis and the final
tableau bit for bit against the host walk of tests/_dual_cases.py; the inputs
are built on the host, and tests/test_dual_cases_cpu.py shows on the oracle
that each does what its name says."""
import numpy as np
import pytest

import _dual_cases as dc
import _maxinc_cases as mc
from lpsol_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def waves_of(lps, place="lds"):
    """the widths of the launch bins a ragged engine of these LPs plans"""
    eng = mc.make_engine(lps, place=place)
    try:
        return {b["waves"] for b in eng.plan()}
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# A. the second and third trip of `i += NT`, NT = 256 in LDS and NT = 1024 device-placed
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,place", [(m, n, "lds") for m, n in dc.LATER_LDS] + [(m, n, "device") for m, n in dc.LATER_DEV])
def test_later_trips_of_the_lane_loops(m, n, place):
    stack = np.stack([dc.edge_lp(m, n)] * 3)
    assert stack.shape[1] * stack.shape[2] > dc.ONE_WAVE_ELEMS          # four waves in LDS
    recs = dc.device_run(stack, place=place)
    assert all((r["status"], r["log"]) == (_lib.OPTIMAL, [[m - 1, n - 1]]) for r in recs)
    dc.assert_records(recs, stack)


def test_later_trips_in_a_ragged_batch():
    lds = [dc.edge_lp(3, 767), dc.edge_lp(8, 10), dc.edge_lp(513, 6), dc.edge_lp(3, 600)]
    assert waves_of(lds) == {1, 4}
    assert waves_of([lds[0]]) == waves_of([lds[2]]) == waves_of([lds[3]]) == {4}
    recs = dc.device_run(lds, place="lds")
    for i, (rec, T) in enumerate(zip(recs, lds)):
        dc.assert_record(rec, T, tag=i)
        assert rec["log"] == [[T.shape[0] - 2, T.shape[1] - 2]]
    dev = [dc.edge_lp(3, 2049), dc.edge_lp(8, 10), dc.edge_lp(1030, 4), dc.edge_lp(3, 767)]
    recs = dc.device_run(dev, place="device")
    for i, (rec, T) in enumerate(zip(recs, dev)):
        dc.assert_record(rec, T, tag=i)
        assert rec["log"] == [[T.shape[0] - 2, T.shape[1] - 2]]


# ---------------------------------------------------------------------------
# B. two candidates in one lane: the lane keeps its first, and its minimum is over all its trips
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tol", dc.LANE_TOLS, ids=dc.LANE_TOL_IDS)
@pytest.mark.parametrize("group", list(dc.LANE_GROUPS))
def test_two_candidates_in_one_lane(group, tol):
    NT, place, _, _ = dc.LANE_GROUPS[group]
    cases = dc.lane_cases(group)
    at = 1 + dc.LANE_TOLS.index(tol)
    for kind in ("col", "row"):
        names = [k for k in cases if k.startswith(kind)]
        stack = np.stack([cases[k][0] for k in names])
        if place == "lds":
            assert waves_of(list(stack)) == ({4} if group == "nt256" else {1})
        for k in (1, dc.CAP):                   # one selection alone, and the whole walk
            recs = dc.device_run(stack, k, tol=tol, place=place)
            for name, rec in zip(names, recs):
                assert rec["log"][0] == cases[name][at], (name, k)
                dc.assert_record(rec, cases[name][0], k, tol, tag=(name, k))
    lps = [cases[k][0] for k in cases]          # RAGGED is an instantiation of its own
    recs = dc.device_run(lps, tol=tol, place=place)
    for name, rec in zip(cases, recs):
        assert rec["log"][0] == cases[name][at], name
        dc.assert_record(rec, cases[name][0], dc.CAP, tol, tag=name)


# ---------------------------------------------------------------------------
# C. tol.zero, tol.pivot and tol.cost at the start of a call, to 0 and raised
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tol", dc.FIELD_TOLS, ids=dc.FIELD_TOL_IDS)
@pytest.mark.parametrize("place", ["lds", "device"])
def test_each_tolerance_field_in_both_directions(tol, place):
    lps = dc.field_lps()
    if place == "lds":
        assert waves_of(lps) == {1, 4}
    recs = dc.device_run(lps, dc.FIELD_CAP, tol=tol, place=place)
    for i, (rec, T) in enumerate(zip(recs, lps)):
        dc.assert_record(rec, T, dc.FIELD_CAP, tol, tag=i)
    by = {name: next(r for r, T in zip(recs, lps) if T is dc.TOL_CASES[name]) for name in dc.TOL_CASES}
    stated = 0
    for name, rec in by.items():
        want = dc.tol_want(name, tol)
        if want is not None:
            assert (rec["status"], rec["log"]) == want, name
            stated += 1
    assert stated >= 2
    for name in ("cost_small", "neg_cost"):
        if by[name]["status"] == _lib.BAD_ARG:              # nothing applied
            assert by[name]["npiv"] == 0 and dc.same_bits(by[name]["T"], dc.TOL_CASES[name])
