"""lp_phased_solve (csrc/batch.hip k_twophase_dev): the two-phase solve of LPs
whose working tableau stays in device memory.  Every LP of every batch is
compared with the reporting mode of oracle/phase1.py through
_twophase_cases.check_lp: == on integers, bytes on the tableau, the objective
and the basis.

1. place="device" puts the small cases of the two-phase contract tests -- every
   outcome, the scan and set-up cases, the edge shapes -- through the new
   kernel, at the default chunk and at one pivot per launch, and each result
   equals the place="lds" run of the same batch.
2. The large cases (tests/_phased_cases.py; test_phased_cases_cpu.py) are above
   the two-phase LDS limit: place="auto" places every LP in device memory.

Every call passes a finite max_pivots (tc.oracle_batch): several of the large
LPs cycle, and an uncapped call on them never returns."""
import numpy as np
import pytest

import _phased_cases as pc
import _twophase_cases as tc
from lpsol_amd import _lib, solve_lp_batch, solve_lp_ragged
from lpsol_amd import generators as gen
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def record(eng, out, B):
    status, stage, rows, ninit, npiv, nstd = out
    return dict(status=status.tolist(), stage=stage.tolist(), rows=rows.tolist(), ninit=ninit.tolist(),
                npiv=npiv.tolist(), nstd=nstd.tolist(), T=eng.download(), z=eng.objective(),
                basis=[list(map(int, b)) for b in eng.get_basis()], log=[eng.log(i).tolist() for i in range(B)])


def run(stack, tol=None, max_pivots=-1, chunk=None, place="device", eng=None, log_cap=tc.LOG_CAP):
    """test_gpu_twophase.run() with a placement: "lds" is solve_lp, the others solve_lp_placed"""
    stack = np.ascontiguousarray(stack)
    B, m, n = stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1
    own = eng is None
    if own:
        eng = _lib.BatchEngine(B, m, n, log_cap=log_cap, place=place)
    try:
        if tol:
            eng.set_tol(**tol)
        if chunk:
            eng.set_chunk(chunk)
        eng.upload(stack)
        solve = eng.solve_lp if place == "lds" else eng.solve_lp_placed
        return record(eng, solve(max_pivots), B)
    finally:
        if own:
            eng.close()


def check_batch(res, stack, recs, where=""):
    for i, (T, o) in enumerate(zip(stack, recs)):
        tc.check_lp(res, i, T, o, finite=bool(np.isfinite(o["T"]).all()), where=where)


def device_and_lds(stack, tol=None, cap=None, where="", chunks=(None, 1)):
    """the batch under place="device" at each chunk, every LP against the
    oracle and every run equal to the place="lds" run"""
    recs, max_pivots = tc.oracle_batch(stack, tol, cap)
    lds = run(stack, tol=tol, max_pivots=max_pivots, place="lds")
    for chunk in chunks:
        res = run(stack, tol=tol, max_pivots=max_pivots, chunk=chunk)
        check_batch(res, stack, recs, f"{where} chunk {chunk}")
        tc.same_result(res, lds)
    return lds, recs


# ---------------------------------------------------------------------------
# 1. place="device" on the small cases
# ---------------------------------------------------------------------------

BATCHES = tc.outcome_batches() + tc.four_wave_batches()


@pytest.mark.parametrize("b", BATCHES, ids=[b["name"] for b in BATCHES])
def test_every_outcome_from_device_memory(b):
    res, recs = device_and_lds(b["stack"], b["tol"], b["cap"], b["name"])
    for i, want in b["want"].items():
        assert (res["status"][i], res["stage"][i]) == want, (b["name"], i)


def test_infeasible_from_device_memory():
    """(INFEASIBLE, ARTIFICIAL), which no outcome batch holds: small LPs, and sum x = 1 with sum x = 2 at the
    widest shape lp_twophase_solve takes"""
    small = np.stack([gen.phase1_lp("infeasible", 2, 4, s) for s in (1, 2, 3)])
    wide = np.stack([tc.wide_stack((1,), ())[0], tc.wide_infeasible()])
    for stack, at in ((small, (0, 1, 2)), (wide, (1,))):
        res, _ = device_and_lds(stack, where="infeasible")
        for i in at:
            assert (res["status"][i], res["stage"][i]) == (tc.INFEASIBLE, tc.ARTIFICIAL), i


@pytest.mark.parametrize("waves", [1, 4], ids=["one_wave_shape", "four_wave_shape"])
def test_scan_and_set_up_from_device_memory(waves):
    stack = tc.scan_stack(waves)
    pins = tc.scan_pins(waves)
    zero, _ = device_and_lds(stack, cap=0, where="cap 0")
    for i, name in enumerate(tc.SCAN_NAMES):
        p = pins[name]
        assert zero["basis"][i] == p["basis"], name
        assert (zero["status"][i], zero["stage"][i]) == (tc.CAP_REACHED, tc.ARTIFICIAL if p["k"] else tc.PHASE2), name
    full, _ = device_and_lds(stack, where="full")
    for i, name in enumerate(tc.SCAN_NAMES):
        p = pins[name]
        assert (full["status"][i], full["stage"][i], full["rows"][i]) == (p["status"], p["stage"], p["rows"]), name


def test_tiny_shapes_from_device_memory():
    for m, n in tc.TINY_SHAPES:
        T = tc.tiny_lp(m, n)
        stack = np.stack([T, np.concatenate([T[:1], T[:0:-1]])])
        res, _ = device_and_lds(stack, where=f"{m}x{n}")
        assert res["stage"] == [tc.PHASE2] * 2 and min(res["ninit"]) >= 1, (m, n)


def test_nonfinite_cells_from_device_memory():
    labels, stack = tc.nonfinite_stack()
    recs = [tc.report(T, None, tc.NONFINITE_CAP) for T in stack]
    lds = run(stack, max_pivots=tc.NONFINITE_CAP, place="lds")
    for chunk in (None, 1):
        res = run(stack, max_pivots=tc.NONFINITE_CAP, chunk=chunk)
        for i, (T, o) in enumerate(zip(stack, recs)):
            tc.check_lp(res, i, T, o, finite=False, where=labels[i])
        tc.same_result(res, lds)


def test_wide_shape_from_device_memory():
    stack = tc.wide_stack()
    res, _ = device_and_lds(stack, where="wide")
    m = stack.shape[1] - 1
    assert res["status"] == [tc.OPTIMAL] * 4 and res["rows"] == [m, m, m - 1, m - 1]


def test_tall_shape_from_device_memory():
    stack = tc.tall_stack()
    res, _ = device_and_lds(stack, where="tall")
    assert res["status"] == [tc.OPTIMAL] * 3 and res["rows"] == [tc.TALL_N] * 3         # 128 rows dropped


# ---------------------------------------------------------------------------
# 2. the large cases under place="auto"
# ---------------------------------------------------------------------------

def auto_engine(stack, log_cap=tc.LOG_CAP):
    B, m, n = stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1
    eng = _lib.BatchEngine(B, m, n, log_cap=log_cap, place="auto")
    assert [eng.phased_placement(i) for i in range(B)] == ["device"] * B
    return eng


def test_ge81_is_lds_for_the_plain_call_and_device_for_this_one():
    stack = pc.ge81_stack()
    recs, max_pivots = tc.oracle_batch(stack)
    eng = auto_engine(stack)
    try:
        assert [eng.placement(i) for i in range(4)] == ["lds"] * 4
        plan = eng.plan_phased()
        assert len(plan) == 1 and plan[0]["lds_bytes"] == _lib.phased_lds_bytes(*pc.GE_SHAPE) and plan[0]["lps"] == 4
        res = run(stack, max_pivots=max_pivots, place="auto", eng=eng)
    finally:
        eng.close()
    check_batch(res, stack, recs, "ge81")
    assert res["status"] == [tc.OPTIMAL] * 4 and res["rows"] == [82] * 4


@pytest.mark.parametrize("chunk", [1, 7, None], ids=["chunk_1", "chunk_7", "default_chunk"])
def test_dropped_rows_and_drive_out_at_each_chunk(chunk):
    """at chunks 1 and 7 a launch boundary falls inside the drive-out and directly before the compaction"""
    stack = pc.drop_stack()
    recs, max_pivots = tc.oracle_batch(stack)
    eng = auto_engine(stack, log_cap=2048)
    try:
        res = run(stack, max_pivots=max_pivots, chunk=chunk, place="auto", eng=eng)
    finally:
        eng.close()
    for i, (T, o) in enumerate(zip(stack, recs)):       # the log kept is longer than LOG_CAP: compare it apart
        assert res["log"][i] == o["init_seq"] + o["seq"], i
        res["log"][i] = res["log"][i][:tc.LOG_CAP]
    check_batch(res, stack, recs, f"drop chunk {chunk}")
    assert res["rows"] == [pc.DROP_ROWS] * 4
    assert [res["ninit"][i] - recs[i]["nart"] for i in range(4)] == [pc.DROP_DRIVE_OUT.get(i, 0) for i in range(4)]


LARGE = pc.large_batches()


@pytest.mark.parametrize("b", LARGE, ids=[b["name"] for b in LARGE])
def test_large_outcomes(b):
    stack = b["stack"]
    recs, max_pivots = tc.oracle_batch(stack, b["tol"], b["cap"])
    eng = auto_engine(stack)
    try:
        res = run(stack, tol=b["tol"], max_pivots=max_pivots, place="auto", eng=eng)
    finally:
        eng.close()
    check_batch(res, stack, recs, b["name"])
    for i, want in b["want"].items():
        assert (res["status"][i], res["stage"][i]) == want, (b["name"], i)


# ---------------------------------------------------------------------------
# 3. a log shorter than the pivot count
# ---------------------------------------------------------------------------

def test_log_shorter_than_phase_one():
    stack = pc.ge81_stack((1, 2))
    recs, max_pivots = tc.oracle_batch(stack)
    assert min(len(o["init_seq"]) for o in recs) > 50
    for log_cap in (0, 50):                             # smaller than phase 1's pivots
        eng = auto_engine(stack, log_cap=log_cap)
        try:
            eng.upload(stack)
            status, stage, rows, ninit, npiv, nstd = eng.solve_lp_placed(max_pivots)
            out = eng.download()
            for i, o in enumerate(recs):
                assert (status[i], stage[i], ninit[i], npiv[i]) == (tc.OPTIMAL, tc.PHASE2, len(o["init_seq"]),
                                                                    len(o["seq"]))
                assert tc.same_bits(out[i], o["T"])
                assert eng.log(i).tolist() == (o["init_seq"] + o["seq"])[:log_cap], (log_cap, i)
        finally:
            eng.close()
    res = solve_lp_batch(stack, max_pivots=max_pivots, log_cap=50, place="auto")
    for i, o in enumerate(recs):
        assert res.init_log(i).tolist() == o["init_seq"][:50] and res.log(i).tolist() == []


# ---------------------------------------------------------------------------
# 4. ragged
# ---------------------------------------------------------------------------

def ragged_record(res, B):
    return dict(status=res.status_code.tolist(), stage=res.stage.tolist(), rows=res.rows.tolist(),
                ninit=res.ninit.tolist(), npiv=res.npiv.tolist(), nstd=res.nstd.tolist(), T=res.tableaux,
                z=res.objective, basis=[list(map(int, b)) for b in res.basis],
                log=[res._engine.log(i).tolist() for i in range(B)])


def test_ragged_list_mixes_lds_and_device():
    items = pc.ragged_list()
    recs, max_pivots = tc.oracle_batch(items)
    res = solve_lp_ragged(items, max_pivots=max_pivots, log_cap=tc.LOG_CAP, place="auto")
    eng = res._engine
    where = [eng.phased_placement(i) for i in range(len(items))]
    assert tuple(i for i, w in enumerate(where) if w == "device") == pc.RAGGED_DEVICE
    assert [eng.placement(i) for i in range(len(items))].count("device") == 1      # ge(100, 100) alone
    plan = eng.plan_phased()
    assert plan[0]["lps"] == len(pc.RAGGED_DEVICE)      # the device bin, first
    assert plan[0]["lds_bytes"] == max(_lib.phased_lds_bytes(*pc.shape_of(items[i])) for i in pc.RAGGED_DEVICE)
    assert sum(b["lps"] for b in plan) == len(items)
    assert plan[0]["waves"] in (8, 16) and all(b["waves"] in (1, 4) for b in plan[1:])
    got = ragged_record(res, len(items))
    for i, (T, o) in enumerate(zip(items, recs)):
        tc.check_lp(got, i, T, o, where="ragged")
        # ... and equals what a uniform batch of its own shape gives
        alone = run(T[None], max_pivots=max_pivots, place="auto")
        for key in got:
            a, b = got[key][i], alone[key][0]
            assert tc.same_bits(np.asarray(a), np.asarray(b)) if key in ("T", "z") else a == b, (i, key)


def test_ragged_list_with_an_lp_above_the_device_bound_is_refused_by_index():
    shapes = [(8, 18), pc.GE_SHAPE, (8185, 1), (6, 12)]
    assert _lib.phased_too_large(_lib.PLACE_AUTO, 8185, 1) and not _lib.placed_too_large(_lib.PLACE_AUTO, 8185, 1)
    eng = _lib.RaggedEngine(shapes, place="auto")
    try:
        with pytest.raises(ValueError, match="LP 2 .*too large"):
            eng.solve_lp_placed(10)
        with pytest.raises(ValueError, match="LP 2 .*too large"):
            eng.plan_phased()
        with pytest.raises(ValueError):
            eng.phased_placement(2)
        assert eng.phased_placement(1) == "device" and eng.phased_placement(0) == "lds"
        # nothing was launched and the handle still serves the plain call
        lps = [gen.tableau("mixed", 8, 10, 1), gen.tableau("mixed", 82, 81, 1), np.eye(8186, 2) + 1.0,
               gen.tableau("mixed", 6, 6, 1)]
        assert [pc.shape_of(T) for T in lps] == shapes
        eng.upload(lps)
        st, npiv, _ = eng.solve(400)
        for i in (0, 1, 3):
            o = F64Tableau(lps[i])
            ost, olog, _ = o.solve(400)
            assert (st[i], npiv[i]) == (int(ost), len(olog)), i
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 5. the handle
# ---------------------------------------------------------------------------

def test_the_handle_between_calls():
    stack = pc.ge81_stack((1, 2))
    capped = tc.oracle_batch(stack, None, 40)[0]        # ends in the artificial solve
    recs, max_pivots = tc.oracle_batch(stack)
    eng = auto_engine(stack)
    try:
        first = run(stack, max_pivots=max_pivots, place="auto", eng=eng)
        check_batch(first, stack, recs, "first")
        # solve_lp keeps its own LDS test on the same handle
        eng.upload(stack)
        with pytest.raises(ValueError, match="too large"):
            eng.solve_lp(max_pivots)
        assert tc.same_bits(eng.download(), stack)
        # a second phased call gives the same bits
        tc.same_result(run(stack, max_pivots=max_pivots, place="auto", eng=eng), first)
        # an LP that ended in phase 1 downloads as uploaded
        early = run(stack, max_pivots=40, place="auto", eng=eng)
        check_batch(early, stack, capped, "cap 40")
        assert early["stage"] == [tc.ARTIFICIAL] * 2 and tc.same_bits(early["T"], stack)
        # the plain placed call on canonical LPs of the same shape
        canon = gen.mixed_stack(82, 81, (1, 2))
        assert canon.shape == stack.shape
        eng.upload(canon)
        eng.set_basis(None)
        st, npiv, nstd = eng.solve(2000)
        out = eng.download()
        for i in range(2):
            o = F64Tableau(canon[i])
            ost, olog, onstd = o.solve(2000)
            assert (st[i], npiv[i], nstd[i]) == (int(ost), len(olog), int(onstd)) and tc.same_bits(out[i], o.T), i
        # and the phased call again after it
        tc.same_result(run(stack, max_pivots=max_pivots, place="auto", eng=eng), first)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 6. the front-end
# ---------------------------------------------------------------------------

def test_solve_lp_batch_place():
    stack = pc.ge81_stack((1, 2))
    recs, max_pivots = tc.oracle_batch(stack)
    with pytest.raises(ValueError, match="too large"):
        solve_lp_batch(stack, max_pivots=max_pivots)
    with pytest.raises(ValueError, match="too large"):
        solve_lp_batch(stack, max_pivots=max_pivots, place="lds")
    res = solve_lp_batch(stack, max_pivots=max_pivots, log_cap=tc.LOG_CAP, place="auto")
    got = dict(status=res.status_code.tolist(), stage=res.stage.tolist(), rows=res.rows.tolist(),
               ninit=res.ninit.tolist(), npiv=res.npiv.tolist(), nstd=res.nstd.tolist(), T=res.tableaux,
               z=res.objective, basis=res.basis.tolist(), log=[res._engine.log(i).tolist() for i in range(2)])
    check_batch(got, stack, recs, "front-end")
    assert res.status == ["optimal", "optimal"]
    for i, o in enumerate(recs):
        assert res.init_log(i).tolist() == o["init_seq"] and res.log(i).tolist() == o["seq"]
        assert tc.same_bits(res.tableau(i).toArray(), o["T"])
