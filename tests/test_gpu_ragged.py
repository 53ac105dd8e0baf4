"""Ragged batches on the GPU (lp_ragged_*, lpsol_amd.solve_ragged /
solve_lp_ragged; csrc/batch.hip k_batch<.., true>, k_twophase<.., true>): LPs of
different shapes in one call, each against what the oracle gives for ITS shape.

Every comparison is exact: status, pivot counts, the log and the basis are
equal to the oracle's (oracle/lp_f64.c through oracle.f64.F64Tableau,
oracle/phase1.py) or the golden fixture's, and the tableaux are bit-identical.
Every device call carries a finite pivot cap."""
import ctypes

import numpy as np
import pytest

from conftest import fixture_input, load_golden

import _ragged_cases as rc
import _twophase_cases as tc
from lpsol_amd import _lib, solve_batch, solve_lp_batch, solve_lp_ragged, solve_ragged
from lpsol_amd import generators as gen
from lpsol_amd.batch import ragged_canonical_basis
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu

SMALL = load_golden("small.json")
CAP = 4096      # pivot cap given to both sides where the test is not about caps
LOG_CAP = tc.LOG_CAP


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bits(a) == bits(b)


# ------------------------------------------------------------------ oracle
_ORACLE = {}


def oracle_solve(T, cap=CAP):
    """(status, log, nstd, final tableau) of lpf_solve, computed once per input"""
    key = (T.shape, T.tobytes(), cap)
    if key not in _ORACLE:
        o = F64Tableau(T)
        st, log, nstd = o.solve(cap=cap, logcap=max(cap, 1))
        _ORACLE[key] = (st, log, nstd, o.T)
    return _ORACLE[key]


# ------------------------------------------------------------------ device
def shapes_of(lps):
    return [rc.shape_of(T) for T in lps]


def engine_solve(lps, *, cap=CAP, chunk=None, log_cap=LOG_CAP, basis=None, eng=None):
    """one lp_batch_solve of a ragged batch through the thin engine (its own,
    or eng) -> dict of per-LP results"""
    own = eng is None
    if own:
        eng = _lib.RaggedEngine(shapes_of(lps), log_cap=log_cap)
    try:
        if chunk is not None:
            eng.set_chunk(chunk)
        eng.upload(lps)
        if basis is not None:
            eng.set_basis(basis)
        st, npiv, nstd = eng.solve(cap)
        return dict(status=st.tolist(), npiv=npiv.tolist(), nstd=nstd.tolist(), T=eng.download(),
                    z=eng.objective(), log=[eng.log(i).tolist() for i in range(len(lps))],
                    basis=[b.tolist() for b in eng.get_basis()] if basis is not None else None)
    finally:
        if own:
            eng.close()


def assert_lp_matches_oracle(res, i, T, *, cap=CAP, basis0=None, where=""):
    w = f"{where} LP {i}"
    st, log, nstd, want = oracle_solve(T, cap)
    assert res["status"][i] == st, w
    assert res["npiv"][i] == len(log) and res["nstd"][i] == nstd, w
    assert res["log"][i] == log.tolist()[:LOG_CAP], w
    assert same_bits(res["T"][i], want), w
    assert bits(res["z"][i:i + 1]) == bits(np.array([-want[0, 0]])), w
    if basis0 is not None:
        b = list(basis0[i])
        for r, c in log:
            b[r] = c
        assert res["basis"][i] == b, w


def same_lp(a, i, b, j, where=""):
    """LP i of device record a equals LP j of record b in every field"""
    for key in ("status", "npiv", "nstd", "log", "basis"):
        if a[key] is not None:
            assert a[key][i] == b[key][j], (where, key, i, j)
    assert same_bits(a["T"][i], b["T"][j]), (where, i, j)
    assert bits(a["z"][i:i + 1]) == bits(b["z"][j:j + 1]), (where, i, j)


# ---------------------------------------------------------------------------
# 1. every golden solve in one call
# ---------------------------------------------------------------------------

GOLDEN = [fixture_input(fx) for fx in SMALL["solve"]]
GOLDEN_LOG = max(len(fx["seq"]) for fx in SMALL["solve"]) + 1


@pytest.fixture(scope="module")
def golden_result():
    return solve_ragged(GOLDEN, max_pivots=CAP, log_cap=GOLDEN_LOG)


def test_golden_solves_in_one_call(golden_result):
    res = golden_result
    assert len(GOLDEN) == 39 and len(res) == 39
    assert len({T.shape for T in GOLDEN}) > 9
    for i, fx in enumerate(SMALL["solve"]):
        st, log, nstd, T = oracle_solve(GOLDEN[i])
        assert res.status[i] == "optimal" and st == _lib.OPTIMAL, fx["name"]
        assert res.log(i).tolist() == fx["seq"], fx["name"]
        assert res.npiv[i] == len(fx["seq"]) and res.nstd[i] == fx["nstd"], fx["name"]
        assert res.basis[i].tolist() == fx["bfs"], fx["name"]
        assert same_bits(res.tableaux[i], T), fx["name"]
        assert res.objective[i] == -T[0, 0], fx["name"]
        assert res.tableau(i).getZ() == -T[0, 0]
    plan = res.plan()
    assert len(plan) > 1 and {b["waves"] for b in plan} == {1, 4}      # the binning took effect
    assert sum(b["lps"] for b in plan) == 39
    assert [b["lds_bytes"] for b in plan] == sorted((b["lds_bytes"] for b in plan), reverse=True)
    assert plan[0]["lds_bytes"] == max(_lib.batch_lds_bytes(*rc.shape_of(T)) for T in GOLDEN)
    assert plan[-1]["lds_bytes"] < plan[0]["lds_bytes"] // 8            # small LPs get small allocations
    for b in plan:
        assert 1 <= b["lps_per_cu"] <= _lib.BATCH_LDS_MAX // b["lds_bytes"]


# ---------------------------------------------------------------------------
# 2. the uniform path on each shape group gives the same, LP by LP
# ---------------------------------------------------------------------------

def test_equal_to_the_uniform_path_per_shape_group(golden_result):
    res = golden_result
    groups = {}
    for i, T in enumerate(GOLDEN):
        groups.setdefault(T.shape, []).append(i)
    assert len(groups) > 9
    for idx in groups.values():
        uni = solve_batch(np.stack([GOLDEN[i] for i in idx]), max_pivots=CAP, log_cap=GOLDEN_LOG)
        for k, i in enumerate(idx):
            assert uni.status_code[k] == res.status_code[i], i
            assert (uni.npiv[k], uni.nstd[k]) == (res.npiv[i], res.nstd[i]), i
            assert uni.log(k).tolist() == res.log(i).tolist(), i
            assert uni.basis[k].tolist() == res.basis[i].tolist(), i
            assert same_bits(uni.tableaux[k], res.tableaux[i]), i
            assert bits(uni.objective[k:k + 1]) == bits(res.objective[i:i + 1]), i


# ---------------------------------------------------------------------------
# 3. order independence, resume, caps
# ---------------------------------------------------------------------------

def test_order_independence(golden_result):
    n = len(GOLDEN)
    one = [i for i in range(n) if GOLDEN[i].size <= 2048]
    four = [i for i in range(n) if GOLDEN[i].size > 2048]
    assert one and four
    inter = []                                  # one-wave and four-wave LPs alternating
    for k in range(max(len(one), len(four))):
        inter += one[k:k + 1] + four[k:k + 1]
    for name, perm in (("reversed", list(range(n))[::-1]), ("interleaved", inter)):
        assert sorted(perm) == list(range(n))
        res = solve_ragged([GOLDEN[i] for i in perm], max_pivots=CAP, log_cap=GOLDEN_LOG)
        for k, i in enumerate(perm):
            assert res.status_code[k] == golden_result.status_code[i], (name, i)
            assert (res.npiv[k], res.nstd[k]) == (golden_result.npiv[i], golden_result.nstd[i]), (name, i)
            assert res.log(k).tolist() == golden_result.log(i).tolist(), (name, i)
            assert res.basis[k].tolist() == golden_result.basis[i].tolist(), (name, i)
            assert same_bits(res.tableaux[k], golden_result.tableaux[i]), (name, i)


def resume_list():
    """km_deg_d8 and km_std_d8 between neighbours of other shapes, one of them
    larger in m + n than both and four-wave"""
    fx = {f["name"]: fixture_input(f) for f in SMALL["solve"] if f["name"] in ("km_deg_d8", "km_std_d8")}
    return [gen.tableau("mixed", 40, 40, 1), fx["km_deg_d8"], gen.tableau("mixed", 3, 3, 2), fx["km_std_d8"],
            gen.tableau("mixed", 16, 16, 11), gen.tableau("mixed", 1, 1, 1)]


def test_chunked_launches_give_identical_results():
    lps = resume_list()
    basis0 = ragged_canonical_basis(lps)
    results = [engine_solve(lps, chunk=c, basis=basis0) for c in (1, 5, None)]
    for i, T in enumerate(lps):
        assert_lp_matches_oracle(results[2], i, T, basis0=basis0)
    assert results[2]["npiv"][3] == 2 ** 8 - 1
    # the stall switch fired in km_deg_d8, at its own m + n = 24: under the
    # m + n = 120 of its four-wave neighbour it would fire later or not at all
    assert results[2]["nstd"][1] < results[2]["npiv"][1]
    assert results[2]["nstd"][1] == next(f for f in SMALL["solve"] if f["name"] == "km_deg_d8")["nstd"]
    for r in results[:2]:
        for i in range(len(lps)):
            same_lp(r, i, results[2], i)


def test_cap_below_one_lps_pivot_count():
    lps = resume_list()
    counts = [len(oracle_solve(T)[1]) for T in lps]
    cap = 20
    assert counts[3] == 255 and counts[1] > cap and counts[0] > cap         # these three are cut short
    assert all(c < cap for c in (counts[2], counts[4], counts[5]))
    res = engine_solve(lps, cap=cap, basis=ragged_canonical_basis(lps))
    for i, T in enumerate(lps):
        assert_lp_matches_oracle(res, i, T, cap=cap, basis0=ragged_canonical_basis(lps))
        full = oracle_solve(T)
        if counts[i] > cap:
            assert res["status"][i] == _lib.CAP_REACHED
            assert res["log"][i] == full[1].tolist()[:cap]                  # the oracle's prefix
        else:
            assert res["status"][i] == _lib.OPTIMAL and res["log"][i] == full[1].tolist()
            assert same_bits(res["T"][i], full[3])


# ---------------------------------------------------------------------------
# 4. shapes at the edges of the mapping, next to each other
# ---------------------------------------------------------------------------

MAX_M_128 = _lib.batch_max_m(128)

EDGE_LISTS = {
    # 1x1 next to the largest m lp_batch_create takes at n = 128
    "smallest_largest": ([("tall", 1, 1), ("tall", MAX_M_128, 128), ("tall", 1, 1)], 24),
    # 32 x 64 = 2048 elements, the last one-wave shape, next to the first four-wave one
    "wave_threshold": ([("mixed", 31, 32), ("mixed", 31, 33), ("mixed", 31, 32)], CAP),
    # 65 rows on a one-wave block next to 17 x 129 on a four-wave one
    "tall_wide": ([("tall", 64, 16), ("mixed", 16, 112), ("tall", 64, 16)], 40),
}


@pytest.mark.parametrize("name", list(EDGE_LISTS))
def test_edge_shapes_next_to_each_other(name):
    specs, cap = EDGE_LISTS[name]
    lps = [gen.tableau(kind, m, ns, 1 + k) for k, (kind, m, ns) in enumerate(specs)]
    if name == "wave_threshold":
        assert [rc.shape_of(T) for T in lps] == [(31, 63), (31, 64), (31, 63)]
    basis0 = [np.full(T.shape[0] - 1, -1, dtype=np.int32) for T in lps]
    eng = _lib.RaggedEngine(shapes_of(lps), log_cap=LOG_CAP)
    plan = eng.plan()
    assert [b["waves"] for b in plan] == [4, 1] and [b["lps"] for b in plan] == [1, 2]
    assert plan[0]["lds_bytes"] == _lib.batch_lds_bytes(*rc.shape_of(lps[1]))
    assert plan[1]["lds_bytes"] == _lib.batch_lds_bytes(*rc.shape_of(lps[0]))
    res = engine_solve(lps, cap=cap, basis=basis0, eng=eng)
    eng.close()
    assert max(res["npiv"]) <= LOG_CAP and min(res["npiv"]) >= 1
    for i, T in enumerate(lps):
        assert_lp_matches_oracle(res, i, T, cap=cap, basis0=basis0, where=name)


# ---------------------------------------------------------------------------
# 5. packed windows
# ---------------------------------------------------------------------------

def window_list():
    return [gen.tableau("mixed", 8, 10, 1), gen.tableau("mixed", 16, 16, 11), gen.tableau("mixed", 3, 3, 2),
            gen.tableau("mixed", 40, 40, 1), gen.tableau("mixed", 1, 1, 1), gen.tableau("mixed", 24, 32, 11)]


def test_packed_upload_download_windows():
    first = window_list()
    fresh = [gen.tableau("mixed", 3, 3, 7), gen.tableau("mixed", 40, 40, 2)]       # the shapes of LPs 2 and 3
    eng = _lib.RaggedEngine(shapes_of(first), log_cap=LOG_CAP)
    for i in range(6):
        assert eng.lib.lp_ragged_shape(eng.h, i, None, None) == _lib.PIVOTED
    m, n = ctypes.c_int64(), ctypes.c_int64()
    assert eng.lib.lp_ragged_shape(eng.h, 3, ctypes.byref(m), ctypes.byref(n)) == _lib.PIVOTED
    assert (m.value, n.value) == (40, 80)
    assert eng.lib.lp_ragged_shape(eng.h, 6, None, None) == _lib.BAD_ARG
    eng.upload(first[:3])
    eng.upload(first[3:], first=3)
    assert all(same_bits(a, b) for a, b in zip(eng.download(), first))
    eng.solve(CAP)
    solved = eng.download()
    logs = [eng.log(i).tolist() for i in range(6)]
    for i in range(6):
        assert same_bits(solved[i], oracle_solve(first[i])[3]) and logs[i] == oracle_solve(first[i])[1].tolist()
    eng.upload(fresh, first=2)
    whole = eng.download()
    assert same_bits(whole[2], fresh[0]) and same_bits(whole[3], fresh[1])
    for i in (0, 1, 4, 5):
        assert same_bits(whole[i], solved[i])                       # every other LP's bytes unchanged
        assert eng.log(i).tolist() == logs[i]
    assert eng.log(2).shape == (0, 2) and eng.log(3).shape == (0, 2)            # state reset
    for a, k in ((0, 2), (2, 2), (1, 4), (5, 1), (3, 0), (6, 0)):
        assert all(same_bits(x, y) for x, y in zip(eng.download(a, k), whole[a:a + k])), (a, k)
    with pytest.raises(ValueError):
        eng.upload(fresh, first=5)
    with pytest.raises(ValueError):
        eng.upload(fresh, first=3)                                  # the shapes of LPs 3 and 4 are others
    src = np.zeros(4)
    assert eng.lib.lp_ragged_upload(eng.h, 5, 2, _lib._ptr(src)) == _lib.BAD_ARG
    assert eng.lib.lp_ragged_upload(eng.h, 0, 1, None) == _lib.BAD_ARG
    st2, npiv2, _ = eng.solve(CAP)
    again = eng.download()
    for k, i in enumerate((2, 3)):
        o = oracle_solve(fresh[k])
        assert st2[i] == o[0] and eng.log(i).tolist() == o[1].tolist() and same_bits(again[i], o[3])
    for i in (0, 1, 4, 5):      # a new solve of an optimal tableau: what the oracle does with it
        o = oracle_solve(solved[i])
        assert st2[i] == o[0] and npiv2[i] == len(o[1]) == 0 and same_bits(again[i], o[3])
    eng.close()


# ---------------------------------------------------------------------------
# 6. basis; the uniform layout calls on a ragged batch, the packed ones on a uniform one
# ---------------------------------------------------------------------------

def test_packed_basis_and_the_layout_calls():
    lps = window_list()
    eng = _lib.RaggedEngine(shapes_of(lps), log_cap=LOG_CAP)
    eng.upload(lps)
    with pytest.raises(ValueError, match="no basis"):
        eng.get_basis()
    marks = [np.arange(T.shape[0] - 1, dtype=np.int32) * 7 + 100 * i for i, T in enumerate(lps)]
    eng.set_basis(marks)
    assert [b.tolist() for b in eng.get_basis()] == [b.tolist() for b in marks]
    basis0 = ragged_canonical_basis(lps)
    eng.set_basis(basis0)
    eng.solve(CAP)
    for i, b in enumerate(eng.get_basis()):
        want = basis0[i].tolist()
        for r, c in eng.log(i).tolist():
            want[r] = c
        assert b.tolist() == want and eng.log(i).tolist() == oracle_solve(lps[i])[1].tolist(), i
    # the four calls whose layout assumes one shape name their counterpart
    buf = np.zeros(sum(T.size for T in lps))
    ibuf = np.zeros(sum(T.shape[0] for T in lps), dtype=np.int32)
    calls = [("lp_ragged_upload", lambda: eng.lib.lp_batch_upload(eng.h, 0, 1, _lib._ptr(buf), 100)),
             ("lp_ragged_download", lambda: eng.lib.lp_batch_download(eng.h, 0, 1, _lib._ptr(buf), 100)),
             ("lp_ragged_set_basis", lambda: eng.lib.lp_batch_set_basis(eng.h, ibuf.ctypes.data_as(_lib._P32))),
             ("lp_ragged_get_basis", lambda: eng.lib.lp_batch_get_basis(eng.h, ibuf.ctypes.data_as(_lib._P32)))]
    before = eng.download()
    for name, call in calls:
        assert call() == _lib.BAD_ARG, name
        assert name in eng.lib.lp_batch_last_error(eng.h).decode(), name
    assert all(same_bits(a, b) for a, b in zip(eng.download(), before))
    eng.set_basis(None)
    with pytest.raises(ValueError, match="no basis"):
        eng.get_basis()
    eng.close()


def test_packed_calls_on_a_uniform_batch():
    stack = gen.mixed_stack(8, 10, range(1, 6))
    eng = _lib.BatchEngine(5, 8, 18, log_cap=LOG_CAP)
    lib = eng.lib
    assert lib.lp_ragged_upload(eng.h, 1, 4, _lib._ptr(np.ascontiguousarray(stack[1:]))) == _lib.PIVOTED
    eng.upload(stack[:1])
    assert same_bits(eng.download(), stack)                         # packed = ldh n + 1
    basis0 = np.ascontiguousarray(ragged_canonical_basis(list(stack)), dtype=np.int32)
    assert lib.lp_ragged_set_basis(eng.h, basis0.ctypes.data_as(_lib._P32)) == _lib.PIVOTED
    assert eng.get_basis().tolist() == basis0.tolist()
    st, npiv, nstd = eng.solve(CAP)
    out = np.empty((3, 9, 19))
    assert lib.lp_ragged_download(eng.h, 2, 3, _lib._ptr(out)) == _lib.PIVOTED
    got = np.empty((5, 8), dtype=np.int32)
    assert lib.lp_ragged_get_basis(eng.h, got.ctypes.data_as(_lib._P32)) == _lib.PIVOTED
    assert got.tolist() == eng.get_basis().tolist()
    for i in range(5):
        o = oracle_solve(stack[i])
        assert st[i] == o[0] and eng.log(i).tolist() == o[1].tolist()
        if i >= 2:
            assert same_bits(out[i - 2], o[3])
    m, n = ctypes.c_int64(), ctypes.c_int64()
    assert lib.lp_ragged_shape(eng.h, 4, ctypes.byref(m), ctypes.byref(n)) == _lib.PIVOTED
    assert (m.value, n.value) == (8, 18)
    assert _lib.ragged_plan(eng) == [dict(waves=1, lds_bytes=_lib.batch_lds_bytes(8, 18), lps=5,
                                          lps_per_cu=_lib.ragged_plan(eng)[0]["lps_per_cu"])]
    assert _lib.ragged_plan(eng, True)[0]["lds_bytes"] == _lib.twophase_lds_bytes(8, 18)
    eng.close()


# ---------------------------------------------------------------------------
# 7. fixed-rule run
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX])
def test_fixed_rule_run(rule):
    fx = next(f for f in SMALL["solve"] if f["name"] == "km_deg_d6")
    lps = [gen.tableau("mixed", 40, 40, 1), fixture_input(fx), gen.tableau("mixed", 3, 3, 2),
           gen.tableau("mixed", 16, 16, 11), gen.tableau("mixed", 1, 1, 1)]
    res = solve_ragged(lps, rule=rule, steps=7, log_cap=8)
    for i, T in enumerate(lps):
        o = F64Tableau(T)
        st, log = o.run(rule, 7)
        assert res.status_code[i] == st, i
        assert res.npiv[i] == len(log), i
        assert res.nstd[i] == (len(log) if rule == _lib.RULE_STANDARD else 0), i
        assert res.log(i).tolist() == log.tolist(), i
        assert same_bits(res.tableaux[i], o.T), i
    assert res.npiv[1] == 7 and res.status[1] == "pivoted"
    assert res.status[4] in ("optimal", "unbounded") and res.npiv[4] < 7


# ---------------------------------------------------------------------------
# 8. two-phase on the 17-LP list
# ---------------------------------------------------------------------------

def lp_record(r, n):
    """an LPRaggedResult as the record tc.check_lp reads"""
    return dict(status=r.status_code.tolist(), stage=r.stage.tolist(), rows=r.rows.tolist(),
                ninit=r.ninit.tolist(), npiv=r.npiv.tolist(), nstd=r.nstd.tolist(),
                T=r.tableaux, z=r.objective, basis=[b.tolist() for b in r.basis],
                log=[r._engine.log(i).tolist() for i in range(n)])


def engine_solve_lp(lps, *, cap, chunk=None, eng=None):
    own = eng is None
    if own:
        eng = _lib.RaggedEngine(shapes_of(lps), log_cap=LOG_CAP)
    try:
        if chunk is not None:
            eng.set_chunk(chunk)
        eng.upload(lps)
        status, stage, rows, ninit, npiv, nstd = eng.solve_lp(cap)
        return dict(status=status.tolist(), stage=stage.tolist(), rows=rows.tolist(), ninit=ninit.tolist(),
                    npiv=npiv.tolist(), nstd=nstd.tolist(), T=eng.download(), z=eng.objective(),
                    basis=[b.tolist() for b in eng.get_basis()],
                    log=[eng.log(i).tolist() for i in range(len(lps))])
    finally:
        if own:
            eng.close()


def test_twophase_list_oracle_outcomes():
    """what the list is there for, on the oracle's side: a generator change cannot hollow the test out"""
    lps = rc.twophase_list()
    assert len(lps) == 17 and len({T.shape for T in lps}) >= 13
    for i, T in enumerate(lps):
        o = tc.report(T, cap=rc.TWOPHASE_CAP)
        if i == rc.TWOPHASE_INFEASIBLE_AT:
            assert (o["status"], o["stage"]) == (tc.INFEASIBLE, tc.ARTIFICIAL), i
        else:
            assert (o["status"], o["stage"]) == (tc.OPTIMAL, tc.PHASE2), i
        m = T.shape[0] - 1
        assert o["rows"] == (m - 1 if i in rc.TWOPHASE_DROPS_A_ROW else m), i
        assert (_lib.twophase_waves(*rc.shape_of(T)) == 4) == (i in rc.TWOPHASE_FOUR_WAVE), i


@pytest.mark.parametrize("chunk", [None, 1])
def test_twophase_list(chunk):
    lps = rc.twophase_list()
    if chunk is None:
        r = solve_lp_ragged(lps, max_pivots=rc.TWOPHASE_CAP, log_cap=LOG_CAP)
        res = lp_record(r, len(lps))
        plan = r.plan()
        assert len(plan) == 4 and sum(b["lps"] for b in plan) == 17
        assert sum(b["lps"] for b in plan if b["waves"] == 4) == 4
        # the front-end's views of the same
        o = tc.report(lps[9], cap=rc.TWOPHASE_CAP)
        assert r.init_log(9).tolist() == o["init_seq"] and r.log(9).tolist() == o["seq"]
        assert r.tableau(9).getTableauSize() == (o["rows"], lps[9].shape[1] - 1)
        assert r.status[rc.TWOPHASE_INFEASIBLE_AT] == "infeasible"
    else:
        res = engine_solve_lp(lps, cap=rc.TWOPHASE_CAP, chunk=chunk)
    for i, T in enumerate(lps):
        tc.check_lp(res, i, T, tc.report(T, cap=rc.TWOPHASE_CAP), where=f"chunk {chunk}")


def test_phase1_goldens_in_one_call():
    fxs = SMALL["phase1"]
    lps = [fixture_input(fx) for fx in fxs]
    assert len({T.shape for T in lps}) > 1
    r = solve_lp_ragged(lps, max_pivots=CAP, log_cap=LOG_CAP)
    for i, fx in enumerate(fxs):
        init, seq = r.init_log(i).tolist(), r.log(i).tolist()
        if fx.get("error") == "ValueError":
            assert r.status[i] == "infeasible" and r.stage[i] == _lib.STAGE_ARTIFICIAL, fx["name"]
            assert init == fx["init_seq"] and seq == [], fx["name"]
            continue
        assert r.status[i] == "optimal" and r.stage[i] == _lib.STAGE_PHASE2, fx["name"]
        assert init == fx["init_seq"], fx["name"]
        if fx.get("error") == "IndexError":             # the reference stops there; a row is dropped
            assert r.rows[i] == fx["m"] - 1, fx["name"]
            continue
        assert [int(r.rows[i]), lps[i].shape[1] - 1] == fx["init_size"], fx["name"]
        assert seq == fx["seq"], fx["name"]
        assert r.basis[i][:r.rows[i]].tolist() == fx["bfs"], fx["name"]
        assert r.basis[i][r.rows[i]:].tolist() == [-1] * (lps[i].shape[0] - 1 - int(r.rows[i])), fx["name"]
        tc.check_lp(lp_record(r, len(lps)), i, lps[i], tc.report(lps[i], cap=CAP), where=fx["name"])


# ---------------------------------------------------------------------------
# 9. two-phase: the uniform path per shape gives the same
# ---------------------------------------------------------------------------

def test_twophase_equal_to_the_uniform_path():
    lps = [tc.wide_stack()[0], gen.phase1_lp("ge", 3, 4, 1), gen.phase1_lp("ge", 3, 4, 2)]
    assert rc.shape_of(lps[0]) == (90, 128)
    o = [tc.report(T, cap=tc.PROBE_CAP) for T in lps]
    cap = max(tc.per_solve(x) for x in o) + tc.SAFETY
    r = solve_lp_ragged(lps, max_pivots=cap, log_cap=LOG_CAP)
    assert [b["waves"] for b in r.plan()] == [4, 1]
    assert r.plan()[0]["lds_bytes"] == _lib.twophase_lds_bytes(90, 128)
    res = lp_record(r, 3)
    for i, T in enumerate(lps):
        tc.check_lp(res, i, T, tc.report(T, cap=cap), where="ragged")
    for idx in ([0], [1, 2]):
        u = solve_lp_batch(np.stack([lps[i] for i in idx]), max_pivots=cap, log_cap=LOG_CAP)
        for k, i in enumerate(idx):
            assert (u.status_code[k], u.stage[k], u.rows[k]) == (r.status_code[i], r.stage[i], r.rows[i]), i
            assert (u.ninit[k], u.npiv[k], u.nstd[k]) == (r.ninit[i], r.npiv[i], r.nstd[i]), i
            assert u.init_log(k).tolist() == r.init_log(i).tolist() and u.log(k).tolist() == r.log(i).tolist(), i
            assert u.basis[k].tolist() == r.basis[i].tolist(), i
            assert same_bits(u.tableaux[k], r.tableaux[i]), i


# ---------------------------------------------------------------------------
# 10. two-phase refusal
# ---------------------------------------------------------------------------

def test_twophase_refuses_an_lp_that_is_too_large():
    m = _lib.twophase_max_m(128) + 1
    assert _lib.twophase_lds_bytes(m, 128) > _lib.BATCH_LDS_MAX >= _lib.batch_lds_bytes(m, 128)
    big = gen.tableau("mixed", m, 128 - m, 1)
    assert rc.shape_of(big) == (m, 128)
    lps = [gen.tableau("mixed", 8, 10, 1), gen.tableau("mixed", 16, 16, 11), big, gen.tableau("mixed", 3, 3, 2)]
    eng = _lib.RaggedEngine(shapes_of(lps), log_cap=LOG_CAP)
    eng.upload(lps)
    with pytest.raises(ValueError, match=r"LP 2 .*too large"):
        eng.solve_lp(CAP)
    st = eng.lib.lp_twophase_solve(eng.h, CAP, None, None, None, None, None, None)
    assert st == _lib.BAD_ARG and b"too large" in eng.lib.lp_batch_last_error(eng.h)
    with pytest.raises(ValueError, match=r"LP 2 .*too large"):
        eng.plan(twophase=True)
    assert all(same_bits(a, b) for a, b in zip(eng.download(), lps))       # nothing launched
    # the batch is still good for the plain solve
    eng.set_basis(ragged_canonical_basis(lps))
    res_st, npiv, nstd = eng.solve(CAP)
    out = eng.download()
    for i, T in enumerate(lps):
        o = oracle_solve(T)
        assert res_st[i] == o[0] and eng.log(i).tolist() == o[1].tolist()[:LOG_CAP] and same_bits(out[i], o[3]), i
    eng.close()


# ---------------------------------------------------------------------------
# 11. one handle, call after call
# ---------------------------------------------------------------------------

def test_handle_reuse():
    lps = [gen.tableau("mixed", 8, 10, 1), gen.phase1_lp("ge", 3, 4, 1), gen.tableau("mixed", 40, 40, 1),
           gen.phase1_lp("dep", 6, 8, 2), gen.tableau("mixed", 3, 3, 2), gen.phase1_lp("ge", 32, 32, 2)]
    canonical = (0, 2, 4)
    cap = rc.TWOPHASE_CAP
    none = [np.full(T.shape[0] - 1, -1, dtype=np.int32) for T in lps]
    eng = _lib.RaggedEngine(shapes_of(lps), log_cap=LOG_CAP)

    # solve: every LP as lpf_solve takes it, canonical or not
    a = engine_solve(lps, cap=cap, basis=none, eng=eng)
    fresh = engine_solve(lps, cap=cap, basis=none)
    for i, T in enumerate(lps):
        same_lp(a, i, fresh, i, "solve")
        assert_lp_matches_oracle(a, i, T, cap=cap, basis0=none)
    # solve_lp on the same handle, from the uploaded tableaux
    b = engine_solve_lp(lps, cap=cap, eng=eng)
    fresh = engine_solve_lp(lps, cap=cap)
    for i, T in enumerate(lps):
        tc.same_result({k: v[i] for k, v in b.items()}, {k: v[i] for k, v in fresh.items()})
        tc.check_lp(b, i, T, tc.report(T, cap=cap), where="solve_lp")
    # a window in the middle, then solve again: LPs 2 and 3 anew, the others from where they are
    after_lp = eng.download()
    window = [gen.tableau("mixed", 40, 40, 2), gen.phase1_lp("eq", 7, 8, 3)]
    assert [T.shape for T in window] == [lps[2].shape, lps[3].shape]
    eng.upload(window, first=2)
    now = after_lp[:2] + window + after_lp[4:]
    assert all(same_bits(x, y) for x, y in zip(eng.download(), now))
    eng.set_basis(none)
    st, npiv, nstd = eng.solve(cap)
    c = dict(status=st.tolist(), npiv=npiv.tolist(), nstd=nstd.tolist(), T=eng.download(), z=eng.objective(),
             log=[eng.log(i).tolist() for i in range(len(lps))], basis=[x.tolist() for x in eng.get_basis()])
    fresh = engine_solve(now, cap=cap, basis=none)
    for i, T in enumerate(now):
        same_lp(c, i, fresh, i, "after the window")
        assert_lp_matches_oracle(c, i, T, cap=cap, basis0=none)
    for i in canonical:
        if i != 2:
            assert c["npiv"][i] == 0 and c["status"][i] == _lib.OPTIMAL        # solved already
    eng.close()
