"""Teamed batches on the GPU (lp_teamed_*, team= of BatchEngine / RaggedEngine
/ solve_batch / solve_ragged; csrc/batch.hip k_batch_team): a device-placed LP
worked on by several workgroups, one launch per pivot, the updated tableau
written out of place.

Every comparison is exact: status, pivot counts, the log, the basis and the
objective are equal to the oracle's (oracle/lp_f64.c through
_contract_cases.oracle_solve), and the tableaux are bit-identical (same_values
where the input holds non-finite cells).  Every device call carries a finite
pivot cap."""
import numpy as np
import pytest

from conftest import fixture_input

import _contract_cases as cc
import _ragged_cases as rc
from _team_cases import check, check_plan, check_stack, oracle_solve, ragged_mix, records, teamed_solve
from lpsol_amd import _lib, solve_batch, solve_ragged
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis

pytestmark = pytest.mark.gpu

CAP = 4096
LDS = _lib.BATCH_LDS_MAX


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


# ---------------------------------------------------------------------------
# 1. forced teams at the golden shapes
# ---------------------------------------------------------------------------

GOLDEN = [("cfg1_", 12, 2), ("cfg1_", 12, 3), ("cfg1_", 12, 5), ("cfg1_", 12, 7),
          ("mixed_40x40", 3, 2), ("mixed_40x40", 3, 16), ("pos_64x64", 2, 3)]


@pytest.mark.parametrize("prefix,count,team", GOLDEN, ids=["%s-team%d" % (p.rstrip("_"), g) for p, _, g in GOLDEN])
def test_golden_solves_forced_team(small_golden, prefix, count, team):
    """cfg1 is 9 x 19, E = 171: the odd LPs start at odd doubles, seven ranges are
    shorter than one pass of a workgroup (an empty main loop for most threads,
    the peeled ends alone at the LP's edges) and straddle row ends"""
    fxs = [fx for fx in small_golden["solve"] if fx["name"].startswith(prefix)]
    assert len(fxs) == count
    stack = np.stack([fixture_input(fx) for fx in fxs])
    if prefix == "cfg1_":
        assert stack.shape[1:] == (9, 19)
    basis0 = canonical_basis(stack)
    got = teamed_solve(stack, team, basis=basis0, teams=[team] * count)
    want = check_stack(got, stack, basis0=basis0)
    for fx, g, w in zip(fxs, got, want):
        assert g["status"] == _lib.OPTIMAL and g["log"] == fx["seq"] and g["basis"] == fx["bfs"], fx["name"]
        assert g["nstd"] == fx["nstd"], fx["name"]
    res = solve_batch(stack, place="device", team=team, log_cap=4, max_pivots=CAP)
    for i, w in enumerate(want):
        assert res.status_code[i] == w["status"] and res.log(i).tolist() == w["log"][:4]
        assert cc.same_bits(res.tableaux[i], w["T"]) and res.objective[i] == w["z"]
        assert res.basis[i].tolist() == got[i]["basis"]


# ---------------------------------------------------------------------------
# 2. every outcome at team 3
# ---------------------------------------------------------------------------

def _groups():
    out = {}
    for c in cc.CASES:
        key = (tuple(sorted((c["tol"] or {}).items())), c["cap"])
        out.setdefault(key, []).append(c["name"])
    return list(out.values())


@pytest.mark.parametrize("m,n,row_at", cc.EMBEDDINGS[1:])
def test_special_cases(m, n, row_at):
    """NaN in b, a and c, the overflowing ratio rows, the -inf cost, the negative
    b (LP_OBJ_INCREASED: the objective every workgroup computes for itself), the
    NaN band's unbounded and the all-zero column, under same_values"""
    seen, statuses = 0, set()
    for names in _groups():
        cases, stack = cc.case_stack(m, n, row_at, names)
        tol, cap = cases[0]["tol"], cases[0]["cap"]
        got = teamed_solve(stack, 3, cap=cap, tol=tol, log_cap=8, teams=[3] * len(cases))
        check_stack(got, stack, cap=cap, tol=tol, finite=False)
        for c, g, T in zip(cases, got, stack):
            assert g["status"] == c["status"], c["name"]
            assert g["log"] == cc.mapped_log(c, row_at), c["name"]
            assert g["nstd"] == c["nstd"], c["name"]
            assert cc.same_values(g["T"], T) == c["untouched"], c["name"]
            statuses.add(g["status"])
        seen += len(cases)
    assert seen == len(cc.CASES)
    assert statuses == {cc.OPTIMAL, cc.UNBOUNDED, cc.OBJ_INCREASED, cc.CAP_REACHED}


def test_unbounded_and_the_cap_around_the_pivot_count():
    stack = gen.mixed_stack(8, 10, range(1, 5))
    p = [oracle_solve(T)["npiv"] for T in stack]
    assert p[0] == 6 and max(p) == 9
    for cap in (0, 5, 6, 7, 9, 10):         # below, at and one above LP 0's pivot count; at and above the largest
        got = teamed_solve(stack, 3, cap=cap, log_cap=16, teams=[3] * 4)
        want = check_stack(got, stack, cap=cap)
        assert want[0]["status"] == (cc.CAP_REACHED if cap <= 6 else cc.OPTIMAL)
    ub = cc.base_lp()
    ub[1:, 1] = -1.0                        # the entering column has no positive entry
    got = teamed_solve(ub[None], 3, cap=8, log_cap=8)
    want = check_stack(got, ub[None], cap=8)
    assert want[0]["status"] == cc.UNBOUNDED and want[0]["npiv"] == 0


def zero_then_real():
    """pivot = -1 makes a zero entry eligible.  Column 2 (cost -5) is all zero:
    the standard rule enters it and counts a zero pivot, m + n = 8 times, until
    the stall counter switches to the min-index rule; that enters column 1 and
    applies a real pivot; then column 2 again, zero pivots up to the cap"""
    T = cc.base_lp()
    T[0, 2] = -5.0
    return T


def test_a_zero_pivot_is_counted_not_applied_and_does_not_flip():
    T = zero_then_real()
    tol = dict(pivot=-1.0)
    for cap in (8, 9, 12):
        w = oracle_solve(T, cap, tol)
        assert w["status"] == cc.CAP_REACHED and w["npiv"] == cap and w["nstd"] == 8
        assert w["log"][:8] == [[0, 1]] * 8 and (cap == 8 or w["log"][8] == [1, 0])
        assert cc.same_bits(w["T"], T) == (cap == 8)
        for window in (1, 3, None):
            stack = np.stack([T, T])
            got = teamed_solve(stack, 3, cap=cap, tol=tol, window=window, log_cap=16, teams=[3, 3])
            check_stack(got, stack, cap=cap, tol=tol)


def test_beale_stalls_and_switches_to_the_min_index_rule():
    T = gen.beale()
    w = oracle_solve(T)
    assert w["status"] == cc.OPTIMAL and w["nstd"] < w["npiv"]      # the switch happened
    stack = np.stack([T, T])
    for team in (2, 3):
        got = teamed_solve(stack, team, log_cap=64, teams=[team] * 2)
        check_stack(got, stack)


# ---------------------------------------------------------------------------
# 3. window independence
# ---------------------------------------------------------------------------

def test_window_independence():
    """Klee-Minty d = 8: 255 pivots, and 254 under a cap, so the odd and the even
    count both end in either buffer whatever the window"""
    km = gen.klee_minty(8)
    stack = np.stack([km, gen.klee_minty(8, degenerate=True)])
    basis0 = canonical_basis(stack)
    for cap in (CAP, 254):
        w = oracle_solve(km, cap)
        assert w["npiv"] == min(cap, 255) and w["status"] == (cc.OPTIMAL if cap == CAP else cc.CAP_REACHED)
        results = [teamed_solve(stack, 2, cap=cap, window=k, basis=basis0, log_cap=256, teams=[2, 2])
                   for k in (1, 2, 5, None)]
        check_stack(results[-1], stack, cap=cap, basis0=basis0)
        for r in results[:-1]:
            for a, b in zip(r, results[-1]):
                check(a, b)
                assert a["basis"] == b["basis"]


# ---------------------------------------------------------------------------
# 4. calls in sequence on one engine
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX])
def test_run_twice_equals_one_run(rule):
    """run(3) ends in the second buffer: the copy home and the reset of the
    buffer index are what the download and the second run see"""
    stack = gen.mixed_stack(8, 10, range(1, 4))
    eng = _lib.BatchEngine(3, 8, 18, log_cap=8, place="device", team=3)
    eng.upload(stack)
    st, done = eng.run(rule, 3)
    mid = eng.download()
    for i, T in enumerate(stack):
        w = cc.oracle_run(T, rule, 3)
        assert (st[i], done[i]) == (w["status"], w["npiv"])
        assert cc.same_bits(mid[i], w["T"]) and eng.log(i).tolist() == w["log"]
    assert 3 in done.tolist()                           # an odd count: those LPs ended in the second buffer
    assert eng.objective().tolist() == [-T[0, 0] for T in mid]
    st, done = eng.run(rule, 3)
    twice = eng.download()
    eng.close()
    fresh = _lib.BatchEngine(3, 8, 18, log_cap=8, place="device", team=3)
    fresh.upload(stack)
    st6, done6 = fresh.run(rule, 6)
    once = fresh.download()
    fresh.close()
    assert cc.same_bits(twice, once)
    for i, T in enumerate(stack):
        w = cc.oracle_run(T, rule, 6)
        assert (st6[i], done6[i]) == (w["status"], w["npiv"]) and cc.same_bits(once[i], w["T"])
    assert 6 in done6.tolist()


def test_solve_upload_solve_with_a_basis():
    first = gen.mixed_stack(8, 10, range(1, 4))
    second = gen.mixed_stack(8, 10, range(11, 14))
    eng = _lib.BatchEngine(3, 8, 18, log_cap=32, place="device", team=5)
    check_plan(eng, [5, 5, 5])
    for stack in (first, second, first):
        basis0 = canonical_basis(stack)
        eng.upload(stack)
        assert cc.same_bits(eng.download(), stack)
        eng.set_basis(basis0)
        assert eng.get_basis().tolist() == basis0.tolist()
        got = records(eng, *eng.solve(CAP), basis0)
        want = check_stack(got, stack, basis0=basis0)
        assert {w["npiv"] % 2 for w in want} == {0, 1}          # LPs end in either buffer
        # solved again: optimal at once, nothing moves
        st, npiv, _ = eng.solve(CAP)
        assert st.tolist() == [_lib.OPTIMAL] * 3 and npiv.tolist() == [0] * 3
        assert all(cc.same_bits(a, w["T"]) for a, w in zip(eng.download(), want))
    # a window upload resets only its LPs; the two-phase call ignores teams
    eng.upload(second[:1], first=1)
    st, npiv, _ = eng.solve(CAP)
    assert npiv.tolist() == [0, oracle_solve(second[0])["npiv"], 0]
    assert cc.same_bits(eng.download(1, 1)[0], oracle_solve(second[0])["T"])
    eng.upload(first)
    lp = eng.solve_lp(400)
    plain = _lib.BatchEngine(3, 8, 18, log_cap=32, place="device")
    plain.upload(first)
    assert [a.tolist() for a in lp] == [a.tolist() for a in plain.solve_lp(400)]
    assert cc.same_bits(eng.download(), plain.download())
    plain.close()
    eng.close()


# ---------------------------------------------------------------------------
# 5. ragged batches
# ---------------------------------------------------------------------------

def test_ragged_mix_of_placements_and_teams():
    """LDS-placed LPs, team-1 device LPs and teams of 2, 3, 5 and 7 in one call,
    in a scrambled order; the 3 x 3 LP makes the LPs behind it start at odd
    doubles"""
    lps, teams = ragged_mix()
    toff = np.concatenate([[0], np.cumsum([T.size for T in lps])])
    assert {int(toff[i]) % 2 for i, g in enumerate(teams) if g > 1} == {0, 1}
    where = ["device" if g > 1 or _lib.batch_lds_bytes(*rc.shape_of(T)) > LDS else "lds" for T, g in zip(lps, teams)]
    assert where == ["lds", "lds", "device", "device", "device", "lds", "device", "device", "lds"]
    basis0 = [np.full(T.shape[0] - 1, -1, dtype=np.int32) for T in lps]
    eng = _lib.RaggedEngine([rc.shape_of(T) for T in lps], log_cap=512, place="auto", team=teams)
    assert [eng.placement(i) for i in range(len(lps))] == where
    check_plan(eng, teams)
    plan = eng.plan()                                   # the launch bins hold the LPs of team 1 only
    assert plan[0]["lps"] == 1 and sum(b["lps"] for b in plan) == teams.count(1)
    eng.upload(lps)
    eng.set_basis(basis0)
    got = records(eng, *eng.solve(CAP), basis0)
    eng.close()
    check_stack(got, lps, basis0=basis0)                # caller order kept
    res = solve_ragged(lps, basis=basis0, place="auto", team=teams, log_cap=512, max_pivots=CAP)
    for i, g in enumerate(got):
        assert res.status_code[i] == g["status"] and res.log(i).tolist() == g["log"]
        assert cc.same_bits(res.tableaux[i], g["T"]) and res.basis[i].tolist() == [int(x) for x in g["basis"]]


# ---------------------------------------------------------------------------
# 6. auto
# ---------------------------------------------------------------------------

def test_auto_on_a_small_batch_of_large_lps():
    stack = gen.mixed_stack(100, 100, (1, 2, 3, 4))
    eng = _lib.BatchEngine(4, 100, 200, log_cap=8, place="auto", team="auto")
    assert [eng.placement(i) for i in range(4)] == ["device"] * 4
    g = eng.team_of(0)
    assert g > 1
    check_plan(eng, [g] * 4)
    eng.upload(stack)
    got = records(eng, *eng.solve(CAP), None)
    eng.close()
    want = [oracle_solve(T) for T in stack]
    for a, w in zip(got, want):
        check(a, dict(w, log=w["log"][:8]))
    res = solve_batch(stack, place="auto", team="auto", max_pivots=CAP)
    assert res._engine.team_of(3) == g and all(cc.same_bits(a, w["T"]) for a, w in zip(res.tableaux, want))
    # an LP that auto placement keeps in LDS has no team
    small = _lib.BatchEngine(2, 8, 18, place="auto", team="auto")
    assert [small.placement(i) for i in range(2)] == ["lds"] * 2 and small.team_plan() == []
    check_plan(small, [1, 1])
    small.close()


# ---------------------------------------------------------------------------
# 7. team 1 and the defaults
# ---------------------------------------------------------------------------

def test_team_one_is_the_placed_path():
    lib = _lib.load()
    stack = gen.mixed_stack(8, 10, range(1, 5))
    out = []
    for kw in (dict(), dict(team=1), dict(team="auto")):        # auto on an LDS batch: team 1
        eng = _lib.BatchEngine(4, 8, 18, log_cap=16, place="lds" if kw.get("team") == "auto" else "device", **kw)
        check_plan(eng, [1] * 4)
        eng.upload(stack)
        rec = records(eng, *eng.solve(CAP), None)
        out.append((rec, _lib.ragged_plan(eng)))
        eng.close()
    for rec, plan in out:
        check_stack(rec, stack)
    assert out[0][1] == out[1][1] and len(out[0][1]) == 1
    # the C call itself at team 1, next to lp_placed_create's batch
    import ctypes
    h = ctypes.c_void_p()
    assert lib.lp_teamed_create(4, 8, 18, 16, 0, _lib.PLACE_DEVICE, 1, ctypes.byref(h)) == _lib.PIVOTED
    g = ctypes.c_int()
    assert lib.lp_teamed_size(h, 3, ctypes.byref(g)) == _lib.PIVOTED and g.value == 1
    cnt = ctypes.c_int64(-1)
    assert lib.lp_teamed_plan(h, None, 0, ctypes.byref(cnt)) == _lib.PIVOTED and cnt.value == 0
    assert lib.lp_teamed_set_window(h, 0) == _lib.BAD_ARG
    assert lib.lp_batch_destroy(h) == _lib.PIVOTED
    # defaults: solve_batch / solve_ragged as before
    res = solve_batch(stack, log_cap=16, max_pivots=CAP)
    assert res._engine.team_of(0) == 1 and res._engine.placement(0) == "lds"
    assert all(cc.same_bits(a, r["T"]) for a, r in zip(res.tableaux, out[0][0]))
    rag = solve_ragged(list(stack), log_cap=16, max_pivots=CAP)
    assert rag._engine.team_of(0) == 1 and all(cc.same_bits(a, r["T"]) for a, r in zip(rag.tableaux, out[0][0]))


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------

def test_refusals_come_before_any_device_work():
    with pytest.raises(ValueError, match="LP_PLACE_LDS"):
        _lib.BatchEngine(2, 100, 200, place="lds", team=2)
    with pytest.raises(ValueError, match="largest team"):
        _lib.BatchEngine(2, 100, 200, place="auto", team=100000)
    with pytest.raises(ValueError, match=r"\(m\+1\)\(n\+1\) / 2"):
        _lib.BatchEngine(2, 2, 4, place="device", team=8)
    with pytest.raises(ValueError, match="LP 1:"):
        _lib.RaggedEngine([(100, 200), (2, 4)], place="device", team=[2, 8])
    with pytest.raises(ValueError, match="LP_PLACE_LDS"):
        solve_batch(gen.mixed_stack(8, 10, [1]), team=2)
    eng = _lib.BatchEngine(2, 2, 4, place="device", team=7)        # the largest team a 3 x 5 tableau takes
    check_plan(eng, [7, 7])
    with pytest.raises(ValueError):
        eng.set_window(0)
    with pytest.raises(ValueError):
        eng.team_of(2)
    eng.close()
