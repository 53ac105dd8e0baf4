"""lp_cut_extend, extend_into / extend and ProblemResult.add_rows on the GPU,
where the first tests do not look (csrc/batch.hip: k_cut_copy, k_cut_rows,
k_cut_basis, the staging in lp_cut_extend): windows whose lanes
lie in later workgroups on a ragged side, windows and runs of LPs that get no
row, three groups of rows and groups wider than a wave, the regrowth of the
staged table and rows, a destination whose last call was a two-phase solve that
dropped a row, teams, sources on one side of the one-wave and LDS thresholds
whose extended LPs are on the other, and stated rows near overflow and in the
subnormal range.

Every comparison is bit for bit with the host statement of tests/_cut_cases.py
(extend(), then _dual_cases.walk); nothing expected comes from the device.  The
inputs, and where their lanes fall, are vetted by tests/test_cut_cases_cpu.py."""
import numpy as np
import pytest

import _cut_cases as cc
import _dual_cases as dc
import _problem_cases as pc
import _reopt_cases as rc
from lpsol_amd import _lib, solve_problems
from test_gpu_batch_cut import (assert_extended, assert_same_state, assert_walked, destination, shape_of, source,
                                state, stated)

pytestmark = pytest.mark.gpu

same_bits = dc.same_bits
CAP, LOG, GROUP = dc.CAP, dc.LOG_CAP, cc.GROUP


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def filled(dst, cases):
    """upload a tableau of 1 + i in every cell of LP i: what an LP outside a window must keep"""
    fill = [np.full(c["D"].shape, 1.0 + i) for i, c in enumerate(cases)]
    dst.upload(fill if hasattr(dst, "shapes") else np.stack(fill))
    return fill


def state_or_none(dst):
    """state(), a destination no basis was attached to yet holding -1 throughout: what the first window leaves"""
    try:
        return state(dst)
    except ValueError as e:
        assert "no basis attached" in str(e)
        shapes = dst._lp_shapes()
        return dict(T=[np.array(t) for t in dst.download()], basis=[np.full(m, -1, dtype=np.int32) for m, _ in shapes])


def assert_window(src, dst, cases, first, count, held=None):
    """extend_into on [first, first + count): the window is the host loop's, the source and the rest of dst stay"""
    before, was = state(src), (state_or_none(dst) if held is None else held)
    window = cases[first:first + count]
    src.extend_into(dst, *stated(window), first=first)
    got = assert_extended(dst, window, first)
    assert_same_state(got, was, [i for i in range(len(cases)) if not first <= i < first + count])
    assert_same_state(state(src), before)
    return got


# ---------------------------------------------------------------------------
# 6. k_cut_rows and k_cut_basis on windows of more than one workgroup
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ragged_to_ragged", "uniform_to_ragged", "copy"])
def test_windows_across_workgroups_on_a_ragged_side(name):
    batch, windows, walked = dict(ragged_to_ragged=(cc.BLOCK, cc.BLOCK_WINDOWS, cc.BLOCK_WALKED),
                                  uniform_to_ragged=(cc.UNIFORM_BLOCK, cc.UNIFORM_WINDOWS, cc.UNIFORM_WINDOWS[1]),
                                  copy=(cc.COPY_BLOCK, cc.COPY_WINDOWS, cc.COPY_WINDOWS[1]))[name]
    cases = cc.block_cases(batch)
    src = source(cases, ragged=name != "uniform_to_ragged", place="auto")
    held = state(src)
    for first, count in windows:
        dst = destination(cases, True, place="auto")            # fresh: no basis was ever attached to it
        fill = filled(dst, cases)
        window = cases[first:first + count]
        src.extend_into(dst, *stated(window), first=first)
        got = assert_extended(dst, window, first)
        for i in range(len(cases)):
            if not first <= i < first + count:
                assert same_bits(got["T"][i], fill[i]) and (got["basis"][i] == -1).all(), (first, count, i)
        assert_same_state(state(src), held)
        if (first, count) == walked:
            assert_walked(dst, window, first)
        dst.close()
    # the windows one after another on one kept destination: each leaves what the others wrote
    dst = destination(cases, True, place="auto")
    filled(dst, cases)
    for first, count in windows[1:]:
        assert_window(src, dst, cases, first, count)


# ---------------------------------------------------------------------------
# 7. windows in which no LP gets a row
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "uniform"])
def test_a_first_window_without_a_row_then_one_with_rows(ragged):
    batch = cc.ZERO_BATCH if ragged else [(8, 10, 0)] * 6
    cases = cc.block_cases(batch)
    src, dst = source(cases, ragged), destination(cases, ragged)
    held, B = state(src), len(cases)
    zeros = (0, 2) if ragged else (0, B)
    first, count = zeros
    # the very first call on a fresh destination stages no row and no sense
    src.extend_into(dst, [[] for _ in range(count)], [], first=first)
    got = state(dst)
    for i in range(first, first + count):
        assert same_bits(got["T"][i], held["T"][i]) and np.array_equal(got["basis"][i], held["basis"][i]), i
    for i in range(first + count, B):
        assert not got["T"][i].any() and (got["basis"][i] == -1).all(), i
    status, done = dst.run(_lib.RULE_DUAL, CAP)
    assert all(status[i] == _lib.OPTIMAL and done[i] == 0 for i in range(first, first + count))
    assert_same_state(state(dst), got, range(first, first + count))
    if not ragged:
        return
    # a window with rows on the same destination, runs of q = 0 LPs first, in the middle and last in it
    assert [q for _, _, q in batch[1:]] == [0, 0, 2, 0, 0, 3, 0, 0]
    assert_window(src, dst, cases, 1, B - 1)
    assert_walked(dst, cases[1:], 1)
    # and a window without a row again, now that rows were staged: per-LP empty senses as well
    was = state(dst)
    src.extend_into(dst, [np.zeros((0, 3))] * 2, [[], []], first=4)
    assert_extended(dst, cases[4:6], 4)
    assert_same_state(state(dst), was, [i for i in range(B) if i not in (4, 5)])
    assert_same_state(state(src), held)


# ---------------------------------------------------------------------------
# 8. three groups of rows, and groups wider than a wave
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("q", cc.GROUP_QS, ids=["2G+1", "3G"])
@pytest.mark.parametrize("shape,place", [(cc.SMALL, "lds"), (cc.LARGE, "lds"), (cc.LARGE, "device")],
                         ids=["8x10", "40x40", "40x40-device"])
def test_three_groups_of_rows(shape, place, q):
    assert q in (2 * GROUP + 1, 3 * GROUP) and (q + GROUP - 1) // GROUP == 3
    cases = cc.group_cases(shape, q)
    assert all(c["rows"].shape[0] == q for c in cases)
    src, dst = source(cases), destination(cases, place=place)
    assert dst.placement(0) == place
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    status = assert_walked(dst, cases)
    assert {int(s) for s in status} == {_lib.OPTIMAL, _lib.INFEASIBLE}


# ---------------------------------------------------------------------------
# 9. the staged table and rows grow, then shrink
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_staging_grows_with_the_window_and_shrinks_again(ragged):
    if ragged:
        cases, batch = cc.ragged_cases(), [(m, ns, cc.Q_CYCLE[i % 3]) for i, (m, ns) in enumerate(cc.RAGGED_SHAPES)]
        windows = [(4, 1), (3, 3), (0, 9), (2, 2), (7, 1)]
    else:
        cases, batch = [cc.case(*cc.SMALL, s, "lege") for s in range(1, 17)], [(*cc.SMALL, 2)] * 16
        windows = [(5, 1), (4, 3), (0, 16), (9, 2), (15, 1)]
    cost = [cc.window_cost(batch, *w) for w in windows]
    whole = windows.index((0, len(cases)))
    # the table is count + 1 entries of one size and one byte per row; the rows are doubles
    assert all(cost[whole][0] > c[0] and cost[whole][1] >= c[1] and cost[whole][2] > c[2] for c in cost[:whole])
    assert cost[0][2] > 0 and all(a[0] < b[0] and a[2] < b[2] for a, b in zip(cost[:whole], cost[1:whole + 1]))
    assert all(c[0] < cost[whole][0] and c[2] < cost[whole][2] for c in cost[whole + 1:])
    src, dst = source(cases, ragged), destination(cases, ragged)
    filled(dst, cases)
    for first, count in windows:
        assert_window(src, dst, cases, first, count)
    assert_window(src, dst, cases, 0, len(cases))
    assert_walked(dst, cases)


# ---------------------------------------------------------------------------
# 10. a destination whose last call was a two-phase solve that dropped a row
# ---------------------------------------------------------------------------

def test_a_destination_whose_last_solve_dropped_a_row():
    P, s = pc.dependent_block(3)
    P2, _ = pc.dependent_block(4)
    short = solve_problems(np.stack([P[0, 1:], P2[0, 1:]]), np.stack([P[1:, 1:], P2[1:, 1:]]),
                           np.stack([P[1:, 0], P2[1:, 0]]), s, log_cap=LOG)
    assert short.path == "twophase" and (short.rows < len(s)).all()
    dst = short._engine
    assert (dst.m, dst.n) == (4, 6) and all(len(dst.log(i)) > 0 for i in range(2))
    refusal = r"LP %d, row 3: its last two-phase call left 3 of 4 rows live"
    rows4, rhs4 = np.zeros((2, dst.n + 1)), np.zeros((2, dst.m + 1))
    with pytest.raises(ValueError, match=refusal % 0):
        dst.set_costs(rows4)
    # the source: one row and one column fewer, an uploaded optimum and its basis
    cases = [cc.case(3, 2, 1 + i, "lege", 1) for i in range(2)]
    assert all(shape_of(c["D"]) == (4, 6) for c in cases)
    src = source(cases)
    senses = ["<="] * 3 + [("<=", ">=")[int(cases[0]["sense"][0])]]
    dst.set_senses(senses)                                      # the joined senses; the flag stays
    with pytest.raises(ValueError, match=refusal % 0):
        dst.set_rhs(rhs4)
    was = state(dst)
    got = assert_window(src, dst, cases, 0, 1, held=was)
    # LP 1, outside the window, is still refused with its message, under both calls; LP 0 no longer
    for call, arg in ((dst.set_costs, rows4), (dst.set_rhs, rhs4)):
        with pytest.raises(ValueError, match=refusal % 1):
            call(arg)
        with pytest.raises(ValueError, match=refusal % 1):
            call(arg[1:], first=1)
    assert_same_state(state(dst), got)
    slack = dc.slack_table(_lib.sense_codes(senses), 2)
    rhs = np.concatenate([[0.25], dc.scale(np.concatenate([cases[0]["T0"][1:, 0], cases[0]["beta"]]), 5)])
    before, after = dc.assert_set_rhs(dst, [slack, slack], rhs[None], first=0)
    assert not same_bits(after["T"][0][:, 0], before["T"][0][:, 0])
    rc.assert_set_costs(dst, rc.some_costs(dst.n, 7)[None], first=0)
    # the window once more, then the walk: the log is the walk alone, not the two-phase solve's entries
    got = assert_window(src, dst, cases, 0, 1)
    status, done = dst.run(_lib.RULE_DUAL, CAP)
    w = cases[0]["warm"]
    assert (int(status[0]), int(done[0])) == (w["status"], w["npiv"]) and w["npiv"] >= 1
    assert dst.log(0).tolist() == w["log"]
    assert same_bits(dst.download(0, 1)[0], w["T"])
    with pytest.raises(ValueError, match=refusal % 1):
        dst.set_costs(rows4[1:], first=1)


# ---------------------------------------------------------------------------
# 11. teams
# ---------------------------------------------------------------------------

def test_a_teamed_destination_takes_the_rows_and_refuses_the_dual_rule():
    m, ns = cc.LARGE
    cases = [cc.case(m, ns, s, "lege") for s in range(1, 5)]
    src = source(cases, place="device")
    dst = destination(cases, place="device", team=2)
    assert dst.team_of(0) == 2
    src.extend_into(dst, *stated(cases))
    got = assert_extended(dst, cases)
    with pytest.raises(ValueError, match="team"):
        dst.run(_lib.RULE_DUAL, CAP)
    assert_same_state(state(dst), got)
    # extend() from a teamed source keeps the team, and is refused the same way; team=1 runs
    teamed = source(cases, place="device", team=2)
    assert teamed.team_of(0) == 2
    rows, sense = stated(cases)
    kept = teamed.extend(rows, sense)
    assert kept.team_of(0) == 2 and kept.placement(0) == "device"
    got = assert_extended(kept, cases)
    with pytest.raises(ValueError, match="team"):
        kept.run(_lib.RULE_DUAL, CAP)
    assert_same_state(state(kept), got)
    single = teamed.extend(rows, sense, team=1)
    assert single.team_of(0) == 1
    assert_extended(single, cases)
    status = assert_walked(single, cases)
    assert {int(s) for s in status} == {_lib.OPTIMAL, _lib.INFEASIBLE}


# ---------------------------------------------------------------------------
# 12, 13. sources on one side of a threshold, extended LPs on the other
# ---------------------------------------------------------------------------

def test_across_the_one_wave_threshold():
    m, ns = cc.THRESHOLD
    cases = [cc.case(m, ns, s, "lege") for s in range(1, 9)]
    assert dc.elems(cases[0]["opt"]) == 31 * 61 == 1891 <= dc.ONE_WAVE_ELEMS
    assert dc.elems(cases[0]["D"]) == 33 * 63 == 2079 > dc.ONE_WAVE_ELEMS
    src = _lib.BatchEngine(len(cases), m, ns + m, log_cap=LOG)
    src.upload(np.stack([c["T0"] for c in cases]))
    src.derive_basis()
    status, _, _ = src.solve()
    assert (status == _lib.OPTIMAL).all()
    held = state(src)
    for c, T, b in zip(cases, held["T"], held["basis"]):        # the one-wave solve ends where the oracle's does
        assert same_bits(T, c["opt"]) and np.array_equal(b, c["basis"])
    dst = destination(cases)
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    status = assert_walked(dst, cases)
    assert {int(s) for s in status} == {_lib.OPTIMAL, _lib.INFEASIBLE}
    assert_same_state(state(src), held)


def test_add_rows_across_the_lds_limit():
    m, ns = cc.LDS_EDGE
    assert _lib.batch_lds_bytes(m, ns + m) == 161720 <= 163840 < _lib.batch_lds_bytes(m + 2, ns + m + 2) == 166568
    cases = [cc.case(m, ns, s, "le") for s in (1, 2)]
    T0 = np.stack([c["T0"] for c in cases])
    c_, A, b = pc.parts(T0, ns)
    res = solve_problems(c_, A, b, log_cap=LOG, place="auto")
    assert res.status == ["optimal"] * 2 and res._engine.placement(0) == "lds"
    assert all(same_bits(t, c["opt"]) for t, c in zip(res._engine.download(), cases))
    cuts = (np.stack([c["a"] for c in cases]), np.stack([c["beta"] for c in cases]), cases[0]["sense"])
    with pytest.raises(ValueError, match=r'too large.*place="auto" solves such an LP from device memory'):
        res.add_rows(*cuts, place="lds")
    # the old result stays live
    assert same_bits(res.tableau(1).toArray(), cases[1]["opt"]) and res.y.shape == (2, m)
    new = res.add_rows(*cuts, place="auto")
    assert new._engine.placement(0) == "device" and new._engine is not res._engine
    for i, c in enumerate(cases):
        st, npiv, x, z = cc.warm_answer(c)
        assert (new.status_code[i], new.npiv[i]) == (st, npiv) and npiv > 0, i
        assert same_bits(np.asarray(new.x[i]), x[:ns]) and same_bits(new.objective[i], z), i
        assert same_bits(new._engine.download(i, 1)[0], c["warm"]["T"]), i
    assert new.path == "dual" and same_bits(res.tableau(0).toArray(), cases[0]["opt"])


# ---------------------------------------------------------------------------
# 14. stated rows near overflow and in the subnormal range
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("how", cc.EXTREME_ROWS)
def test_extreme_stated_rows(how):
    T, basis, rows, sense = cc.odd_case()
    small = cc.case(*cc.SMALL, 3, "lege", 3)
    for src_T, src_basis, r, s in ((T, basis, rows, sense), (small["opt"], small["basis"], small["rows"], small["sense"])):
        r = cc.extreme_rows(r, how)
        want, wbasis = cc.extend(src_T, src_basis, r, s)
        m, n = shape_of(src_T)
        src = _lib.BatchEngine(2, m, n)
        src.upload(np.stack([src_T, src_T]))
        src.set_basis(np.stack([src_basis, src_basis]))
        dst = _lib.BatchEngine(2, *shape_of(want))
        src.extend_into(dst, [r, r], s)
        got = state(dst)
        nan = np.isnan(want)
        for i in range(2):
            D = got["T"][i]
            assert same_bits(D[:m + 1, :n + 1], src_T)
            assert np.array_equal(np.isnan(D), nan) and same_bits(D[~nan], want[~nan])
            assert np.array_equal(got["basis"][i], wbasis)
