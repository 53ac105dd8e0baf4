"""lp_resolve_set_rhs and ProblemResult.resolve on the GPU, where the first
tests do not look (csrc/batch.hip: k_rhs, the short-row flag):
windows of more than one workgroup, batches that did not all end optimal, the
life cycle of the refusal after a two-phase call that dropped a row, the
device-placed two-phase path, and non-finite and extreme right-hand sides.

set_rhs is compared bit for bit (a NaN matching a NaN) with the host loop of
tests/_dual_cases.py applied to the tableau downloaded just before the call,
resolve and run with that loop followed by the host walk.  The inputs are
vetted on the oracle by tests/test_dual_cases_cpu.py."""
import re

import numpy as np
import pytest

import _dual_cases as dc
import _maxinc_cases as mc
import _problem_cases as pc
from lpsol_amd import _lib, solve_problems, solve_problems_ragged

pytestmark = pytest.mark.gpu

LE = _lib.SENSE_LE


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def rhs_of(b, seed, how="shift", z=0.0):
    return np.concatenate([[z], dc.PERTURB[how](np.asarray(b), seed)])


# ---------------------------------------------------------------------------
# D. k_rhs on windows of more than one workgroup
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("place", ["auto", "device"])       # the 261 x 264 tableau is above a CU's LDS
def test_ragged_windows_across_workgroups(place):
    items = dc.block_problems()
    res = solve_problems_ragged(items, place=place)
    assert res.path == "twophase" and res.status == ["optimal"] * len(items)
    assert (np.asarray(res.rows) == [len(b) for _, _, b, _ in items]).all()
    slacks = [dc.slack_table(s, len(c)) for c, _, _, s in items]
    for k, (first, count) in enumerate(dc.BLOCK_WINDOWS):
        rhs = [rhs_of(b, 10 * k + i, ("shift", "scale")[k % 2], 0.5 * k) for i, (_, _, b, _) in enumerate(items)]
        before, after = dc.assert_set_rhs(res._engine, slacks, rhs[first:first + count], first=first)
        assert any(not dc.same_bits(after["T"][i][:, 0], before["T"][i][:, 0]) for i in range(first, first + count))


@pytest.mark.parametrize("place", ["lds", "device"])
def test_uniform_windows_across_workgroups(place):
    u = dc.UNIFORM_BLOCKS
    T, sense, ns = pc.stack("mixed", u["m"], u["ns"], range(1, u["B"] + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, place=place)
    assert res.path == "plain" and res.status == ["optimal"] * u["B"]
    slack = [dc.slack_table(sense, ns)] * u["B"]
    for k, (first, count) in enumerate(u["windows"]):
        rhs = np.stack([rhs_of(b[i], 100 * k + i, "shift", -1.0 - k) for i in range(u["B"])])
        dc.assert_set_rhs(res._engine, slack, rhs[first:first + count], first=first)


# ---------------------------------------------------------------------------
# E. batches that are not all optimal
# ---------------------------------------------------------------------------

def assert_resolve_rows(new, before, slacks, rhs, nss, cap):
    """resolve against the host loop and the host walk, LP by LP"""
    for i in range(len(new)):
        st, npiv, x, z = dc.host_resolve(before["T"][i], before["basis"][i], slacks[i], rhs[i], cap)
        assert (new.status_code[i], new.npiv[i]) == (st, npiv), i
        assert dc.same_bits(new.x[i], x[:nss[i]]) and dc.same_bits(new.objective[i], z), i
    assert new.path == "dual"


@pytest.mark.parametrize("place", ["lds", "device"])
def test_a_batch_with_an_unbounded_lp(place):
    c, A, b = dc.unbounded_parts()
    B, m, ns = A.shape
    res = solve_problems(c, A, b, log_cap=8, place=place)
    want = ["optimal"] * B
    want[dc.UNBOUNDED_AT] = "unbounded"
    assert res.path == "plain" and res.status == want
    slack = [dc.slack_table([LE] * m, ns)] * B
    rhs = np.stack([rhs_of(b[i], 1 + i, "scale", 0.25) for i in range(B)])
    dc.assert_set_rhs(res._engine, slack, rhs)
    before = dc.snapshot(res._engine)
    b2 = np.stack([dc.shift(b[i], 20 + i) for i in range(B)])
    new = res.resolve(b2)
    cap = 10 * (m + ns + m)
    assert_resolve_rows(new, before, slack, np.concatenate([np.zeros((B, 1)), b2], axis=1), [ns] * B, cap)
    # the unbounded LP keeps a negative cost in row 0: not dual feasible, nothing applied but the new column 0
    u = dc.UNBOUNDED_AT
    assert (new.status[u], new.npiv[u]) == ("bad_arg", 0)
    after = new._engine.download()[u]
    assert dc.same_bits(after[:, 1:], before["T"][u][:, 1:])
    assert dc.same_bits(after[:, 0], dc.set_rhs(before["T"][u], slack[u], np.concatenate([[0.0], b2[u]]))[:, 0])


@pytest.mark.parametrize("place", ["lds", "device"])
def test_a_ragged_batch_with_an_infeasible_lp(place):
    items = dc.infeasible_problems()
    res = solve_problems_ragged(items, log_cap=8, place=place)
    want = ["optimal"] * len(items)
    want[dc.INFEASIBLE_AT] = "infeasible"
    assert res.path == "twophase" and res.status == want
    assert list(res.rows) == [len(b) for _, _, b, _ in items]           # phase 1 ended it with every row live
    slacks = [dc.slack_table(s, len(c)) for c, _, _, s in items]
    nss = [len(c) for c, _, _, _ in items]
    rhs = [rhs_of(b, 3 + i, "shift", 1.0) for i, (_, _, b, _) in enumerate(items)]
    dc.assert_set_rhs(res._engine, slacks, rhs)
    dc.assert_set_rhs(res._engine, slacks, rhs[1:2], first=dc.INFEASIBLE_AT)
    before = dc.snapshot(res._engine)
    b2 = [dc.scale(b, 30 + i) for i, (_, _, b, _) in enumerate(items)]
    new = res.resolve(b2)
    cap = max(10 * (m + n) for m, n in new._engine.shapes)
    assert_resolve_rows(new, before, slacks, [np.concatenate([[0.0], v]) for v in b2], nss, cap)


# ---------------------------------------------------------------------------
# E. the short-row flag: set by a two-phase call, cleared per LP by an upload
# ---------------------------------------------------------------------------

def short_engine(kind):
    """-> (engine with <= senses attached, the LPs, the slack tables)"""
    lps = dc.short_uniform() if kind == "uniform" else dc.short_ragged()
    eng = mc.make_engine(lps, log_cap=16)
    shapes = [dc.shape_of(T) for T in lps]
    senses = [np.full(m, LE, dtype=np.int8) for m, _ in shapes]
    eng.set_senses(senses[0] if kind == "uniform" else senses)
    return eng, lps, [dc.slack_table(s, n - m) for s, (m, n) in zip(senses, shapes)]


def put(eng, T, i):
    eng.upload([T] if isinstance(eng, _lib.RaggedEngine) else T[None], first=i)


def rhs_window(lps, first, count, seed):
    return [rhs_of(T[1:, 0], seed + i, "scale", 0.5) for i, T in enumerate(lps)][first:first + count]


def pack(eng, rhs):
    return rhs if isinstance(eng, _lib.RaggedEngine) else np.stack(rhs)


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
def test_the_short_row_flag_from_set_to_cleared(kind):
    eng, lps, slacks = short_engine(kind)
    s, n = dc.SHORT_AT, len(lps)
    m = dc.shape_of(lps[s])[0]
    refusal = re.escape(f"LP {s}, row {m - 1}: its last two-phase call left {m - 1} of {m} rows live")

    def refused(first, count):
        before = dc.snapshot(eng)
        with pytest.raises(ValueError, match=refusal):
            eng.set_rhs(pack(eng, rhs_window(lps, first, count, 7)), first)
        dc.assert_untouched(dc.snapshot(eng), before, range(n))

    def accepted(first, count, seed):
        dc.assert_set_rhs(eng, slacks, pack(eng, rhs_window(lps, first, count, seed)), first=first)

    try:
        eng.upload(lps)
        status, _, rows, *_ = eng.solve_lp()
        want = [dc.shape_of(T)[0] for T in lps]
        want[s] -= 1
        assert list(rows) == want and (status == _lib.OPTIMAL).all()
        refused(0, n)
        refused(s, 1)
        refused(s - 1, 2)
        accepted(s + 1, n - s - 1, 1)               # the windows without it
        accepted(0, s, 2)
        put(eng, lps[s + 1], s + 1)                 # an upload of another LP leaves the flag
        refused(0, n)
        refused(s, 1)
        put(eng, dc.full_rank(), s)                 # its own upload clears it, before any solve
        accepted(s, 1, 3)
        accepted(0, n, 4)
        put(eng, dc.DEPENDENT, s)                   # and the next two-phase call sets it again
        status, _, rows, *_ = eng.solve_lp()
        assert rows[s] == m - 1
        refused(s, 2)
        eng.upload(lps[:s] + [dc.full_rank()] + lps[s + 1:] if kind == "ragged"
                   else np.concatenate([lps[:s], dc.full_rank()[None], lps[s + 1:]]))
        status, _, rows, *_ = eng.solve_lp()        # a two-phase call that leaves every row live
        assert list(rows) == [dc.shape_of(T)[0] for T in lps] and (status == _lib.OPTIMAL).all()
        accepted(0, n, 5)
        accepted(s, 1, 6)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# E. after lp_phased_solve: the two-phase path with every LP device-placed
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,m,ns,B", [("ge", 8, 10, 32), ("neg", 8, 10, 32), ("ge", 24, 24, 8)])
def test_after_the_device_placed_two_phase_path(kind, m, ns, B):
    T, sense, _ = pc.stack(kind, m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    assert (b < 0).any()                    # rows that phase 1 negates
    res = solve_problems(c, A, b, sense, log_cap=8, place="device")
    assert res.path == "twophase" and res.status == ["optimal"] * B and (res.rows == len(sense)).all()
    assert res._engine.phased_placement(0) == "device"
    slack = [dc.slack_table(sense, ns)] * B
    new_rhs = lambda seed0, how, z: np.stack([rhs_of(b[i], seed0 + i, how, z) for i in range(B)])
    dc.assert_set_rhs(res._engine, slack, new_rhs(1, "shift", -1.5))
    dc.assert_set_rhs(res._engine, slack, new_rhs(50, "scale", 0.0)[1:B - 2], first=1)


def test_the_log_of_a_resolve_after_phase_1_is_the_walk_alone():
    B, m, ns = 16, 8, 10
    T, sense, _ = pc.stack("ge", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, sense, log_cap=dc.LOG_CAP, place="device")
    assert res.path == "twophase" and res.status == ["optimal"] * B and res.ninit.min() >= 1
    slack = dc.slack_table(sense, ns)
    before = dc.snapshot(res._engine)
    assert all(len(log) >= 1 for log in before["log"])              # phase-1 entries are in the log now
    b2 = np.stack([dc.scale(b[i], 1 + i) for i in range(B)])
    new = res.resolve(b2)
    cap = 10 * (len(sense) + new._engine.n)
    pivoted = 0
    for i in range(B):
        w = dc.walk(dc.set_rhs(before["T"][i], slack, np.concatenate([[0.0], b2[i]])), cap)
        assert (new.status_code[i], new.npiv[i]) == (w["status"], w["npiv"]), i
        assert new.log(i).tolist() == w["log"] and new._engine.log(i).tolist() == w["log"], i
        pivoted += w["npiv"] > 0
    assert pivoted >= 2


# ---------------------------------------------------------------------------
# F. non-finite and extreme right-hand sides
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(dc.EXTREME_BATCHES))
def test_extreme_right_hand_sides(which):
    (m, ns), B, place = dc.EXTREME_BATCHES[which]
    T, sense, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, log_cap=dc.LOG_CAP, place=place)
    assert res.path == "plain" and res.status == ["optimal"] * B
    eng = res._engine
    assert eng.placement(0) == place
    slack = dc.slack_table(sense, ns)
    rhs = np.stack([r for _, r in dc.extreme_host(which)])
    assert np.isnan(rhs).any() and np.isinf(rhs).any()
    before, after = dc.assert_set_rhs(eng, [slack] * B, rhs)
    # the stored optimum is the oracle's, so the statuses below are the ones the host test recorded
    assert all(dc.same_bits(before["T"][i], dc.warm(m, ns, 1 + i, "scale")["opt"]) for i in range(B))
    st, done = eng.run(_lib.RULE_DUAL, dc.CAP)
    ran = dc.snapshot(eng)
    for i in range(B):
        w = dc.walk(dc.set_rhs(before["T"][i], slack, rhs[i]))
        assert (int(st[i]), int(done[i]), ran["log"][i]) == (w["status"], w["npiv"], w["log"]), i
        assert dc.same_bits(ran["T"][i], w["T"]), i
        basis = np.array(before["basis"][i])
        for r, col in w["log"]:
            basis[r] = col
        assert np.array_equal(ran["basis"][i], basis), i
    assert [int(s) for s in st] == dc.EXTREME_STATUS[which]
