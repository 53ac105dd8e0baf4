"""lp_cut_extend, extend_into / extend and ProblemResult.add_rows on the GPU
(csrc/batch.hip: k_cut_copy, k_cut_rows, k_cut_basis).

Every comparison is bit for bit with the host statement of tests/_cut_cases.py
(extend(), then _dual_cases.walk); nothing expected comes from the device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _cut_cases as cc
import _dual_cases as dc
import _problem_cases as pc
import _reopt_cases as rc
from lpsol_amd import _lib, solution_x, solve_problems, solve_problems_ragged
from lpsol_amd import generators as gen

pytestmark = pytest.mark.gpu

same_bits = dc.same_bits
CAP, LOG = dc.CAP, dc.LOG_CAP
GROUP = int(re.search(r"define LPK_CUT_GROUP (\d+)",
                      open(os.path.join(ROOT, "linear-program-solver_amd", "csrc", "knobs.h")).read()).group(1))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def shape_of(T):
    return T.shape[0] - 1, T.shape[1] - 1


def source(cases, ragged=False, **kw):
    """an engine that holds the cases' optimal tableaux and bases"""
    kw.setdefault("log_cap", LOG)
    tabs, bases = [c["opt"] for c in cases], [c["basis"] for c in cases]
    if ragged:
        eng = _lib.RaggedEngine([shape_of(t) for t in tabs], **kw)
        eng.upload(tabs)
        eng.set_basis(bases)
    else:
        eng = _lib.BatchEngine(len(tabs), *shape_of(tabs[0]), **kw)
        eng.upload(np.stack(tabs))
        eng.set_basis(np.stack(bases))
    return eng


def destination(cases, ragged=False, **kw):
    kw.setdefault("log_cap", LOG)
    shapes = [shape_of(c["D"]) for c in cases]
    if ragged:
        return _lib.RaggedEngine(shapes, **kw)
    assert len(set(shapes)) == 1
    return _lib.BatchEngine(len(cases), *shapes[0], **kw)


def stated(cases):
    return [c["rows"] for c in cases], [c["sense"] for c in cases]


def state(eng):
    return dict(T=[np.array(t) for t in eng.download()], basis=[np.array(b) for b in eng.get_basis()])


def assert_same_state(a, b, lps=None):
    for i in range(len(a["T"])) if lps is None else lps:
        assert same_bits(a["T"][i], b["T"][i]) and np.array_equal(a["basis"][i], b["basis"][i]), i


def assert_extended(dst, cases, first=0):
    got = state(dst)
    for k, c in enumerate(cases):
        assert same_bits(got["T"][first + k], c["D"]), first + k
        assert np.array_equal(got["basis"][first + k], c["basis2"]), first + k
    return got


def assert_walked(dst, cases, first=0):
    """run(RULE_DUAL) on dst against the host walk of each case's D: status, done, log, x, objective, tableau"""
    status, done = dst.run(_lib.RULE_DUAL, CAP)
    xs, z = dst.solution()
    got = dst.download()
    for k, c in enumerate(cases):
        i = first + k
        w = dc.walk(c["D"], CAP)
        assert (status[i], done[i]) == (w["status"], w["npiv"]), i
        assert dst.log(i).tolist() == w["log"][:LOG], i
        assert same_bits(got[i], w["T"]), i
        x = solution_x(w["T"], rc.basis_of(c["basis2"], w["log"]))
        assert same_bits(np.asarray(xs[i]), x) and same_bits(z[i], -w["T"][0, 0]), i
    return status


# ---------------------------------------------------------------------------
# uniform -> uniform
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("workload", cc.WORKLOADS)
def test_uniform_to_uniform_is_the_host_loop_and_the_host_walk(workload):
    cases = [cc.case(*cc.SMALL, s, workload) for s in cc.SEEDS[cc.SMALL]]
    src, dst = source(cases), destination(cases)
    before = state(src)
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    assert_same_state(state(src), before)                   # the source is not changed
    status = assert_walked(dst, cases)
    assert np.count_nonzero(status == _lib.OPTIMAL) == (64 if workload == "le" else 40)
    assert np.count_nonzero(status == _lib.INFEASIBLE) == (0 if workload == "le" else 24)
    assert_same_state(state(src), before)
    # the thin call on the kept destination once more: its LPs are as uploaded again
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    assert_walked(dst, cases)


def test_a_window_across_several_workgroups_leaves_the_rest_alone():
    B, first, count = 300, 37, 200
    cases = [cc.case(*cc.SMALL, 1 + i % 64, "lege") for i in range(B)]
    src, dst = source(cases), destination(cases)
    fill = np.stack([np.full(c["D"].shape, 1.0 + i) for i, c in enumerate(cases)])
    dst.upload(fill)
    window = cases[first:first + count]
    src.extend_into(dst, *stated(window), first=first)
    got = assert_extended(dst, window, first)
    outside = [i for i in range(B) if not first <= i < first + count]
    for i in outside:
        assert same_bits(got["T"][i], fill[i]), i
        assert (got["basis"][i] == -1).all(), i             # none was attached: as lp_solution_canonical has it
    # count 0 is a no-op, at the end of the batch too
    src.extend_into(dst, [], [], first=B)
    src.extend_into(dst, [], [], first=3)
    assert_same_state(state(dst), got)
    # a second window with the basis attached: the first one's entries stay
    src.extend_into(dst, *stated(cases[:5]), first=0)
    now = assert_extended(dst, cases[:5], 0)
    assert_same_state(now, got, range(5, B))
    assert_walked(dst, window[:40], first)


# ---------------------------------------------------------------------------
# ragged on either side
# ---------------------------------------------------------------------------

def test_uniform_to_ragged_and_ragged_to_ragged():
    uni = [cc.case(*cc.SMALL, 1 + i, "lege", cc.Q_CYCLE[i % 3]) for i in range(9)]
    for cases, ragged_src in ((uni, False), (cc.ragged_cases(), True)):
        assert {c["rows"].shape[0] for c in cases} == {0, 1, 3}
        src, dst = source(cases, ragged_src), destination(cases, True)
        before = state(src)
        src.extend_into(dst, *stated(cases))
        assert_extended(dst, cases)
        assert_walked(dst, cases)
        assert_same_state(state(src), before)
        # a window that begins and ends inside the batch
        dst2 = destination(cases, True)
        src.extend_into(dst2, *stated(cases[2:7]), first=2)
        got = assert_extended(dst2, cases[2:7], 2)
        assert all((got["basis"][i] == -1).all() and not got["T"][i].any() for i in (0, 1, 7, 8))
    # q = 0 leaves the walk nothing to do: the LP was optimal
    assert all(dc.walk(c["D"], CAP)["npiv"] == 0 for c in uni if c["rows"].shape[0] == 0)


def test_ragged_to_uniform():
    cases = [cc.case(8, 10, 1, "lege", 3), cc.case(10, 10, 2, "lege", 1), cc.case(11, 10, 3, "le", 0),
             cc.case(8, 10, 4, "le", 3)]
    assert {shape_of(c["D"]) for c in cases} == {(11, 21)}
    src, dst = source(cases, True), destination(cases)
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    assert_walked(dst, cases)


# ---------------------------------------------------------------------------
# placements, teams, group edges
# ---------------------------------------------------------------------------

def test_a_device_placed_destination_holds_the_same_bits():
    cases = [cc.case(*cc.MID, s, "lege") for s in cc.SEEDS[cc.MID]]
    src = source(cases)
    for place in ("lds", "device"):
        dst = destination(cases, place=place)
        assert dst.placement(0) == place
        src.extend_into(dst, *stated(cases))
        assert_extended(dst, cases)
        assert_walked(dst, cases)


def test_a_teamed_source_after_a_solve():
    m, ns = cc.LARGE
    cases = [cc.case(m, ns, s, "le") for s in range(1, 5)]
    src = _lib.BatchEngine(4, m, ns + m, log_cap=LOG, place="device", team=2)
    assert src.team_of(0) == 2
    src.upload(np.stack([c["T0"] for c in cases]))
    src.derive_basis()
    status, _, _ = src.solve()
    assert (status == _lib.OPTIMAL).all()
    held = state(src)
    for c, T, b in zip(cases, held["T"], held["basis"]):    # the teamed solve ends where the oracle's does
        assert same_bits(T, c["opt"]) and np.array_equal(b, c["basis"])
    dst = destination(cases, place="device")
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    assert_walked(dst, cases)
    assert_same_state(state(src), held)


def test_one_row_more_than_a_group():
    q = GROUP + 1
    cases = [cc.case(*cc.SMALL, s, "lege", q) for s in range(1, 9)]
    assert all(c["rows"].shape[0] == q for c in cases) and GROUP >= 1
    src, dst = source(cases), destination(cases)
    src.extend_into(dst, *stated(cases))
    assert_extended(dst, cases)
    assert_walked(dst, cases)
    # and exactly a group, and a single row
    for q in sorted({GROUP, 1}):
        cases = [cc.case(*cc.SMALL, s, "lege", q) for s in range(1, 9)]
        dst = destination(cases)
        src.extend_into(dst, *stated(cases))
        assert_extended(dst, cases)


# ---------------------------------------------------------------------------
# non-finite and signed-zero cells
# ---------------------------------------------------------------------------

def test_non_finite_cells_and_skipped_basis_entries():
    T, basis, rows, sense = cc.odd_case()
    want, wbasis = cc.extend(T, basis, rows, sense)
    src = _lib.BatchEngine(2, 3, 4)
    src.upload(np.stack([T, T]))
    src.set_basis(np.stack([basis, basis]))
    dst = _lib.BatchEngine(2, 6, 7)
    src.extend_into(dst, [rows, rows], sense)
    got = state(dst)
    nan = np.isnan(want)
    assert nan[4:, :5].any() and np.isinf(want[4:, :5]).any()
    for i in range(2):
        D = got["T"][i]
        assert same_bits(D[:4, :5], T)                      # the copied NaN, inf and -0.0 keep their bits
        assert np.array_equal(np.isnan(D), nan) and same_bits(D[~nan], want[~nan])
        assert D[5, 0] == 0.0 and np.signbit(D[5, 0])       # a >= cut whose priced cell is +0.0 stores -0.0
        assert np.array_equal(got["basis"][i], wbasis)


# ---------------------------------------------------------------------------
# forms
# ---------------------------------------------------------------------------

def test_a_two_phase_source_with_an_equality_row():
    blocks = [pc.mixed_sense_block(s) for s in range(1, 9)]
    P, sense = np.stack([p for p, _ in blocks]), blocks[0][1]
    res = solve_problems(P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0], sense, log_cap=LOG)
    assert res.path == "twophase" and (res.rows == 5).all() and (sense == pc.EQ).any()
    ok = [i for i in range(8) if res.status[i] == "optimal"]
    assert ok
    src = res._engine
    held = state(src)
    n, ns = src.n, res.ns
    rows, senses = [], np.array([cc.LE, cc.GE], dtype=np.int8)
    for i in range(8):
        a = np.stack([cc.coefficients(50 + i, k, ns) for k in range(2)])
        ax = [cc.dot(a[k], res.x[i]) for k in range(2)]
        rows.append(cc.stated(a, [np.floor(48 * ax[0]) / 64, np.ceil(64 * ax[1]) / 64 + 0.125], n))
    new = src.extend(rows, senses)
    got = state(new)
    for i in range(8):
        D, b2 = cc.extend(held["T"][i], held["basis"][i], rows[i], senses)
        assert same_bits(got["T"][i], D) and np.array_equal(got["basis"][i], b2), i
    y = new.duals()
    eq = np.nonzero(sense == pc.EQ)[0]
    assert np.isnan(y[:, eq]).all() and y.shape == (8, 7)
    status, done = new.run(_lib.RULE_DUAL, CAP)
    for i in ok:
        w = dc.walk(got["T"][i], CAP)
        assert (status[i], done[i]) == (w["status"], w["npiv"]), i
    y = new.duals()
    assert np.isnan(y[:, eq]).all() and np.isfinite(y[ok][:, 5:]).all()
    assert_same_state(state(src), held)


def test_a_source_with_dropped_rows_is_refused():
    P, s = pc.dependent_block(3)
    P2, _ = pc.dependent_block(4)
    short = solve_problems(np.stack([P[0, 1:], P2[0, 1:]]), np.stack([P[1:, 1:], P2[1:, 1:]]),
                           np.stack([P[1:, 0], P2[1:, 0]]), s, log_cap=4)
    assert (short.rows < len(s)).all()
    src = short._engine
    dst = _lib.BatchEngine(2, src.m + 1, src.n + 1)
    before = dst.download()
    with pytest.raises(ValueError, match=r"LP 0, row 3: its last two-phase call left 3 of 4 rows live"):
        src.extend_into(dst, np.zeros((2, 1, src.n + 1)), ["<="])
    with pytest.raises(ValueError, match=r"LP 1, row 3"):
        src.extend_into(dst, np.zeros((1, 1, src.n + 1)), ["<="], first=1)
    assert same_bits(dst.download(), before)
    with pytest.raises(ValueError, match="phase 1 left 3 of its 4 rows"):
        short.add_rows(np.zeros((2, 1, short.ns)), np.zeros((2, 1)))


# ---------------------------------------------------------------------------
# every refusal leaves the destination as it was
# ---------------------------------------------------------------------------

def test_refusals_change_nothing():
    cases = [cc.case(*cc.SMALL, s, "lege") for s in range(1, 5)]
    src, dst = source(cases), destination(cases)
    src.extend_into(dst, *stated(cases))
    before = state(dst)
    lib, rows, sense = src.lib, np.ascontiguousarray(np.stack([c["rows"] for c in cases])), cases[0]["sense"]
    flat = np.ascontiguousarray(np.tile(sense, 4), dtype=np.int8)
    pr_, ps = _lib._ptr(rows), flat.ctypes.data_as(_lib._P8)

    def refused(match, s=src, d=dst, first=0, count=4, r=pr_, sn=ps):
        assert lib.lp_cut_extend(s.h if s else None, d.h if d else None, first, count, r, sn) == _lib.BAD_ARG
        if d:
            assert re.search(match, d._err(d.h)), d._err(d.h)
        assert_same_state(state(dst), before)

    refused("", d=None)
    refused("source batch is NULL", s=None)
    refused("one batch", s=dst)
    other = _lib.BatchEngine(3, *shape_of(cases[0]["D"]))
    refused("4 LPs, the destination 3", d=other)
    for first, count in ((-1, 1), (4, 1), (2, 3), (5, 0)):
        refused("out of bounds", first=first, count=count)
    refused("rows or sense is NULL", r=None)
    refused("rows or sense is NULL", sn=None)
    wrong = _lib.RaggedEngine([(10, 20), (10, 21), (7, 17), (10, 20)])
    refused(r"LP 1: the destination's 10 x 21 is not the source's 8 x 18", d=wrong)
    refused(r"LP 2: the destination's 7 x 17", d=wrong, first=2, count=1)
    for bad, what in ((_lib.SENSE_EQ, "an equality owns no column"), (3, "sense 3 is not"), (-1, "sense -1 is not")):
        odd = flat.copy()
        odd[5] = bad
        refused(r"LP 2, row 1 of its new rows: " + what, sn=odd.ctypes.data_as(_lib._P8))
    src.set_basis(None)
    refused("no basis attached to the source")
    src.set_basis(np.stack([c["basis"] for c in cases]))
    # senses on the destination that disagree with the call, or with the source's
    m = cc.SMALL[0]
    dst.set_senses(["<="] * m + ["<=", "<="])
    refused(r"LP 0, row 9: .* the sense of this call")
    dst.set_senses(["<="] * m + ["<=", ">="])
    src.set_senses([">="] + ["<="] * (m - 1))
    refused(r"LP 0, row 0: .* the source's senses")
    src.set_senses(["<="] * m)
    src.extend_into(dst, *stated(cases))                    # and with senses that agree it goes through
    assert_extended(dst, cases)
    src.extend_into(dst, *stated(cases[1:3]), first=1)
    # the Python layer's own checks
    with pytest.raises(ValueError, match="out of bounds"):
        src.extend_into(dst, rows, sense, first=1)
    with pytest.raises(ValueError, match="must be"):
        src.extend_into(dst, rows[:, :, :5], sense)
    with pytest.raises(ValueError, match="2 more rows"):
        src.extend_into(dst, rows[:, :1], sense[:1])
    assert_extended(dst, cases)


# ---------------------------------------------------------------------------
# add_rows end to end
# ---------------------------------------------------------------------------

def problem_cuts(cases):
    return (np.stack([c["a"] for c in cases]), np.stack([c["beta"] for c in cases]), cases[0]["sense"])


def assert_result(new, cases, wants):
    """a result against per-LP host answers (status, npiv, x of all columns, objective)"""
    for i, (c, (st, npiv, x, z)) in enumerate(zip(cases, wants)):
        ns = c["a"].shape[1]
        assert (new.status_code[i], new.npiv[i]) == (st, npiv), i
        assert same_bits(np.asarray(new.x[i]), x[:ns]) and same_bits(new.objective[i], z), i
    assert new.path == "dual" and not new.ninit.any() and not new.stage.any() and not new.nstd.any()


@pytest.mark.parametrize("workload", cc.WORKLOADS)
def test_add_rows_is_the_host_composition_and_the_old_result_stays_live(workload):
    m, ns = cc.SMALL
    cases = [cc.case(m, ns, s, workload) for s in range(1, 33)]
    T0 = np.stack([c["T0"] for c in cases])
    c_, A, b = pc.parts(T0, ns)
    res = solve_problems(c_, A, b, log_cap=LOG)
    assert res.path == "plain" and all(same_bits(t, c["opt"]) for t, c in zip(res._engine.download(), cases))
    new = res.add_rows(*problem_cuts(cases))
    assert_result(new, cases, [cc.warm_answer(c) for c in cases])
    assert new._engine is not res._engine and len(new.sense) == m + 2 and (new.rows == m + 2).all()
    assert same_bits(new._host["b"], np.concatenate([b, np.stack([c["beta"] for c in cases])], axis=1))
    assert [new.log(i).tolist() for i in range(4)] == [c["warm"]["log"] for c in cases[:4]]
    # the old result answers as before
    assert same_bits(res.tableau(3).toArray(), cases[3]["opt"]) and res.y.shape == (32, m)
    again = res.resolve(b)
    assert again.status == ["optimal"] * 32 and not again.npiv.any()
    # y of the new result: finite where the LP ended optimal, one entry per joined row
    ok = [i for i in range(32) if new.status[i] == "optimal"]
    assert new.y.shape == (32, m + 2) and np.isfinite(new.y[ok]).all()
    # chains: resolve with m + q right-hand sides, reoptimize(c=), add_rows once more
    finals = [dc.walk(c["D"], c["cap"]) for c in cases]
    bases = [rc.basis_of(c["basis2"], w["log"]) for c, w in zip(cases, finals)]
    slack = dc.slack_table(cases[0]["joined"], ns)
    b2 = np.concatenate([b, np.stack([c["beta"] for c in cases])], axis=1) + 0.125
    third = new.add_rows(*problem_cuts([cc.case(m, ns, 40 + s, "le") for s in range(1, 33)]))
    wants = []
    for c, w, bs, extra in zip(cases, finals, bases, [cc.case(m, ns, 40 + s, "le") for s in range(1, 33)]):
        rows = cc.stated(extra["a"], extra["beta"], w["T"].shape[1] - 1)
        D, bs2 = cc.extend(w["T"], bs, rows, extra["sense"])
        ww = dc.walk(D, 10 * (D.shape[0] + D.shape[1] - 2))
        wants.append((ww["status"], ww["npiv"], solution_x(ww["T"], rc.basis_of(bs2, ww["log"])), -ww["T"][0, 0]))
    assert_result(third, cases, wants)
    assert (third.rows == m + 4).all() and third._engine.n == ns + m + 4
    warm = new.resolve(b2)
    cap = 10 * (m + 2 + ns + m + 2)
    assert_result(warm, cases, [dc.host_resolve(w["T"], bs, slack, np.concatenate([[0.0], b2[i]]), cap)
                                for i, (w, bs) in enumerate(zip(finals, bases))])


def test_add_rows_then_new_costs():
    m, ns = cc.SMALL
    cases = [cc.case(m, ns, s, "le") for s in range(1, 17)]
    T0 = np.stack([c["T0"] for c in cases])
    c_, A, b = pc.parts(T0, ns)
    new = solve_problems(c_, A, b, log_cap=LOG).add_rows(*problem_cuts(cases))
    assert new.status == ["optimal"] * 16
    c2 = np.stack([rc.tilt(c_[i], 1 + i) for i in range(16)])
    got = new.reoptimize(c=c2)
    for i, c in enumerate(cases):
        w = c["warm"]
        row = np.concatenate([[0.0], c2[i], np.zeros(m + 2)])
        st, npiv, nstd, _, x, z, _ = rc.host_primal(w["T"], rc.basis_of(c["basis2"], w["log"]), row)
        assert (got.status_code[i], got.npiv[i], got.nstd[i]) == (st, npiv, nstd), i
        assert same_bits(got.x[i], x[:ns]) and same_bits(got.objective[i], z), i


def test_add_rows_on_a_ragged_result():
    cases = cc.ragged_cases()
    items = [(*pc.parts(c["T0"], c["a"].shape[1]), None) for c in cases]
    res = solve_problems_ragged(items, log_cap=LOG)
    assert res.status == ["optimal"] * len(cases)
    new = res.add_rows([c["a"] for c in cases], [c["beta"] for c in cases], [c["sense"] for c in cases])
    assert_result(new, cases, [(lambda w, c: (w["status"], w["npiv"],
                                              solution_x(w["T"], rc.basis_of(c["basis2"], w["log"])), -w["T"][0, 0]))(
                                                  dc.walk(c["D"], max(x["cap"] for x in cases)), c) for c in cases])
    assert [len(s) for s in new.sense] == [c["D"].shape[0] - 1 for c in cases]
    assert same_bits(res.tableau(1).toArray(), cases[1]["opt"])
    assert [len(y) for y in new.y] == [len(s) for s in new.sense]
