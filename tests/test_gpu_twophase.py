"""Batched two-phase solve on the GPU (lp_twophase_solve, csrc/batch.hip
k_twophase): every LP of a batch against oracle/phase1.py's solve_lp, LP by LP.
Every comparison is exact: == on integers, byte equality on tableaux and
objectives.  Shapes are the smallest that reach each path: one wave and four,
the skip path, drive-out pivots, dropped rows, an infeasible LP, the cap in
either solve, a relaunch at every pivot."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import fixture_input, load_golden

from lpsol_amd import Simplex, Tableau, _lib, solve_lp_batch
from lpsol_amd import generators as gen
from oracle import phase1
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu

SMALL = load_golden("small.json")
REL = 1e-9
LOG_CAP = 512


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


# ------------------------------------------------------------------ oracle
class _Spy(F64Tableau):
    """F64Tableau that counts what find_bfs / solve_lp do with it: the direct
    pivots (the drive-outs) and each solve's (status, pivots, nstd)"""
    seen = None

    def pivot(self, r, c):
        _Spy.seen["drive"] += 1
        return super().pivot(r, c)

    def solve(self, *a, **k):
        out = super().solve(*a, **k)
        _Spy.seen["solves"].append((int(out[0]), len(out[1]), int(out[2])))
        return out


_ORACLE = {}


def _tolkey(tol):
    return tuple(sorted((tol or {}).items()))


def oracle(T, tol=None):
    """phase1.solve_lp(T, tol), computed once per input, plus "drive" (number of
    drive-out pivots) and "nstd" (standard-rule pivots of phase 2)."""
    key = (T.shape, T.tobytes(), _tolkey(tol))
    if key not in _ORACLE:
        _Spy.seen = {"drive": 0, "solves": []}
        real = phase1.F64Tableau
        phase1.F64Tableau = _Spy
        try:
            o = phase1.solve_lp(T, tol)
        finally:
            phase1.F64Tableau = real
        o["drive"] = _Spy.seen["drive"]
        if "error" not in o:
            o["nstd"] = _Spy.seen["solves"][-1][2]
        _ORACLE[key] = o
    return _ORACLE[key]


# ------------------------------------------------------------------ device
def run(stack, tol=None, max_pivots=-1, chunk=None, eng=None):
    stack = np.ascontiguousarray(stack)
    B, m, n = stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1
    own = eng is None
    if own:
        eng = _lib.BatchEngine(B, m, n, log_cap=LOG_CAP)
    try:
        if tol:
            eng.set_tol(**tol)
        if chunk:
            eng.set_chunk(chunk)
        eng.upload(stack)
        status, stage, rows, ninit, npiv, nstd = eng.solve_lp(max_pivots)
        return dict(status=status.tolist(), stage=stage.tolist(), rows=rows.tolist(),
                    ninit=ninit.tolist(), npiv=npiv.tolist(), nstd=nstd.tolist(),
                    T=eng.download(), z=eng.objective(), basis=eng.get_basis().tolist(),
                    log=[eng.log(i).tolist() for i in range(B)])
    finally:
        if own:
            eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_lp(res, i, T, o, where=""):
    """LP i of a device result against the oracle's solve_lp of T"""
    w = f"{where} LP {i}"
    m = T.shape[0] - 1
    if "error" in o:
        assert o["error"] == "ValueError"
        assert (res["status"][i], res["stage"][i]) == (_lib.INFEASIBLE, _lib.STAGE_ARTIFICIAL), w
        assert res["log"][i] == o["init_seq"], w
        assert res["ninit"][i] == len(o["init_seq"]) and res["npiv"][i] == 0 and res["nstd"][i] == 0, w
        assert np.array_equal(bits(res["T"][i]), bits(T)), w       # untouched
        return
    assert (res["status"][i], res["stage"][i]) == (_lib.OPTIMAL, _lib.STAGE_PHASE2), w
    mp = o["init_size"][0]
    assert res["rows"][i] == mp, w
    assert res["ninit"][i] == len(o["init_seq"]), w
    assert res["npiv"][i] == len(o["seq"]), w
    assert res["nstd"][i] == o["nstd"], w
    assert res["log"][i][:res["ninit"][i]] == o["init_seq"], w
    assert res["log"][i][res["ninit"][i]:] == o["seq"], w
    assert res["basis"][i][:mp] == o["bfs"], w
    assert res["basis"][i][mp:] == [-1] * (m - mp), w
    assert np.array_equal(bits(res["T"][i][:mp + 1]), bits(o["T"])), w
    assert not bits(res["T"][i][mp + 1:]).any(), w                 # +0.0, every bit
    assert bits(res["z"][i:i + 1])[0] == bits(np.array([o["objective"]]))[0], w


def check_batch(res, stack, tol=None, where=""):
    for i in range(len(stack)):
        check_lp(res, i, stack[i], oracle(stack[i], tol), where)


# ------------------------------------------------------------------ batches
def batch1():
    """arrays of 7x13 (m = 6, n = 12; one wave): neg and ge LPs, and LPs that are canonical already"""
    lps = [gen.phase1_lp("neg", 5, 6, s) for s in range(1, 9)]
    lps += [gen.phase1_lp("ge", 5, 6, s) for s in range(1, 9)]
    lps += [gen.tableau("mixed", 6, 6, s) for s in (1, 2)]
    return np.stack(lps)


SEEDS2 = (1, 2, 48, 228)


def batch2():
    """arrays of 7x9 (m = 6, n = 8; one wave): equality rows; dep repeats a row, so one is dropped"""
    return np.stack([gen.phase1_lp("eq", 5, 8, s) for s in SEEDS2] +
                    [gen.phase1_lp("dep", 4, 8, s) for s in SEEDS2])


def degenerate(seed, ones):
    """eq(30, 72, seed) with b = A x1, x1 = 1 on the first `ones` coordinates
    (dyadic, exact): a degenerate vertex, so artificials stay basic at 0"""
    T = gen.phase1_lp("eq", 30, 72, seed)
    x1 = np.zeros(72)
    x1[:ones] = 1.0
    T[1:, 0] = T[1:, 1:] @ x1
    return T


def test_one_wave_mixed_kinds_and_the_skip_path():
    stack = batch1()
    assert stack.shape == (18, 7, 13) and _lib.twophase_waves(6, 12) == 1
    # coverage that must not go away: LPs without phase 1, LPs with one
    skip = [i for i in range(18) if not oracle(stack[i])["init_seq"]]
    assert {7, 16, 17} <= set(skip) and len(skip) < 10
    assert any((stack[i][1:, 0] < 0).any() for i in range(8))
    res = run(stack)
    check_batch(res, stack, where="batch1")
    for i in skip:
        assert res["ninit"][i] == 0 and res["rows"][i] == 6


def test_equality_rows_dropped_rows_and_drive_out_pivots():
    stack = batch2()
    assert stack.shape == (8, 7, 9)
    drive = [oracle(t)["drive"] for t in stack]
    # the oracle's init_seq is longer than its artificial solve for these seeds
    assert drive[:4] == [1, 0, 1, 2]                # eq 1, 48: one drive-out pivot; 228: two
    assert drive[6] >= 1 and drive[7] >= 1          # dep 48, 228 pivot an artificial out
    assert all(oracle(t)["init_size"][0] == 5 for t in stack[4:])     # every dep LP drops one row
    assert all(oracle(t)["init_size"][0] == 6 for t in stack[:4])
    res = run(stack)
    check_batch(res, stack, where="batch2")


def test_infeasible_among_feasible():
    inf = gen.phase1_lp("infeasible", 2, 8, 1)
    stack = np.stack([gen.phase1_lp("eq", 1, 8, 1), inf, gen.phase1_lp("eq", 1, 8, 2),
                      gen.phase1_lp("eq", 1, 8, 3)])
    assert stack.shape == (4, 3, 9)
    o = oracle(inf)
    assert o.get("error") == "ValueError" and o["init_seq"] == [[0, 0]]
    res = run(stack)
    check_batch(res, stack, where="infeasible")
    assert (res["status"][1], res["stage"][1]) == (_lib.INFEASIBLE, _lib.STAGE_ARTIFICIAL)
    assert res["log"][1] == [[0, 0]]
    assert np.array_equal(bits(res["T"][1]), bits(inf))


def test_four_waves_equalities_and_dropped_rows():
    stack = np.stack([gen.phase1_lp("eq", 30, 72, s) for s in range(1, 5)] +
                     [gen.phase1_lp("dep", 29, 72, s) for s in range(1, 5)])
    assert stack.shape == (8, 32, 73) and _lib.twophase_waves(31, 72) == 4
    assert all(oracle(t)["init_size"][0] == 30 for t in stack[4:])
    check_batch(run(stack), stack, where="4w eq/dep")


def test_four_waves_inequalities_and_negative_b():
    stack = np.stack([gen.phase1_lp("ge", 32, 32, s) for s in range(1, 4)] +
                     [gen.phase1_lp("neg", 32, 32, s) for s in range(1, 4)] +
                     [gen.tableau("mixed", 33, 32, 1)])
    assert stack.shape == (7, 34, 66) and _lib.twophase_waves(33, 65) == 4
    assert oracle(stack[6])["init_seq"] == []
    check_batch(run(stack), stack, where="4w ge/neg")


def test_four_waves_drive_out_at_a_degenerate_vertex():
    stack = np.stack([degenerate(s, 16) for s in range(1, 9)])
    drive = [oracle(t)["drive"] for t in stack]
    assert (drive[1], drive[3], drive[5]) == (3, 2, 2)
    na = [len(oracle(t)["init_seq"]) - d for t, d in zip(stack, drive)]
    assert min(na) >= 40                            # long artificial solves: the stall logic runs
    check_batch(run(stack), stack, where="4w degenerate")


def test_results_do_not_depend_on_the_chunk():
    """a relaunch at every pivot (chunk 1) passes through every stage
    transition with the state in global memory"""
    stack = batch2()
    want = run(stack)
    check_batch(want, stack, where="default chunk")
    for chunk in (1, 3):
        got = run(stack, chunk=chunk)
        for k, v in want.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(bits(got[k]), bits(v)), (chunk, k)
            else:
                assert got[k] == v, (chunk, k)


def test_cap_applies_to_each_solve_separately():
    stack = batch1()
    os_ = [oracle(t) for t in stack]
    na = [len(o["init_seq"]) - o["drive"] for o in os_]
    n2 = [len(o["seq"]) for o in os_]
    K = sorted(na + n2)[len(na + n2) // 2]          # a middle value of the per-solve counts
    art = [i for i in range(len(stack)) if na[i] >= K]
    ph2 = [i for i in range(len(stack)) if na[i] < K <= n2[i]]
    free = [i for i in range(len(stack)) if na[i] < K and n2[i] < K]
    assert K > 0 and art and ph2 and free, (K, na, n2)
    res = run(stack, max_pivots=K)
    for i in free:
        check_lp(res, i, stack[i], os_[i], "cap, uncapped")
    for i in art:
        assert (res["status"][i], res["stage"][i]) == (_lib.CAP_REACHED, _lib.STAGE_ARTIFICIAL), i
        assert res["log"][i] == os_[i]["init_seq"][:K], i
        assert (res["ninit"][i], res["npiv"][i]) == (K, 0), i
        assert np.array_equal(bits(res["T"][i]), bits(stack[i])), i
    for i in ph2:
        assert (res["status"][i], res["stage"][i]) == (_lib.CAP_REACHED, _lib.STAGE_PHASE2), i
        assert res["log"][i] == os_[i]["init_seq"] + os_[i]["seq"][:K], i
        assert (res["ninit"][i], res["npiv"][i]) == (len(os_[i]["init_seq"]), K), i


def test_tolerances_reach_every_stage():
    tol = dict(zero=1e-7, pivot=1e-7)
    stack = batch2()
    check_batch(run(stack, tol=tol), stack, tol=tol, where="tol")


class _Capped(F64Tableau):
    """F64Tableau whose solve takes a given cap and keeps its (status, log)"""
    cap, kept = 0, None

    def solve(self, *a, **k):
        out = super().solve(_Capped.cap)
        _Capped.kept.append((int(out[0]), out[1].tolist()))
        return out


CYCLE_CAP = 400


def test_the_oracles_artificial_assertion_is_reported_not_asserted():
    """The oracle's 'unbounded artificial problem' assertion on the degenerate
    eq(30, 72, 5) with 8 ones.  Its artificial solve does not end 'unbounded':
    the standard rule cycles away from the starting objective, the stall switch
    (which compares with the objective at the START of the solve) never fires,
    and lpf_solve stops at the oracle wrapper's built-in 2^20-pivot log limit
    with LP_CAP_REACHED after 1048576 standard-rule pivots.  Without a cap the
    device solve of this LP does not end either, as Simplex.solve itself would
    not.  So the batch runs under a cap above everything its neighbours need:
    the LP reports (LP_CAP_REACHED, LP_STAGE_ARTIFICIAL) with the oracle's first
    CYCLE_CAP pivots, stays as uploaded, and the neighbours equal the oracle."""
    bad = degenerate(5, 8)
    with pytest.raises(AssertionError, match="unbounded artificial problem"):
        phase1.solve_lp(bad)
    _Capped.cap, _Capped.kept = CYCLE_CAP, []
    real = phase1.F64Tableau
    phase1.F64Tableau = _Capped
    try:
        with pytest.raises(AssertionError, match="unbounded artificial problem"):
            phase1.solve_lp(bad)
    finally:
        phase1.F64Tableau = real
    (st, log), = _Capped.kept
    assert st == _lib.CAP_REACHED and len(log) == CYCLE_CAP <= LOG_CAP
    good = [degenerate(s, 8) for s in range(1, 5)]
    stack = np.stack(good[:2] + [bad] + good[2:])
    for i in (0, 1, 3, 4):                      # the cap binds on none of the neighbours
        o = oracle(stack[i])
        assert len(o["init_seq"]) < CYCLE_CAP and len(o["seq"]) < CYCLE_CAP and o["drive"] >= 5
    res = run(stack, max_pivots=CYCLE_CAP)
    assert (res["status"][2], res["stage"][2]) == (_lib.CAP_REACHED, _lib.STAGE_ARTIFICIAL)
    assert (res["ninit"][2], res["npiv"][2], res["rows"][2]) == (CYCLE_CAP, 0, 31)
    assert res["log"][2] == log
    assert np.array_equal(bits(res["T"][2]), bits(bad))
    for i in (0, 1, 3, 4):
        check_lp(res, i, stack[i], oracle(stack[i]), "next to the cycling one")


class _LogSimplex(Simplex):
    def __init__(self, tab, log):
        self._plog = log
        super().__init__(tab)

    def _mark(self, r, c):
        self._plog.append([int(r), int(c)])
        super()._mark(r, c)


ONE_LP = {"p1_eq_6x8_s1", "p1_ge_10x12_s2", "p1_dep_6x8_s1"}


@pytest.mark.parametrize("fx", SMALL["phase1"], ids=[fx["name"] for fx in SMALL["phase1"]])
def test_goldens_as_batches_of_one(fx):
    """the reference's own pivots, sizes, bases and objective through
    solve_lp_batch.  init_bfs is compared on the rows phase 2 does not touch,
    and phase 2's pivots replayed over it give the final basis."""
    T = fixture_input(fx)
    r = solve_lp_batch(T[None], log_cap=LOG_CAP)
    init, seq = r.init_log(0).tolist(), r.log(0).tolist()
    if fx.get("error") == "ValueError":
        assert r.status == ["infeasible"] and r.stage[0] == _lib.STAGE_ARTIFICIAL
        assert init == fx["init_seq"] and seq == []
        return
    assert r.status == ["optimal"] and r.stage[0] == _lib.STAGE_PHASE2
    assert init == fx["init_seq"]
    if fx.get("error") == "IndexError":                 # the reference stops there; a row is dropped
        assert r.rows[0] == fx["m"] - 1
        twin = next(f for f in SMALL["phase1"] if f.get("phase1") == dict(fx["phase1"], kind="eq"))
        obj = float(Fraction(twin["objective"]))
    else:
        assert [int(r.rows[0]), T.shape[1] - 1] == fx["init_size"]
        assert seq == fx["seq"]
        basis = r.basis[0][:r.rows[0]].tolist()
        assert basis == fx["bfs"]
        touched = {p[0] for p in seq}
        assert all(basis[i] == c for i, c in enumerate(fx["init_bfs"]) if i not in touched)
        replay = list(fx["init_bfs"])
        for i, c in seq:
            replay[i] = c
        assert replay == basis
        obj = float(Fraction(fx["objective"]))
    assert abs(r.objective[0] - obj) <= REL * max(1.0, abs(obj))
    assert r.tableau(0).getTableauSize() == (int(r.rows[0]), T.shape[1] - 1)
    if fx["name"] in ONE_LP:                            # and the one-LP front-end on the same LP
        log = []
        t = Tableau.fromArray(T)
        s = _LogSimplex(t, log)
        ninit = len(log)
        s.solve()
        assert log[:ninit] == init and log[ninit:] == seq
        assert list(t.getTableauSize()) == [int(r.rows[0]), T.shape[1] - 1]
        assert list(s.getBasicSequence()) == r.basis[0][:r.rows[0]].tolist()


def test_one_lp_fixtures_exist():
    assert ONE_LP <= {fx["name"] for fx in SMALL["phase1"]}


def test_a_two_phase_call_leaves_the_batch_usable():
    stack = batch1()
    mixed = np.stack([gen.tableau("mixed", 6, 6, s) for s in range(1, 19)])
    assert mixed.shape == stack.shape
    eng = _lib.BatchEngine(len(stack), 6, 12, log_cap=LOG_CAP)
    fresh = _lib.BatchEngine(len(stack), 6, 12, log_cap=LOG_CAP)
    try:
        check_batch(run(stack, eng=eng), stack, where="before")
        eng.upload(mixed)
        fresh.upload(mixed)
        got, want = eng.solve(), fresh.solve()
        for a, b in zip(got, want):
            assert a.tolist() == b.tolist()
        assert np.array_equal(bits(eng.download()), bits(fresh.download()))
        assert np.array_equal(bits(eng.objective()), bits(fresh.objective()))
        for i in range(len(stack)):
            assert eng.log(i).tolist() == fresh.log(i).tolist()
        # and a second two-phase call on the same handle
        check_batch(run(stack, eng=eng), stack, where="after")
    finally:
        eng.close()
        fresh.close()


def test_a_widened_shape_that_does_not_fit_is_refused():
    n = 128
    m = _lib.twophase_max_m(n) + 1
    assert _lib.batch_lds_bytes(m, n) <= _lib.BATCH_LDS_MAX < _lib.twophase_lds_bytes(m, n)
    T = gen.tableau("mixed", m, n - m, 1)
    assert T.shape == (m + 1, n + 1)
    eng = _lib.BatchEngine(1, m, n)
    try:
        eng.upload(T[None])
        with pytest.raises(ValueError, match="too large"):
            eng.solve_lp()
        assert np.array_equal(bits(eng.download()[0]), bits(T))    # nothing ran
        status, npiv, _ = eng.solve()
        o = F64Tableau(T)
        st, log, _ = o.solve()
        assert status.tolist() == [st] and npiv.tolist() == [len(log)]
        assert np.array_equal(bits(eng.download()[0]), bits(o.T))
    finally:
        eng.close()
