"""General-form batches on the GPU (lp_general_set_form, lp_general_upload,
lp_general_solution, lp_general_duals; BatchEngine / RaggedEngine set_form(),
upload_general(), general_solution(), general_duals(); solve_problems and
solve_problems_ragged with lb, ub, maximize, c0).

Everything is compared in bits: the assembled tableaux with
general_standard_form, x and the objective with general_recover of the
device's own x', the duals and reduced costs with general_duals of the
downloaded tableaux, and the solves with the old calls on host-built
standard-form tableaux."""
import numpy as np
import pytest

import _general_cases as gc
import _problem_cases as pc
from _problem_cases import same_bits
from lpsol_amd import (_lib, solve_lp_batch, solve_lp_ragged, solve_batch, solve_problems, solve_problems_ragged)
from lpsol_amd import problem as pr

pytestmark = pytest.mark.gpu

CAP = 4096
BIG = (100, 100)        # mixed(100, 100) is 100 x 200: above one CU's LDS, device-placed under "auto"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def general_engine(P, lb, ub, sense, kind, mx, **kw):
    """an engine sized for the form, holding the standard-form tableaux of P"""
    mp, n = pr.general_shape(sense, kind)
    eng = _lib.BatchEngine(P.shape[0], mp, n, **kw)
    eng.set_form(sense, kind, mx)
    eng.upload_general(pr.pack_general(P, lb, ub))
    return eng


def recovery_check(eng, lb, ub, sense, kind, mx, windows=()):
    """general_solution() and general_duals() of the whole batch and of the
    windows against the host formulas on download() and on the device's x'"""
    T = eng.download()
    xs, _ = eng.solution()
    x, z = eng.general_solution()
    y, r = eng.general_duals()
    B, ns = len(T), len(kind)
    lo, hi = np.broadcast_to(lb, (B, ns)), np.broadcast_to(ub, (B, ns))
    want_x, want_z = pr.general_recover(xs, T[:, 0, 0], lo, hi, kind, mx)
    assert same_bits(x, want_x) and same_bits(z, want_z)
    want = [pr.general_duals(t, sense, kind, mx) for t in T]
    want_y, want_r = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    assert same_bits(y, want_y) and same_bits(r, want_r)
    eq = np.asarray(sense) == pc.EQ
    assert (pc.bits(y[:, eq]) == pc.QNAN_BITS).all()
    for first, count in windows:
        xw, zw = eng.general_solution(first, count)
        yw, rw = eng.general_duals(first, count)
        sl = slice(first, first + count)
        assert same_bits(xw, want_x[sl]) and same_bits(zw, want_z[sl])
        assert same_bits(yw, want_y[sl]) and same_bits(rw, want_r[sl])
    return x, z, y, r


# ---------------------------------------------------------------------------
# 1. the assembly against the host formula
# ---------------------------------------------------------------------------

def _one_by_one(kind):
    """three 1 x 1 LPs of one kind, dyadic values of both signs"""
    P = np.array([[[0.5, -1.25], [2.0, 1.5]], [[-0.0, 3.0], [-1.0, -0.5]], [[4.0, -0.0], [0.25, 2.0]]])
    lb = np.array([[-0.5], [1.0], [0.0]]) if kind in (gc.LOWER, gc.BOXED) else None
    ub = np.array([[0.75], [1.0], [-2.0]]) if kind in (gc.BOXED, gc.UPPER) else None
    if kind in (gc.UPPER, gc.FREE):
        lb = np.full((3, 1), -gc.INF)
    sense = np.array([(pc.LE, pc.GE, pc.EQ, pc.GE, pc.LE)[kind]], dtype=np.int8)
    return P, lb, ub, sense, np.array([kind], dtype=np.int8)


def _five_by_five():
    lps = [gc.general_lp(seed) for seed in range(5, 41, 5)]       # kinds 0, 1, 2, 3, 4 under mixed senses
    return (np.stack([lp[0] for lp in lps]), np.stack([lp[3] for lp in lps]), np.stack([lp[4] for lp in lps]),
            lps[0][1], lps[0][2])


def _special():
    P, sense = pc.special_block()
    # the NaN cost under the FREE variable (flipped, never multiplied), the denormal under the UPPER one
    kind = np.array([gc.FREE, gc.PLAIN, gc.UPPER], dtype=np.int8)
    return np.stack([P] * 3), np.array([-gc.INF, 0.0, -gc.INF]), np.array([gc.INF, gc.INF, 2.0]), sense, kind


def _boxed_8x10(B=64):
    T, sense, ns = pc.stack("mixed", 8, 10, range(1, B + 1))
    lb = np.array([(j % 3) / 4.0 for j in range(ns)])
    return pc.block(T, ns), lb, lb + 1.5, sense, np.full(ns, gc.BOXED, dtype=np.int8)


ASSEMBLE = {"kind_%d" % k: (lambda k=k: _one_by_one(k)) for k in range(5)}
ASSEMBLE.update(five_kinds_5x5=_five_by_five, special_cells=_special, boxed_8x10_x64=_boxed_8x10)


@pytest.mark.parametrize("mx", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("name", list(ASSEMBLE))
def test_assembly_equals_the_host(name, mx):
    P, lb, ub, sense, kind = ASSEMBLE[name]()
    eng = general_engine(P, lb, ub, sense, kind, mx)
    want = pr.general_standard_form(P, lb, ub, sense, kind, mx)
    got = eng.download()
    assert same_bits(got, want)
    assert all(eng.general_vars(i) == (P.shape[1] - 1, P.shape[2] - 1) for i in range(P.shape[0]))
    # once more over what is there now: every cell is written, none is left over
    eng.upload(np.full_like(want, 7.0))
    eng.upload_general(pr.pack_general(P, lb, ub))
    assert same_bits(eng.download(), want)
    if name == "special_cells":
        return          # the sign of a NaN that went through a subtraction is not defined: only copies and flips here
    # the recovery of whatever basis the tableaux show, and the duals of their row 0
    eng.derive_basis()
    lo, hi = pr._bounds(lb, ub, (P.shape[0], P.shape[2] - 1))
    recovery_check(eng, lo, hi, sense, kind, mx, windows=((1, 2),))


def test_all_plain_min_is_the_problem_form():
    blocks = np.stack([pc.mixed_sense_block(s, 5)[0] for s in range(1, 8)])
    for P, sense in ((blocks, np.array(pc.MIXED_SENSE, dtype=np.int8)),
                     (np.stack([pc.special_block()[0]] * 3), pc.special_block()[1])):
        ns = P.shape[2] - 1
        kind = np.zeros(ns, dtype=np.int8)
        eng = general_engine(P, None, None, sense, kind, False)
        old = _lib.BatchEngine(P.shape[0], P.shape[1] - 1, pr.problem_columns(sense, ns))
        old.set_senses(sense)
        old.upload_problems(P)
        assert same_bits(eng.download(), old.download())
        assert same_bits(eng.general_duals()[0], old.duals())


# ---------------------------------------------------------------------------
# 2. windows
# ---------------------------------------------------------------------------

def test_window_leaves_the_other_lps_alone_and_resets_its_own():
    P, lb, ub, sense, kind = _boxed_8x10(8)
    fresh = pc.block(pc.stack("mixed", 8, 10, range(101, 104))[0], 10)
    eng = general_engine(P, lb, ub, sense, kind, False, log_cap=64)
    status, _, _, ninit, npiv, _ = eng.solve_lp(CAP)        # the shifted b has both signs: phase 1 runs
    assert (status == _lib.OPTIMAL).any() and (ninit + npiv > 0).all()
    T0, basis0, logs0 = eng.download(), eng.get_basis(), [eng.log(i) for i in range(8)]
    x0, z0 = eng.general_solution()
    eng.upload_general(pr.pack_general(fresh, lb + 0.25, ub), first=2)
    T1, basis1 = eng.download(), eng.get_basis()
    keep = [0, 1, 5, 6, 7]
    want = pr.general_standard_form(fresh, lb + 0.25, ub, sense, kind, False)
    assert same_bits(T1[keep], T0[keep]) and same_bits(basis1, basis0)
    assert same_bits(T1[2:5], want)
    for i in range(8):      # the records: the solve's outside the window, reset inside it
        assert same_bits(eng.log(i), logs0[i] if i in keep else np.zeros((0, 2), dtype=np.int64))
    # the LPs outside keep their bounds: their recovery has not moved
    x1, z1 = eng.general_solution()
    assert same_bits(x1[keep], x0[keep]) and same_bits(z1[keep], z0[keep])
    # a re-uploaded LP solves from scratch, as on an engine of its own
    ref = _lib.BatchEngine(3, want.shape[1] - 1, want.shape[2] - 1, log_cap=64)
    ref.upload(want)
    for a, b in zip(eng.solve_lp(CAP), ref.solve_lp(CAP)):
        assert same_bits(a[2:5], b)
    assert same_bits(eng.download(2, 3), ref.download()) and same_bits(eng.get_basis()[2:5], ref.get_basis())
    for k in range(3):
        assert same_bits(eng.log(2 + k), ref.log(k))
    lo = np.stack([lb] * 2 + [lb + 0.25] * 3 + [lb] * 3)
    recovery_check(eng, lo, ub, sense, kind, False, windows=((2, 3), (0, 2)))


def test_windows_in_reverse_order_and_a_second_upload_keep_their_bounds():
    P, _, _, sense, kind = _five_by_five()
    B, ns = P.shape[0], P.shape[2] - 1
    lb = np.stack([np.full(ns, -1.0 + 0.25 * i) for i in range(B)])
    ub = lb + 2.0
    mp, n = pr.general_shape(sense, kind)
    eng = _lib.BatchEngine(B, mp, n)
    eng.set_form(sense, kind, True)
    G = pr.pack_general(P, lb, ub)
    eng.upload_general(G[5:], first=5)
    eng.upload_general(G[:5], first=0)
    assert same_bits(eng.download(), pr.general_standard_form(P, lb, ub, sense, kind, True))
    eng.solve_lp(CAP)
    x0, _, _, _ = recovery_check(eng, lb, ub, sense, kind, True, windows=((5, 3), (0, 5)))
    # other bounds for LPs [2, 4): their recovery moves, nobody else's does
    lb2, ub2 = lb.copy(), ub.copy()
    lb2[2:4] -= 0.5
    ub2[2:4] += 4.0
    solved = eng.download()
    eng.upload_general(pr.pack_general(P[2:4], lb2[2:4], ub2[2:4]), first=2)
    got, others = eng.download(), [0, 1, 4, 5, 6, 7]
    assert same_bits(got[2:4], pr.general_standard_form(P[2:4], lb2[2:4], ub2[2:4], sense, kind, True))
    assert same_bits(got[others], solved[others])
    eng.derive_basis()
    x1, _, _, _ = recovery_check(eng, lb2, ub2, sense, kind, True)
    assert not same_bits(x1[2:4], x0[2:4])


# ---------------------------------------------------------------------------
# 3. ragged batches
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged():
    lps = gc.ragged_general()
    want = [pr.general_standard_form(P, lb, ub, s, k, mx) for P, s, k, lb, ub, mx in lps]
    return lps, want


def ragged_engine(lps, place="auto"):
    """the 70 x 200 LP is 110 x 280 in standard form: above one CU's LDS, device-placed under auto"""
    eng = _lib.RaggedEngine([pr.general_shape(s, k) for _, s, k, _, _, _ in lps], place=place)
    eng.set_form([lp[1] for lp in lps], [lp[2] for lp in lps], [lp[5] for lp in lps])
    return eng


def packed(lps):
    return [pr.pack_general(P, lb, ub) for P, _, _, lb, ub, _ in lps]


def ragged_recovery_check(eng, lps, first=0, count=None):
    count = len(lps) - first if count is None else count
    T = eng.download(first, count)
    xs, _ = eng.solution(first, count)
    x, z = eng.general_solution(first, count)
    y, r = eng.general_duals(first, count)
    assert len(x) == len(y) == len(r) == len(z) == count
    for k, (P, s, kind, lb, ub, mx) in enumerate(lps[first:first + count]):
        want_x, want_z = pr.general_recover(xs[k], T[k][0, 0], lb, ub, kind, mx)
        want_y, want_r = pr.general_duals(T[k], s, kind, mx)
        assert same_bits(x[k], want_x) and same_bits(z[k:k + 1], np.array([want_z])), (first, k)
        assert same_bits(y[k], want_y) and same_bits(r[k], want_r), (first, k)


def test_ragged_windows(ragged):
    lps, want = ragged
    eng = ragged_engine(lps)
    for i, (P, s, k, _, _, _) in enumerate(lps):
        assert eng.general_vars(i) == (P.shape[0] - 1, P.shape[1] - 1)
    marks = [np.full(w.shape, 7.0 + i) for i, w in enumerate(want)]
    for first, count in pc.RAGGED_WINDOWS:
        eng.upload(marks)
        eng.upload_general(packed(lps[first:first + count]), first=first)
        got = eng.download()
        for i in range(len(lps)):
            inside = first <= i < first + count
            assert same_bits(got[i], want[i] if inside else marks[i]), (first, count, i)


def test_ragged_recovery_and_duals(ragged):
    lps, want = ragged
    eng = ragged_engine(lps)
    eng.upload_general(packed(lps))
    got = eng.download()
    assert all(same_bits(g, w) for g, w in zip(got, want))
    assert eng.placement(14) == "device" and eng.placement(0) == "lds"
    eng.solve_lp_placed(CAP)    # whatever each LP's outcome: both are reads of the stored tableaux
    ragged_recovery_check(eng, lps)
    for first, count in pc.RAGGED_WINDOWS[1:]:
        ragged_recovery_check(eng, lps, first, count)


# ---------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------

def e2e_lp_check(res, ref, i, s, kind, lb, ub, mx, T_final):
    """LP i of a general result against the old call's LP i on the standard form"""
    def pick(a):
        return a[i]

    xs = np.asarray(pick(ref.x))
    assert same_bits(pick(res.basis), pick(ref.basis))
    want_x, want_z = pr.general_recover(xs, T_final[0, 0], lb, ub, kind, mx)
    want_y, want_r = pr.general_duals(T_final, s, kind, mx)
    assert same_bits(pick(res.x), want_x) and same_bits(res.objective[i:i + 1], np.array([want_z]))
    assert same_bits(pick(res.y), want_y) and same_bits(pick(res.reduced_costs), want_r)
    assert same_bits(pick(res.slack), gc.slack_of(xs, s, kind))


def e2e_counts_check(res, ref, path):
    assert res.path == path
    assert same_bits(res.status_code, ref.status_code) and res.status == ref.status
    if path == "twophase":
        assert same_bits(res.stage, ref.stage) and same_bits(res.rows, ref.rows) and same_bits(res.ninit, ref.ninit)
    else:
        assert not res.stage.any() and not res.ninit.any()
    assert same_bits(res.npiv, ref.npiv) and same_bits(res.nstd, ref.nstd)


@pytest.mark.parametrize("mx", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("pattern", range(5))
def test_solve_problems_per_kind_pattern(pattern, mx):
    seeds = [s for s in gc.SEEDS if s % 5 == pattern]
    lps = [gc.general_lp(s) for s in seeds]
    P, lb, ub = (np.stack([lp[k] for lp in lps]) for k in (0, 3, 4))
    sense, kind = lps[0][1], lps[0][2]
    c, A, b = P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0]
    c0 = np.arange(len(seeds)) / 4.0
    res = solve_problems(c, A, b, sense, lb=lb, ub=ub, maximize=mx, c0=c0, max_pivots=CAP, log_cap=16)
    assert same_bits(res.kind, kind) and res.maximize is mx
    P = P.copy()
    P[:, 0, 0] = -c0
    T0 = pr.general_standard_form(P, lb, ub, sense, kind, mx)
    ref = solve_lp_batch(T0, max_pivots=CAP, result="solution", log_cap=16)
    e2e_counts_check(res, ref, "twophase")
    assert (res.status_code == _lib.OPTIMAL).any()
    for i in range(len(seeds)):
        e2e_lp_check(res, ref, i, sense, kind, lb[i], ub[i], mx, res.tableau(i).toArray())
        # and against the oracle where it ends optimal: the answer in the caller's terms
        o = gc.oracle_solve(P[i], sense, kind, lb[i], ub[i], mx)
        assert o["status"] == res.status_code[i]
        if o["status"] == _lib.OPTIMAL:
            assert same_bits(res.x[i], o["x"]) and res.objective[i] == o["z"]
    assert same_bits(res.log(0), ref.log(0)) and same_bits(res.init_log(0), ref.init_log(0))


def test_solve_problems_ragged_all_seeds_both_directions():
    lps = [(*gc.general_lp(s), mx) for mx in (False, True) for s in gc.SEEDS]
    # the call derives the kinds from the bounds: a LOWER variable whose lb is 0 is PLAIN there
    lps = [(P, s, pr.general_kinds(lb, ub), lb, ub, mx) for P, s, _, lb, ub, mx in lps]
    assert {int(k) for lp in lps for k in lp[2]} == {0, 1, 2, 3, 4}
    problems = [(P[0, 1:], P[1:, 1:], P[1:, 0], s, lb, ub, mx) for P, s, k, lb, ub, mx in lps]
    res = solve_problems_ragged(problems, max_pivots=CAP)
    T0 = [pr.general_standard_form(P, lb, ub, s, k, mx) for P, s, k, lb, ub, mx in lps]
    ref = solve_lp_ragged(T0, max_pivots=CAP, result="solution")
    e2e_counts_check(res, ref, "twophase")
    names = set(res.status)
    assert "optimal" in names and "unbounded" in names
    for i, (P, s, k, lb, ub, mx) in enumerate(lps):
        assert same_bits(res.kind[i], k) and res.maximize[i] is mx
        e2e_lp_check(res, ref, i, s, k, lb, ub, mx, res.tableau(i).toArray())


def test_solve_problems_plain_path():
    """all rows <= and every shifted LP canonical: Simplex.solve alone, under max as well"""
    P, lb, ub, sense, kind = _boxed_8x10(16)
    c, A, b = P[:, 0, 1:], P[:, 1:, 1:], P[:, 1:, 0]
    lb = np.zeros_like(lb)          # b stays >= 0 under a zero shift: canonical
    for mx in (False, True):
        res = solve_problems(c, A, b, lb=lb, ub=ub, maximize=mx, max_pivots=CAP)
        assert res.kind.tolist() == [gc.BOXED] * 10
        T0 = pr.general_standard_form(P, lb, ub, sense, kind, mx)
        ref = solve_batch(T0, max_pivots=CAP, result="solution")
        e2e_counts_check(res, ref, "plain")
        assert (res.status_code == _lib.OPTIMAL).all() and (res.rows == 18).all()
        for i in range(len(P)):
            e2e_lp_check(res, ref, i, sense, kind, lb, ub, mx, res.tableau(i).toArray())


def test_reduced_costs_of_a_problem_form_call():
    """the old call gains reduced_costs: row 0 under the structural variables"""
    T, sense, ns = pc.stack("mixed", 8, 10, range(1, 5))
    c, A, b = pc.parts(T, ns)
    res = solve_problems(c, A, b, max_pivots=CAP)
    assert res.kind is None and res.path == "plain"
    want = np.stack([res.tableau(i).toArray()[0, 1:ns + 1] for i in range(4)])
    assert same_bits(res.reduced_costs, want) and (res.reduced_costs >= -1e-9).all()


# ---------------------------------------------------------------------------
# 5. placement and teams
# ---------------------------------------------------------------------------

def _big_lower(seeds):
    T, sense, ns = pc.stack("mixed", *BIG, seeds)
    return pc.block(T, ns), np.zeros(ns), None, sense, np.full(ns, gc.LOWER, dtype=np.int8)


def _solve_all(eng):
    assert eng.derive_basis()[1] == -1
    return eng.solve(CAP)


def test_device_placed_batch():
    P, lb, ub, sense, kind = _five_by_five()
    want = pr.general_standard_form(P, lb, ub, sense, kind, True)
    eng = general_engine(P, lb, ub, sense, kind, True, place="device")
    assert eng.placement(0) == "device"
    assert same_bits(eng.download(), want)
    ref = _lib.BatchEngine(len(want), want.shape[1] - 1, want.shape[2] - 1, place="device")
    ref.upload(want)
    for a, b in zip(eng.solve_lp_placed(CAP), ref.solve_lp_placed(CAP)):
        assert same_bits(a, b)
    assert same_bits(eng.download(), ref.download()) and same_bits(eng.get_basis(), ref.get_basis())
    recovery_check(eng, lb, ub, sense, kind, True, windows=((3, 4),))


def test_teamed_batch_after_a_teamed_solve():
    kw = dict(place="device", team=2)
    P, lb, ub, sense, kind = _big_lower((2, 3, 4))
    fresh = _big_lower((5, 6, 7))[0]
    eng = general_engine(P, lb, ub, sense, kind, False, **kw)
    assert eng.team_of(0) == 2
    status, npiv, _ = _solve_all(eng)       # wherever a teamed solve leaves the current tableau
    assert (status == _lib.OPTIMAL).all() and (npiv % 2 == 1).any()
    want = pr.general_standard_form(fresh, lb, ub, sense, kind, False)
    ref = _lib.BatchEngine(3, want.shape[1] - 1, want.shape[2] - 1, **kw)
    ref.upload(want)
    eng.upload_general(pr.pack_general(fresh, lb, ub))
    assert same_bits(eng.download(), want)
    for a, b in zip(_solve_all(eng), _solve_all(ref)):
        assert same_bits(a, b)
    assert same_bits(eng.download(), ref.download()) and same_bits(eng.get_basis(), ref.get_basis())
    recovery_check(eng, lb, np.full(BIG[1], gc.INF), sense, kind, False)


# ---------------------------------------------------------------------------
# 6. refusals on a live batch
# ---------------------------------------------------------------------------

def test_refusals_on_a_live_batch():
    lib = _lib.load()
    P, lb, ub, sense, kind = _five_by_five()
    P, lb, ub = P[:4], lb[:4], ub[:4]
    G = pr.pack_general(P, lb, ub)
    mp, n = pr.general_shape(sense, kind)
    eng = _lib.BatchEngine(4, mp, n, log_cap=8)
    # before any form
    for call in (lambda: eng.upload_general(G), eng.general_solution, eng.general_duals):
        with pytest.raises(ValueError, match="no form attached"):
            call()
    assert lib.lp_general_upload(eng.h, 0, 4, _lib._ptr(G)) == _lib.BAD_ARG
    assert b"no form attached" in lib.lp_batch_last_error(eng.h)
    assert not eng.download().any()
    eng.set_form(sense, kind, False)
    eng.upload_general(G)
    want = pr.general_standard_form(P, lb, ub, sense, kind, False)
    # a shape mismatch, a bad kind, a bad sense, a bad direction: each names its entry and changes nothing
    for s, k, mx, text in ((sense, [0, 1, 2, 2, 4], False, "7 rows and 12 columns"),
                           (sense[:4], kind, False, "5 rows and 10 columns"),
                           (sense, [0, 1, 2, 3], False, "6 rows and 9 columns")):
        with pytest.raises(ValueError, match=text):
            eng.set_form(s, k, mx)
    dims = np.array([5, 5], dtype=np.int64)
    p64 = lambda a: a.ctypes.data_as(_lib._P64)
    p8 = lambda a: a.ctypes.data_as(_lib._P8)
    one, badk, bads = np.zeros(1, dtype=np.int8), np.array([0, 1, 7, 3, 4], dtype=np.int8), sense.copy()
    bads[3] = 3
    assert lib.lp_general_set_form(eng.h, p64(dims[:1]), p64(dims[1:]), p8(sense), p8(badk), p8(one)) == _lib.BAD_ARG
    assert b"variable 2" in lib.lp_batch_last_error(eng.h) and b"kind 7" in lib.lp_batch_last_error(eng.h)
    assert lib.lp_general_set_form(eng.h, p64(dims[:1]), p64(dims[1:]), p8(bads), p8(kind), p8(one)) == _lib.BAD_ARG
    assert b"row 3" in lib.lp_batch_last_error(eng.h) and b"sense 3" in lib.lp_batch_last_error(eng.h)
    two = np.array([2], dtype=np.int8)
    assert lib.lp_general_set_form(eng.h, p64(dims[:1]), p64(dims[1:]), p8(sense), p8(kind), p8(two)) == _lib.BAD_ARG
    assert eng.general_vars(3) == (5, 5)
    eng.upload(np.zeros_like(want))
    eng.upload_general(G)                   # still under the form attached before
    assert same_bits(eng.download(), want)
    # windows out of bounds, a NULL source, and the empty window
    for first in (-1, 1, 5):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.upload_general(G, first=first)
    for first, count in ((-1, 2), (3, 2), (5, 0), (0, -1)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.general_duals(first, count)
        with pytest.raises(ValueError, match="out of bounds"):
            eng.general_solution(first, count)
    assert lib.lp_general_upload(eng.h, 0, 2, None) == _lib.BAD_ARG
    assert b"NULL" in lib.lp_batch_last_error(eng.h)
    with pytest.raises(ValueError, match="no basis attached"):
        eng.general_solution()
    assert same_bits(eng.download(), want)
    # the batch still solves
    ref = _lib.BatchEngine(4, mp, n, log_cap=8)
    ref.upload(want)
    for a, b in zip(eng.solve_lp(CAP), ref.solve_lp(CAP)):
        assert same_bits(a, b)
    solved, log0 = eng.download(), eng.log(0)
    assert same_bits(solved, ref.download())
    assert lib.lp_general_upload(eng.h, 4, 0, None) == _lib.PIVOTED
    assert lib.lp_general_upload(eng.h, 0, 0, _lib._ptr(G)) == _lib.PIVOTED
    y, r = eng.general_duals(4, 0)
    assert y.shape[0] == 0 and r.shape[0] == 0
    assert same_bits(eng.download(), solved) and same_bits(eng.log(0), log0)
    recovery_check(eng, lb, ub, sense, kind, False)
    # detached: refused again
    eng.set_form(None)
    with pytest.raises(ValueError, match="no form attached"):
        eng.upload_general(G)
    # a ragged batch names the LP as well
    rag = _lib.RaggedEngine([(2, 4), (4, 9)])
    with pytest.raises(ValueError, match="LP 1.*4 rows and 8 columns"):
        rag.set_form([[0, 1], [0, 1, 2]], [[0, 0], [0, 1, 2, 3, 0]], [False, True])
    rag.set_form([[0, 1], [0, 1, 2]], [[0, 0], [0, 1, 2, 3, 4]], [False, True])
    assert rag.general_vars(1) == (3, 5)


# ---------------------------------------------------------------------------
# 7. the hand LPs
# ---------------------------------------------------------------------------

def test_hand_lps_are_exact_on_the_device():
    for h in gc.hand_lps():
        res = solve_problems(np.array([h["c"]]), np.array([h["A"]]), np.array([h["b"]]), h["sense"],
                             lb=h["lb"], ub=h["ub"], maximize=h["maximize"], c0=h["c0"], max_pivots=CAP)
        assert res.status == [h["status"]]
        if h["status"] != "optimal":
            continue
        assert res.x[0].tolist() == h["x"] and res.objective[0] == h["z"]
        assert res.y[0].tolist() == h["y"] and (res.reduced_costs[0] == np.array(h["r"])).all()
    one = gc.hand_lps()[:3]
    res = solve_problems_ragged([(h["c"], h["A"], h["b"], h["sense"], h["lb"], h["ub"], h["maximize"]) for h in one],
                                c0=[h["c0"] for h in one], max_pivots=CAP)
    for i, h in enumerate(one):
        assert res.x[i].tolist() == h["x"] and res.objective[i] == h["z"]
        assert res.y[i].tolist() == h["y"] and (res.reduced_costs[i] == np.array(h["r"])).all()
