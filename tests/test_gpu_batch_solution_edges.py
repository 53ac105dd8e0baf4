"""Batch solutions on the GPU, where test_gpu_batch_solution.py does not reach
(lp_solution_canonical, lp_solution_gather; csrc/batch.hip k_canon_*, k_solution).

a. The canonical scan at its row-slice edges (16|17 and 128|129 rows) and at
   S = 16 (1024 threads, all of s_nnz / s_one), LDS- and device-placed; hand-made
   columns whose entries lie in different slices, so that the reduction across
   the slices decides; windows of one ragged batch that run S = 16, 4 and 1.
b. 1500 ragged and 2048 uniform LPs in one window: the lane lookup's halvings,
   the first-bad minimum across many workgroups of both of its kernels.
c. The gather on teamed, ragged device-placed and phased batches and through
   result="solution" with place= and team=, against the float64 oracle
   (tests/_solution_cases.py oracle_solution, report_solution), which shares
   no code with the engine or with lpsol_amd.batch.solution_x.
d. NULL outputs of the two C calls.

Every comparison is exact, byte for byte, and every solve carries the pivot
cap CAP, which no oracle solve reaches (tests/test_solution_cases_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import _solution_cases as sc
from _solution_cases import same_bits
from lpsol_amd import _lib, solve_batch, solve_lp_batch, solve_lp_ragged, solve_ragged
from test_gpu_batch_solution import e2e_check, engine, gather_check, ragged_engine, same_list

pytestmark = pytest.mark.gpu

CAP = 4096


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


# ---------------------------------------------------------------------------
# a. the scan at the slice edges and at S = 16
# ---------------------------------------------------------------------------

def scan_window(eng, want, first, count):
    """derive_basis on a window of a uniform engine against the host's (basis,
    flags) of the whole batch"""
    want_basis, want_flags = want
    flags, bad = eng.derive_basis(first=first, count=count)
    assert same_bits(flags, want_flags[first:first + count])
    assert bad == next((i for i in range(first, first + count) if want_flags[i]), -1)
    assert same_bits(eng.get_basis()[first:first + count], want_basis[first:first + count])


@pytest.mark.parametrize("m,ns", sc.TALL_SHAPES, ids=["%dx%d" % (m, ns + m) for m, ns in sc.TALL_SHAPES])
def test_scan_at_the_slice_edges(m, ns):
    stack = sc.edge_stack(m, ns)
    eng = engine(stack, place="auto")
    assert eng.placement(0) == ("lds" if m <= 129 else "device")
    want_basis, want_flags, want_bad = sc.host_canonical(stack)
    exp = sc.edge_want(m, ns)
    assert same_bits(want_basis, exp[0]) and same_bits(want_flags, exp[1]) and want_bad == exp[2]
    for first, count in ((0, 5), (1, 3), (4, 1), (0, 5)):
        scan_window(eng, (want_basis, want_flags), first, count)
    assert same_bits(eng.get_basis(), want_basis)


@pytest.mark.parametrize("m", sc.TALL_HAND_M, ids=["S4", "S16"])
@pytest.mark.parametrize("name", sc.TALL_HAND_NAMES)
def test_hand_made_columns_across_the_slices(name, m):
    stack, basis, flags, first_bad = sc.tall_hand_stack(name, m)
    eng = engine(stack, place="auto")
    got_flags, got_bad = eng.derive_basis()
    assert same_bits(eng.get_basis(), basis)
    assert same_bits(got_flags, flags) and got_bad == first_bad
    # the case alone in its window: one LP, the same slices
    got_flags, got_bad = eng.derive_basis(first=1, count=1)
    assert got_flags.tolist() == [flags[1]] and got_bad == first_bad
    assert same_bits(eng.get_basis(), basis)


def test_the_slices_follow_the_window():
    items = sc.window_items()
    eng = ragged_engine(items, place="auto")
    assert [eng.placement(i) for i in range(5)] == ["lds"] * 5
    want_basis, want_flags, _ = sc.host_canonical_list(items)
    marks = [np.arange(T.shape[0] - 1, dtype=np.int32) + 1000 * (i + 1) for i, T in enumerate(items)]
    # the whole batch S = 16, [2, 5) S = 4, [2, 3) S = 1, [1, 2) S = 16 on one LP
    for first, count in ((0, 5), (2, 3), (2, 1), (1, 1)):
        eng.set_basis(marks)
        flags, bad = eng.derive_basis(first=first, count=count)
        assert same_bits(flags, want_flags[first:first + count]), (first, count)
        assert bad == (sc.WINDOW_BAD if first <= sc.WINDOW_BAD < first + count else -1), (first, count)
        got = eng.get_basis()
        for i in range(5):
            inside = first <= i < first + count
            assert same_bits(got[i], want_basis[i] if inside else marks[i]), (first, count, i)


# ---------------------------------------------------------------------------
# b. many LPs in one window
# ---------------------------------------------------------------------------

def ragged_scan_window(eng, want, first, count):
    want_basis, want_flags = want
    flags, bad = eng.derive_basis(first=first, count=count)
    assert same_bits(flags, want_flags[first:first + count]), (first, count)
    assert bad == next((i for i in range(first, first + count) if want_flags[i]), -1), (first, count)
    got = eng.get_basis()
    assert all(same_bits(got[i], want_basis[i]) for i in range(first, first + count)), (first, count)
    return got


def test_many_ragged_lps_scan():
    items = sc.many_ragged()
    eng = ragged_engine(items)
    want_basis, want_flags, want_bad = sc.host_canonical_list(items)
    assert same_bits(want_flags, sc.many_flags()) and want_bad == sc.MANY_BAD[0]
    ragged_scan_window(eng, (want_basis, want_flags), 0, sc.MANY)
    marks = [np.full(T.shape[0] - 1, 7000 + i, dtype=np.int32) for i, T in enumerate(items)]
    for first, count in sc.MANY_WINDOWS:
        eng.set_basis(marks)
        got = ragged_scan_window(eng, (want_basis, want_flags), first, count)
        outside = [i for i in range(sc.MANY) if not first <= i < first + count]
        assert all(same_bits(got[i], marks[i]) for i in outside), (first, count)
    flags, bad = eng.derive_basis(first=700, count=800)
    assert bad == 701 and np.nonzero(flags)[0].tolist() == [i - 700 for i in sc.MANY_BAD if 700 <= i < 1500]
    flags, bad = eng.derive_basis(first=1499, count=1)
    assert bad == 1499 and flags.tolist() == [sc.many_kind(1499)]


def oracle_list(items, start):
    return [sc.oracle_solution(T, b, CAP) for T, b in zip(items, start)]


def against_oracle(want, status, basis, x, z, first=0):
    """the engine's status, basis, x and z of LPs first, first + 1, ... against oracle_solution's"""
    assert len(x) == len(z) == len(want)
    for k, (st, b, wx, wz) in enumerate(want):
        i = first + k
        assert status[i] == st, i
        assert same_bits(np.asarray(basis[i]), b), i
        assert same_bits(np.asarray(x[k]), wx), i
        assert same_bits(z[k:k + 1], np.array([wz])), i


def test_many_ragged_lps_solution():
    spoiled, items = sc.many_ragged(), sc.many_ragged(spoiled=False)
    eng = ragged_engine(spoiled, log_cap=4)
    assert eng.derive_basis()[1] == sc.MANY_BAD[0]
    eng.upload(items)                   # mended
    flags, bad = eng.derive_basis()
    assert bad == -1 and not flags.any()
    start = [b.copy() for b in eng.get_basis()]
    st, npiv, _ = eng.solve(CAP)
    assert (st == _lib.OPTIMAL).all() and (npiv > 0).any()
    x, z = gather_check(eng)
    want = oracle_list(items, start)
    against_oracle(want, st, eng.get_basis(), x, z)
    xw, zw = eng.solution(first=733, count=517)
    assert same_list(xw, x[733:1250]) and same_bits(zw, z[733:1250])
    against_oracle(want[733:1250], st, eng.get_basis(), xw, zw, first=733)


def test_many_uniform_lps_scan():
    stack = sc.many_uniform()
    eng = engine(stack)
    want_basis, want_flags, _ = sc.host_canonical(stack)
    for first, count in sc.UNIFORM_WINDOWS:
        scan_window(eng, (want_basis, want_flags), first, count)
    assert eng.derive_basis(first=1, count=1000)[1] == -1
    assert eng.derive_basis(first=1000, count=24)[1] == 1023
    assert eng.derive_basis(first=1024, count=1024)[1] == 1024
    assert eng.derive_basis()[1] == 0
    assert same_bits(eng.get_basis(), want_basis)


def test_first_bad_with_every_workgroup_contending():
    stack = sc.all_bad_uniform()
    eng = engine(stack)
    want_basis, want_flags, _ = sc.host_canonical(stack)
    for first, count in ((0, 2048), (1, 2047), (1001, 1000), (2047, 1)):
        scan_window(eng, (want_basis, want_flags), first, count)
        assert eng.derive_basis(first=first, count=count)[1] == first


# ---------------------------------------------------------------------------
# c. the gather on every kind of batch, against the oracle
# ---------------------------------------------------------------------------

def test_teamed_solution_against_the_oracle():
    stack = sc.teamed_stack()
    eng = engine(stack, place="auto", team=4, log_cap=4)
    assert eng.team_of(0) == eng.team_of(1) == 4 and eng.placement(0) == "device"
    _, bad = eng.derive_basis()
    assert bad == -1
    start = eng.get_basis().copy()
    st, npiv, _ = eng.solve(CAP)
    assert (npiv % 2 == 1).all() and npiv.tolist() == [235, 303]       # both end in the second buffer
    x, z = gather_check(eng)
    against_oracle(oracle_list(stack, start), st, eng.get_basis(), x, z)
    assert (st == _lib.OPTIMAL).all() and x.any()


def test_teamed_solution_mid_solve_against_the_oracle():
    stack = sc.teamed_stack()
    eng = engine(stack, place="auto", team=4, log_cap=4)
    assert eng.team_of(0) == 4
    eng.derive_basis()
    start = eng.get_basis().copy()
    st, done = eng.run(_lib.RULE_STANDARD, 3)
    assert done.tolist() == [3, 3]
    x, z = gather_check(eng)
    want = [sc.oracle_solution(T, b, CAP, rule=_lib.RULE_STANDARD, steps=3) for T, b in zip(stack, start)]
    against_oracle(want, st, eng.get_basis(), x, z)


def paired_basis(T):
    """a hand-set start in which rows 2k and 2k + 1 share slack column 2k: x
    of that column is the later row's b, as long as neither row pivots"""
    m, n = T.shape[0] - 1, T.shape[1] - 1
    return (n - m + 2 * (np.arange(m) // 2)).astype(np.int32)


def test_the_later_row_wins_on_ragged_placed_and_teamed_batches():
    """duplicate basis columns survive a solve in the rows that never pivot:
    the engine's x takes the later row there, as the oracle's loop does"""
    items = sc.placed_items()
    start = [paired_basis(T) for T in items]
    want = oracle_list(items, start)
    assert sum(len(set(b.tolist())) < len(b) for _, b, _, _ in want) >= 2        # still there at the end: LPs 1 and 3
    eng = ragged_engine(items, place="auto", team=[1, 4, 1, 1, 1], log_cap=4)
    assert eng.placement(1) == "device" and eng.team_of(1) == 4
    eng.set_basis(start)
    st, _, _ = eng.solve(CAP)
    x, z = gather_check(eng)
    against_oracle(want, st, eng.get_basis(), x, z)
    xw, zw = eng.solution(first=1, count=3)
    against_oracle(want[1:4], st, eng.get_basis(), xw, zw, first=1)
    # uniform, device-placed, a team of 4
    stack = sc.teamed_stack()
    start = np.stack([paired_basis(T) for T in stack])
    want = oracle_list(stack, start)
    assert all(len(set(b.tolist())) < len(b) for _, b, _, _ in want)
    eng = engine(stack, place="auto", team=4, log_cap=4)
    eng.set_basis(start)
    st, _, _ = eng.solve(CAP)
    x, z = gather_check(eng)
    against_oracle(want, st, eng.get_basis(), x, z)


def result_against_oracle(res, want):
    against_oracle(want, res.status_code, res.basis, res.x, res.objective)


def test_sixteen_slices_end_to_end():
    stack = sc.s16_stack()
    slim, full = e2e_check(solve_batch, stack, (0, 1), place="auto", log_cap=4)
    assert slim._engine.placement(0) == "device" and sc.slices(stack.shape[1] - 1) == 16
    want = oracle_list(stack, sc.host_canonical(stack)[0])
    result_against_oracle(slim, want)
    result_against_oracle(full, want)
    assert slim.npiv.tolist() == [391, 465]


@pytest.mark.parametrize("team", [1, "auto"])
def test_ragged_mixed_placement_against_the_oracle(team):
    items = sc.placed_items()
    slim, full = e2e_check(solve_ragged, items, (0, 1, 4), place="auto", team=team, log_cap=4)
    assert [slim._engine.placement(i) for i in range(5)] == ["lds", "device", "lds", "lds", "lds"]
    want = oracle_list(items, sc.host_canonical_list(items)[0])
    result_against_oracle(slim, want)
    result_against_oracle(full, want)
    assert (slim.status_code == _lib.OPTIMAL).all()


def phased_against_oracle(res, items):
    for i, T in enumerate(items):
        st, stage, rows, basis, x, z = sc.report_solution(T, CAP)
        assert (res.status_code[i], res.stage[i], res.rows[i]) == (st, stage, rows), i
        assert same_bits(np.asarray(res.basis[i]), basis), i
        assert same_bits(np.asarray(res.x[i]), x), i
        assert same_bits(res.objective[i:i + 1], np.array([z])), i


def test_phased_solutions_against_the_oracle():
    items = sc.phased_mix()
    m = items[4].shape[0] - 1
    for fn, inputs in ((solve_lp_ragged, items), (solve_lp_batch, np.stack(items[:4])),
                       (solve_lp_batch, np.stack(items[4:]))):
        slim, full = e2e_check(fn, inputs, range(len(inputs)), place="device", log_cap=4)
        assert slim._engine.phased_placement(0) == "device"
        phased_against_oracle(slim, list(inputs))
        phased_against_oracle(full, list(inputs))
    # the last call's LPs drop a row: the basis keeps -1 there
    assert (slim.rows < m).all() and all((np.asarray(b)[int(r):] == -1).all() for b, r in zip(slim.basis, slim.rows))


@pytest.mark.parametrize("fn,inputs", [(solve_batch, "e2e_mixed"), (solve_ragged, "e2e_ragged"),
                                       (solve_lp_batch, "e2e_phase1"), (solve_lp_ragged, "e2e_ragged_phase1")],
                         ids=["solve_batch", "solve_ragged", "solve_lp_batch", "solve_lp_ragged"])
def test_e2e_with_place_and_team(fn, inputs):
    inputs = getattr(sc, inputs)()[:16]
    slim, _ = e2e_check(fn, inputs, (0, 15), place="device", log_cap=4)
    assert slim._engine.placement(0) == "device"
    if fn in (solve_batch, solve_ragged):
        teamed, _ = e2e_check(fn, inputs, (0, 15), place="device", team=2, log_cap=4)
        assert teamed._engine.team_of(0) == 2
        same = same_list if fn is solve_ragged else same_bits
        assert same(teamed.x, slim.x) and same(teamed.basis, slim.basis)
        assert same_bits(teamed.objective, slim.objective)


# ---------------------------------------------------------------------------
# d. NULL outputs
# ---------------------------------------------------------------------------

def test_canonical_without_flags_or_first_bad():
    stack = sc.edge_stack(8, 10)
    want_basis, want_flags, want_bad = sc.host_canonical(stack)
    P32 = C.POINTER(C.c_int32)
    # no flags: first_bad and the basis all the same
    eng = engine(stack)
    bad = C.c_int64(-7)
    assert eng.lib.lp_solution_canonical(eng.h, 0, 5, None, C.byref(bad)) == _lib.PIVOTED
    assert bad.value == want_bad and same_bits(eng.get_basis(), want_basis)
    # no first_bad: the flags and the basis all the same
    eng = engine(stack)
    flags = np.full(5, -7, dtype=np.int32)
    assert eng.lib.lp_solution_canonical(eng.h, 0, 5, flags.ctypes.data_as(P32), None) == _lib.PIVOTED
    assert same_bits(flags, want_flags) and same_bits(eng.get_basis(), want_basis)
    # neither, on a window
    eng = engine(stack)
    assert eng.lib.lp_solution_canonical(eng.h, 1, 2, None, None) == _lib.PIVOTED
    got = eng.get_basis()
    assert same_bits(got[1:3], want_basis[1:3]) and (got[:1] == -1).all() and (got[3:] == -1).all()


def test_gather_without_x_on_a_ragged_window():
    items = sc.e2e_ragged()
    eng = ragged_engine(items)
    eng.derive_basis()
    st, _, _ = eng.solve(CAP)
    assert (st == _lib.OPTIMAL).all()
    x, z = eng.solution()
    none, zw = eng.solution(first=7, count=9, want_x=False)
    assert none is None and same_bits(zw, z[7:16])
    xw, none = eng.solution(first=7, count=9, want_z=False)
    assert none is None and same_list(xw, x[7:16])
    x2, z2 = eng.solution()
    assert same_list(x2, x) and same_bits(z2, z)
    against_oracle(oracle_list(items, sc.host_canonical_list(items)[0]), st, eng.get_basis(), x, z)
