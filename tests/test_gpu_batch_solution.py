"""Batch solutions on the GPU (lp_solution_canonical, lp_solution_gather;
BatchEngine / RaggedEngine derive_basis() and solution(); result="solution" of
the four batch solve functions; csrc/batch.hip k_canon_*, k_solution).

Every comparison is exact, byte for byte: the canonical scan against
lpsol_amd.batch._canonical on the same tableaux (tests/_solution_cases.py
host_canonical: basis entries, both flag bits, first_bad), the solution gather
against the host formula (lpsol_amd.batch.solution_x) on download() and
get_basis(), and result="solution" against result="full".  Every solve carries
a finite pivot cap."""
import numpy as np
import pytest

import _solution_cases as sc
from _solution_cases import same_bits
from lpsol_amd import _lib, solve_batch, solve_lp_batch, solve_lp_ragged, solve_ragged
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis, ragged_canonical_basis, solution_x

pytestmark = pytest.mark.gpu

CAP = 4096
BIG = (100, 100)        # mixed(100, 100) is 100 x 200: above one CU's LDS, device-placed under "auto"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def engine(stack, **kw):
    eng = _lib.BatchEngine(stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1, **kw)
    eng.upload(stack)
    return eng


def ragged_engine(items, **kw):
    eng = _lib.RaggedEngine([(T.shape[0] - 1, T.shape[1] - 1) for T in items], **kw)
    eng.upload(items)
    return eng


# ---------------------------------------------------------------------------
# 1. the canonical scan against _canonical
# ---------------------------------------------------------------------------

def scan_check(eng, stack):
    """derive_basis() on the whole batch against the host on `stack`"""
    want_basis, want_flags, want_bad = sc.host_canonical(stack)
    flags, bad = eng.derive_basis()
    assert same_bits(flags, want_flags) and bad == want_bad
    assert same_bits(eng.get_basis(), want_basis)
    return want_basis, want_flags, want_bad


@pytest.mark.parametrize("name", sc.HAND_NAMES)
def test_hand_made_scan_cases(name):
    stack, basis, flags, first_bad = sc.hand_stack(name)
    eng = engine(stack)
    want = scan_check(eng, stack)
    assert same_bits(want[0], basis) and same_bits(want[1], flags) and want[2] == first_bad


@pytest.mark.parametrize("at", [0, 2, 4])
def test_first_bad_by_position(at):
    stack, first_bad = sc.position_stack(at)
    eng = engine(stack)
    assert scan_check(eng, stack)[2] == first_bad == at
    # a window that begins behind the bad LP does not see it
    if at < 4:
        flags, bad = eng.derive_basis(first=at + 1)
        assert bad == -1 and not flags.any() and len(flags) == 4 - at


@pytest.mark.parametrize("m,ns", sc.EDGE_SHAPES, ids=["%dx%d" % (m, ns + m) for m, ns in sc.EDGE_SHAPES])
def test_scan_at_the_wave_and_block_edges(m, ns):
    stack = sc.edge_stack(m, ns)
    want = scan_check(engine(stack), stack)
    exp = sc.edge_want(m, ns)
    assert same_bits(want[0], exp[0]) and same_bits(want[1], exp[1]) and want[2] == exp[2]


def window_check(stack, **kw):
    """upload 7 LPs; a window of three on an engine with no basis attached
    leaves -1 outside it; after set_basis on all LPs the entries outside keep
    their values"""
    assert stack.shape[0] == 7
    m = stack.shape[1] - 1
    eng = engine(stack, **kw)
    want_basis, want_flags, _ = sc.host_canonical(stack)
    with pytest.raises(ValueError, match="no basis attached"):
        eng.get_basis()
    flags, bad = eng.derive_basis(first=2, count=3)
    got = eng.get_basis()
    assert same_bits(flags, want_flags[2:5])
    assert bad == next((i for i in range(2, 5) if want_flags[i]), -1)
    assert same_bits(got[2:5], want_basis[2:5])
    assert (got[:2] == -1).all() and (got[5:] == -1).all()
    marks = np.arange(7 * m, dtype=np.int32).reshape(7, m) + 1000
    eng.set_basis(marks)
    flags, bad = eng.derive_basis(first=2, count=3)
    got = eng.get_basis()
    assert same_bits(flags, want_flags[2:5]) and same_bits(got[2:5], want_basis[2:5])
    assert same_bits(got[:2], marks[:2]) and same_bits(got[5:], marks[5:])
    # detached and derived again: -1 outside once more
    eng.set_basis(None)
    eng.derive_basis(first=6, count=1)
    got = eng.get_basis()
    assert (got[:6] == -1).all() and same_bits(got[6:], want_basis[6:])
    # the empty window and the windows out of bounds
    flags, bad = eng.derive_basis(first=7, count=0)
    assert len(flags) == 0 and bad == -1
    for first, count in ((-1, 2), (6, 2), (8, 0), (0, -1)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.derive_basis(first=first, count=count)
    assert same_bits(eng.get_basis(), got)
    return eng


def seven(m, ns):
    """seven LPs: sc.edge_stack's five and two more, LP 5 with a negative b"""
    more = gen.mixed_stack(m, ns, (6, 7)).copy()
    more[0, 2 if m > 1 else 1, 0] = -2.0
    return np.concatenate([sc.edge_stack(m, ns), more])


def test_scan_window():
    window_check(seven(8, 10))


def test_scan_window_device_placed():
    eng = window_check(seven(8, 10), place="device")
    assert eng.placement(0) == "device"


def test_scan_device_placed_above_lds():
    stack = sc.edge_stack(*BIG)[:3]
    eng = engine(stack, place="auto")
    assert eng.placement(0) == "device"
    scan_check(eng, stack)
    flags, bad = eng.derive_basis(first=1, count=2)
    assert flags.tolist() == [sc.NO_COLUMN, 0] and bad == 1


def test_scan_reads_the_home_buffer_of_a_teamed_batch():
    stack = gen.mixed_stack(*BIG, (1, 2))
    eng = engine(stack, place="auto", team=4)
    assert eng.team_of(0) == 4
    basis0 = scan_check(eng, stack)[0]
    assert same_bits(basis0, canonical_basis(stack))
    st, npiv, _ = eng.solve(CAP)
    assert (st == _lib.OPTIMAL).all() and (npiv % 2 == 1).any()      # an odd count ends in the second buffer
    scan_check(eng, eng.download())     # the final tableaux: wherever the last pivot wrote them, they are home


def test_scan_ragged():
    items = sc.ragged_items()
    eng = ragged_engine(items)
    want_basis, want_flags, want_bad = sc.host_canonical_list(items)
    flags, bad = eng.derive_basis()
    assert flags.tolist() == sc.RAGGED_FLAGS and same_bits(flags, want_flags) and bad == want_bad == 3
    got = eng.get_basis()
    assert len(got) == 12 and all(same_bits(g, w) for g, w in zip(got, want_basis))
    # the good LPs, against ragged_canonical_basis
    good = [i for i in range(12) if not want_flags[i]]
    ref = ragged_canonical_basis([items[i] for i in good])
    assert all(same_bits(got[i], r) for i, r in zip(good, ref))
    # windows: behind the first bad LP, and one LP
    flags, bad = eng.derive_basis(first=4)
    assert bad == 8 and flags.tolist() == sc.RAGGED_FLAGS[4:]
    flags, bad = eng.derive_basis(first=9, count=2)
    assert bad == -1 and flags.tolist() == [0, 0]
    got = eng.get_basis()
    assert all(same_bits(g, w) for g, w in zip(got, want_basis))


def test_scan_ragged_placed_and_mixed_heights():
    """LPs of 1 to 100 rows in one window: the row slices follow the tallest"""
    items = [sc.edge_stack(m, ns)[k] for k, (m, ns) in enumerate([(1, 1), (100, 100), (2, 3), (65, 4), (3, 60)])]
    eng = ragged_engine(items, place="auto")
    assert [eng.placement(i) for i in range(5)] == ["lds", "device", "lds", "lds", "lds"]
    want_basis, want_flags, want_bad = sc.host_canonical_list(items)
    flags, bad = eng.derive_basis()
    assert same_bits(flags, want_flags) and bad == want_bad == 1
    assert all(same_bits(g, w) for g, w in zip(eng.get_basis(), want_basis))


def test_scan_after_a_solve():
    stack = gen.mixed_stack(8, 10, range(1, 17))
    eng = engine(stack)
    eng.derive_basis()
    st, _, _ = eng.solve(CAP)
    assert (st == _lib.OPTIMAL).all()
    scan_check(eng, eng.download())


# ---------------------------------------------------------------------------
# 2. the solution gather against the host formula
# ---------------------------------------------------------------------------

def gather_check(eng):
    """solution() against solution_x on download() and get_basis(), z against
    objective(); nothing stored changes"""
    ragged = isinstance(eng, _lib.RaggedEngine)
    T, basis = eng.download(), eng.get_basis()
    logs = [eng.log(i) for i in range(eng.count)]
    want_z = eng.objective()
    x, z = eng.solution()
    assert same_bits(z, want_z) and same_bits(z, np.array([-t[0, 0] for t in T]))
    assert len(x) == eng.count
    for i in range(eng.count):
        assert same_bits(x[i], solution_x(T[i], basis[i])), i
    if not ragged:
        assert x.shape == (eng.count, eng.n)
    T2, basis2 = eng.download(), eng.get_basis()
    assert all(same_bits(a, b) for a, b in zip(T, T2)) and all(same_bits(a, b) for a, b in zip(basis, basis2))
    assert all(same_bits(a, eng.log(i)) for i, a in enumerate(logs))
    # windows give the same values
    if eng.count >= 3:
        xw, zw = eng.solution(first=1, count=2)
        assert same_bits(zw, z[1:3]) and all(same_bits(xw[k], x[1 + k]) for k in range(2))
    return x, z


@pytest.mark.parametrize("m,ns,B,place", [(8, 10, 33, "lds"), (40, 40, 3, "lds"), (100, 100, 2, "auto")],
                         ids=["8x10x33", "40x40x3", "100x100x2-auto"])
def test_solution_after_solve(m, ns, B, place):
    stack = gen.mixed_stack(m, ns, range(1, B + 1))
    eng = engine(stack, place=place, log_cap=8)
    eng.derive_basis()
    st, npiv, _ = eng.solve(CAP)
    assert (st == _lib.OPTIMAL).all()
    x, _ = gather_check(eng)
    assert (npiv > 0).any() and x.any()


def test_solution_ragged_after_solve():
    items = sc.ragged_items()
    items[3][2, 0] = 0.5                            # the two bad LPs mended
    items[8][9, 1 + 4 + 8] = 1.0
    eng = ragged_engine(items, log_cap=8)
    _, bad = eng.derive_basis()
    assert bad == -1
    st, _, _ = eng.solve(CAP)
    assert (st == _lib.OPTIMAL).all()
    x, _ = gather_check(eng)
    assert [len(a) for a in x] == [13] * 12


def test_solution_mid_solve():
    stack = gen.mixed_stack(8, 10, range(1, 5))
    eng = engine(stack, log_cap=8)
    eng.derive_basis()
    st, done = eng.run(_lib.RULE_STANDARD, 3)
    assert (done > 0).any()
    gather_check(eng)


def test_solution_after_two_phase_skips_the_dropped_rows():
    ge = np.stack([gen.phase1_lp("ge", 8, 10, s) for s in (1, 2, 3)])
    eng = engine(ge, log_cap=8)
    st, stage, rows, *_ = eng.solve_lp(CAP)
    assert (st == _lib.OPTIMAL).all()
    gather_check(eng)
    dep = sc.dropped_row_lp()
    eng = engine(np.stack([dep, dep]), log_cap=8)
    st, stage, rows, *_ = eng.solve_lp(CAP)
    m = dep.shape[0] - 1
    assert (st == _lib.OPTIMAL).all() and (rows < m).all()
    assert (eng.get_basis()[:, m - 1] == -1).all()
    gather_check(eng)


def test_solution_of_a_hand_set_basis():
    stack = gen.mixed_stack(8, 2, range(1, 4))          # n = 10
    eng = engine(stack)
    basis = np.tile(np.arange(2, 10, dtype=np.int32), (3, 1))
    basis[0, 5] = basis[0, 1]           # a duplicate column: the later row wins
    basis[1, 0] = -1                    # skipped
    basis[1, 7] = 10                    # n: skipped
    basis[2, :] = 4                     # all rows on one column: the last row wins
    eng.set_basis(basis)
    x, z = gather_check(eng)
    b = stack[:, 1:, 0]
    assert x[0, basis[0, 1]] == b[0, 5] != b[0, 1]
    assert x[1].tolist() == [0.0] * 3 + b[1, 1:7].tolist() + [0.0]
    assert x[2].tolist() == [0.0] * 4 + [b[2, 7]] + [0.0] * 5
    # the uploaded T[0][0] is +0.0: z is -0.0, as objective() has it
    assert not stack[:, 0, 0].view(np.uint64).any()
    assert (z == 0.0).all() and np.signbit(z).all()


def test_solution_x_alone_and_z_alone():
    stack = gen.mixed_stack(8, 10, range(1, 6))
    eng = engine(stack)
    eng.derive_basis()
    eng.solve(CAP)
    x, z = eng.solution()
    xa, none = eng.solution(want_z=False)
    assert none is None and same_bits(xa, x)
    none, za = eng.solution(want_x=False)
    assert none is None and same_bits(za, z)
    none, zw = eng.solution(first=3, count=2, want_x=False)
    assert none is None and same_bits(zw, z[3:])
    assert eng.solution(want_x=False, want_z=False) == (None, None)
    x0, z0 = eng.solution(first=5, count=0)
    assert x0.shape == (0, 18) and z0.shape == (0,)
    for first, count in ((-1, 2), (4, 2), (6, 0), (0, -1)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.solution(first=first, count=count)


def test_solution_needs_a_basis():
    stack = gen.mixed_stack(8, 2, range(1, 3))
    eng = engine(stack)
    with pytest.raises(ValueError, match="no basis attached"):
        eng.solution()
    eng.derive_basis()
    eng.solution()
    eng.set_basis(None)
    with pytest.raises(ValueError, match="no basis attached"):
        eng.solution()
    reng = ragged_engine(list(stack))
    with pytest.raises(ValueError, match="no basis attached"):
        reng.solution()


# ---------------------------------------------------------------------------
# 3. end to end: result="solution" against result="full"
# ---------------------------------------------------------------------------

def same_list(a, b):
    return len(a) == len(b) and all(same_bits(p, q) for p, q in zip(a, b))


def e2e_check(fn, inputs, picks, **kw):
    slim = fn(inputs, result="solution", max_pivots=CAP, **kw)
    full = fn(inputs, max_pivots=CAP, **kw)
    assert slim.tableaux is None and full.tableaux is not None
    assert slim.status == full.status and len(slim) == len(full)
    fields = ["status_code", "npiv", "nstd", "objective"]
    if hasattr(full, "stage"):
        fields += ["stage", "rows", "ninit"]
    for f in fields:
        assert same_bits(getattr(slim, f), getattr(full, f)), f
    ragged = isinstance(full.basis, list)
    if ragged:
        assert same_list(slim.basis, full.basis) and same_list(slim.x, full.x)
    else:
        assert same_bits(slim.basis, full.basis) and same_bits(slim.x, full.x)
    for i in picks:
        assert same_bits(slim.tableau(i).toArray(), full.tableau(i).toArray()), i
        assert same_bits(slim.log(i), full.log(i)), i
    return slim, full


def test_e2e_solve_batch():
    slim, _ = e2e_check(solve_batch, sc.e2e_mixed(), (0, 31, 63), log_cap=8)
    assert slim.x.shape == (64, 18) and (slim.status_code == _lib.OPTIMAL).all()
    e2e_check(solve_batch, sc.e2e_mixed(), (5,), rule=_lib.RULE_STANDARD, steps=2)


def test_e2e_solve_lp_batch():
    slim, _ = e2e_check(solve_lp_batch, sc.e2e_phase1(), (0, 7, 15), log_cap=8)
    assert (slim.status_code == _lib.OPTIMAL).all() and (slim.ninit > 0).all()
    e2e_check(solve_lp_batch, sc.e2e_mixed(), (0, 31, 63))
    dep = sc.dropped_row_lp()
    slim, _ = e2e_check(solve_lp_batch, np.stack([dep] * 3), (0, 1, 2))
    assert slim.tableau(1).toArray().shape[0] == int(slim.rows[1]) + 1 < dep.shape[0]


def test_e2e_solve_ragged():
    slim, _ = e2e_check(solve_ragged, sc.e2e_ragged(), (0, 9, 19), log_cap=8)
    assert [len(a) for a in slim.x] == [m + ns for m, ns in sc.E2E_SHAPES]
    e2e_check(solve_ragged, list(sc.e2e_mixed()), (0, 31, 63))


def test_e2e_solve_lp_ragged():
    e2e_check(solve_lp_ragged, sc.e2e_ragged_phase1(), (0, 9, 19), log_cap=8)
    e2e_check(solve_lp_ragged, list(sc.e2e_phase1()), (0, 7, 15))
    e2e_check(solve_lp_ragged, sc.e2e_ragged(), (3,))


def test_e2e_a_bad_lp_raises_the_default_paths_message():
    stack = sc.e2e_mixed()[:8].copy()
    stack[5, 3, 0] = -1.0
    stack[7, 8, 1 + 10 + 7] = 0.0       # a later bad LP: the first is named
    with pytest.raises(ValueError) as full:
        solve_batch(stack)
    with pytest.raises(ValueError) as slim:
        solve_batch(stack, result="solution")
    assert str(slim.value) == str(full.value) and "LP 5 of the batch" in str(full.value)
    items = sc.ragged_items()
    with pytest.raises(ValueError) as full:
        solve_ragged(items)
    with pytest.raises(ValueError) as slim:
        solve_ragged(items, result="solution")
    assert str(slim.value) == str(full.value) and "LP 3 of the batch" in str(full.value)


def test_e2e_a_given_basis_is_uploaded_as_before():
    stack = sc.e2e_mixed()[:8]
    given = canonical_basis(stack)
    e2e_check(solve_batch, stack, (0, 7), basis=given)
    items = sc.e2e_ragged()
    e2e_check(solve_ragged, items, (0, 19), basis=ragged_canonical_basis(items))
    # a given basis is not checked: a spoiled LP solves as the default path solves it
    bad = stack.copy()
    bad[2, 3, 0] = -1.0
    e2e_check(solve_batch, bad, (2,), basis=given)
