"""Problem-form batches on the GPU (lp_problem_set_senses, lp_problem_upload,
lp_problem_duals, lp_problem_vars; BatchEngine / RaggedEngine set_senses(),
upload_problems(), duals(), nvars(); solve_problems, solve_problems_ragged;
csrc/batch.hip k_assemble, k_duals).

Every comparison is exact, byte for byte: the assembled tableaux against
lpsol_amd.problem.assemble_tableaux, the duals against problem_duals on
download(), and solve_problems against the result="solution" call its `path`
names, run on the host-assembled tableaux.  Every solve carries a finite pivot
cap."""
import numpy as np
import pytest

import _problem_cases as pc
from _problem_cases import same_bits
from lpsol_amd import (_lib, assemble_tableaux, problem_columns, problem_duals, solve_batch, solve_lp_batch,
                       solve_lp_ragged, solve_problems, solve_problems_ragged, solve_ragged)
from lpsol_amd import generators as gen

pytestmark = pytest.mark.gpu

CAP = 4096
BIG = (100, 100)        # mixed(100, 100) is 100 x 200: above one CU's LDS, device-placed under "auto"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def problem_engine(P, sense, **kw):
    """an engine sized for the senses, holding the assembled tableaux of P"""
    eng = _lib.BatchEngine(P.shape[0], P.shape[1] - 1, problem_columns(sense, P.shape[2] - 1), **kw)
    eng.set_senses(sense)
    eng.upload_problems(P)
    return eng


def tableau_engine(T, **kw):
    eng = _lib.BatchEngine(T.shape[0], T.shape[1] - 1, T.shape[2] - 1, **kw)
    eng.upload(T)
    return eng


def ragged_shapes(blocks, senses):
    return [(p.shape[0] - 1, problem_columns(s, p.shape[1] - 1)) for p, s in zip(blocks, senses)]


# ---------------------------------------------------------------------------
# 1. k_assemble against the host formula
# ---------------------------------------------------------------------------

def _mixed_blocks(m, ns, B):
    T, sense, _ = pc.stack("mixed", m, ns, range(1, B + 1))
    return pc.block(T, ns), sense


def _eq_blocks():
    T, sense, ns = pc.stack("eq", 5, 4, range(1, 4))
    return pc.block(T, ns), sense


ASSEMBLE = {
    "mixed_3x5_x5": lambda: _mixed_blocks(3, 5, 5),
    "mixed_8x10_x65": lambda: _mixed_blocks(8, 10, 65),     # 65 x 171 lanes: no multiple of 256, 44 workgroups
    "one_by_one_le": lambda: (np.array([[[0.5, -1.0], [2.0, 1.0]]]), np.array([pc.LE], dtype=np.int8)),
    "one_by_one_eq": lambda: (np.array([[[0.5, -1.0], [2.0, 1.0]]]), np.array([pc.EQ], dtype=np.int8)),
    "all_eq_pure_copy": _eq_blocks,
    "mixed_senses": lambda: (np.stack([pc.mixed_sense_block(s)[0] for s in range(1, 8)]),
                             np.array(pc.MIXED_SENSE, dtype=np.int8)),
    "special_cells": lambda: (np.stack([pc.special_block()[0]] * 3), pc.special_block()[1]),
}


@pytest.mark.parametrize("name", list(ASSEMBLE))
def test_assemble_equals_the_host(name):
    P, sense = ASSEMBLE[name]()
    eng = problem_engine(P, sense)
    want = assemble_tableaux(P, sense)
    got = eng.download()
    assert same_bits(got, want)
    assert all(eng.nvars(i) == P.shape[2] - 1 for i in range(P.shape[0]))
    if name == "all_eq_pure_copy":
        assert same_bits(got, P)
    # once more over what is there now: every cell is written, none is left over
    eng.upload(np.full_like(want, 7.0))
    eng.upload_problems(P)
    assert same_bits(eng.download(), want)


# ---------------------------------------------------------------------------
# 2. windows
# ---------------------------------------------------------------------------

def test_window_leaves_the_other_lps_alone_and_resets_its_own():
    P, sense = _mixed_blocks(8, 10, 8)
    fresh, _, _ = pc.stack("mixed", 8, 10, range(101, 104))
    fresh = pc.block(fresh, 10)
    eng = problem_engine(P, sense, log_cap=64)
    assert eng.derive_basis()[1] == -1
    status, npiv, _ = eng.solve(CAP)
    assert (status == _lib.OPTIMAL).all() and (npiv > 0).all()
    T0, basis0, logs0 = eng.download(), eng.get_basis(), [eng.log(i) for i in range(8)]
    eng.upload_problems(fresh, first=2)
    T1, basis1 = eng.download(), eng.get_basis()
    keep = [0, 1, 5, 6, 7]
    assert same_bits(T1[keep], T0[keep]) and same_bits(basis1, basis0)
    assert same_bits(T1[2:5], assemble_tableaux(fresh, sense))
    for i in range(8):      # the records: npiv of the solve outside the window, reset inside it
        assert same_bits(eng.log(i), logs0[i] if i in keep else np.zeros((0, 2), dtype=np.int64))
    # a re-uploaded LP solves from scratch, as on an engine of its own
    ref = tableau_engine(assemble_tableaux(fresh, sense), log_cap=64)
    ref.derive_basis()
    rs, rn, rd = ref.solve(CAP)
    assert eng.derive_basis(first=2, count=3)[1] == -1
    status, npiv, nstd = eng.solve(CAP)
    assert same_bits(status[2:5], rs) and same_bits(npiv[2:5], rn) and same_bits(nstd[2:5], rd)
    assert (npiv[keep] == 0).all() and (status[keep] == _lib.OPTIMAL).all()
    assert same_bits(eng.download(2, 3), ref.download()) and same_bits(eng.get_basis()[2:5], ref.get_basis())
    for k in range(3):
        assert same_bits(eng.log(2 + k), ref.log(k))


# ---------------------------------------------------------------------------
# 3. ragged batches
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged():
    blocks, senses = pc.ragged_blocks()
    return blocks, senses, assemble_tableaux(blocks, senses)


def test_ragged_windows(ragged):
    blocks, senses, want = ragged
    shapes = ragged_shapes(blocks, senses)
    eng = _lib.RaggedEngine(shapes)
    eng.set_senses(senses)
    for i, (p, s) in enumerate(zip(blocks, senses)):
        assert eng.nvars(i) == p.shape[1] - 1 == shapes[i][1] - int(np.count_nonzero(s != pc.EQ))
    marks = [np.full((m + 1, n + 1), 7.0 + i) for i, (m, n) in enumerate(shapes)]
    for first, count in pc.RAGGED_WINDOWS:
        eng.upload(marks)
        eng.upload_problems(blocks[first:first + count], first=first)
        got = eng.download()
        for i in range(len(shapes)):
            inside = first <= i < first + count
            assert same_bits(got[i], want[i] if inside else marks[i]), (first, count, i)


# ---------------------------------------------------------------------------
# 4. placement and teams
# ---------------------------------------------------------------------------

def _solve_all(eng):
    assert eng.derive_basis()[1] == -1
    return eng.solve(CAP)


def test_device_placed_batch():
    P, sense = _mixed_blocks(*BIG, 3)
    want = assemble_tableaux(P, sense)
    eng = problem_engine(P, sense, place="auto")
    assert eng.placement(0) == "device"
    assert same_bits(eng.download(), want)
    ref = tableau_engine(want, place="auto")
    for a, b in zip(_solve_all(eng), _solve_all(ref)):
        assert same_bits(a, b)
    assert same_bits(eng.download(), ref.download()) and same_bits(eng.get_basis(), ref.get_basis())
    assert same_bits(eng.duals(), np.stack([problem_duals(T, sense, BIG[1]) for T in ref.download()]))


def test_teamed_batch_after_a_teamed_solve():
    first, sense, ns = pc.stack("mixed", *BIG, (2, 3, 4))
    fresh, _, _ = pc.stack("mixed", *BIG, (5, 6, 7))
    kw = dict(place="device", team=2)
    eng = problem_engine(pc.block(first, ns), sense, **kw)
    assert eng.team_of(0) == 2
    status, npiv, _ = _solve_all(eng)       # wherever a teamed solve leaves the current tableau
    assert (status == _lib.OPTIMAL).all() and (npiv % 2 == 1).any()
    ref = tableau_engine(first, **kw)
    _solve_all(ref)
    assert same_bits(eng.download(), ref.download())
    eng.upload_problems(pc.block(fresh, ns))
    ref.upload(fresh)
    assert same_bits(eng.download(), fresh)
    for a, b in zip(_solve_all(eng), _solve_all(ref)):
        assert same_bits(a, b)
    assert same_bits(eng.download(), ref.download()) and same_bits(eng.get_basis(), ref.get_basis())


# ---------------------------------------------------------------------------
# 5. refusals on a live batch
# ---------------------------------------------------------------------------

def test_refusals_on_a_live_batch():
    lib = _lib.load()
    P, sense = _mixed_blocks(3, 5, 4)
    eng = _lib.BatchEngine(4, 3, 8, log_cap=8)
    # before any senses
    with pytest.raises(ValueError, match="no senses attached"):
        eng.upload_problems(P)
    with pytest.raises(ValueError, match="no senses attached"):
        eng.duals()
    assert lib.lp_problem_upload(eng.h, 0, 4, _lib._ptr(P)) == _lib.BAD_ARG
    assert b"no senses attached" in lib.lp_batch_last_error(eng.h)
    ns = np.zeros(1, dtype=np.int64)
    assert lib.lp_problem_vars(eng.h, 0, ns.ctypes.data_as(_lib._P64)) == _lib.BAD_ARG
    assert not eng.download().any()
    eng.set_senses(sense)
    eng.upload_problems(P)
    want = assemble_tableaux(P, sense)
    # a bad sense value names the row and changes nothing
    bad = np.array([0, 0, 5], dtype=np.int8)
    assert lib.lp_problem_set_senses(eng.h, bad.ctypes.data_as(_lib._P8)) == _lib.BAD_ARG
    assert b"row 2" in lib.lp_batch_last_error(eng.h) and b"sense 5" in lib.lp_batch_last_error(eng.h)
    assert eng.nvars(3) == 5
    eng.upload(np.zeros_like(want))
    eng.upload_problems(P)                  # still under the senses attached before
    assert same_bits(eng.download(), want)
    # windows out of bounds, and the empty one
    for first in (-1, 1, 5):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.upload_problems(P, first=first)
    for first, count in ((-1, 2), (3, 2), (5, 0), (0, -1)):
        with pytest.raises(ValueError, match="out of bounds"):
            eng.duals(first, count)
    assert lib.lp_problem_upload(eng.h, 0, 2, None) == _lib.BAD_ARG
    assert b"NULL" in lib.lp_batch_last_error(eng.h)
    eng.derive_basis()
    eng.solve(CAP)
    solved, log0 = eng.download(), eng.log(0)
    assert len(log0) > 0
    assert lib.lp_problem_upload(eng.h, 4, 0, None) == _lib.PIVOTED
    assert lib.lp_problem_upload(eng.h, 0, 0, _lib._ptr(P)) == _lib.PIVOTED
    assert eng.duals(4, 0).shape == (0, 3)
    assert same_bits(eng.download(), solved) and same_bits(eng.log(0), log0)
    # detached: refused again
    eng.set_senses(None)
    with pytest.raises(ValueError, match="no senses attached"):
        eng.upload_problems(P)
    # k >= n leaves no structural variable
    small = _lib.BatchEngine(2, 3, 3)
    with pytest.raises(ValueError, match="no structural variable"):
        small.set_senses(["<=", "<=", ">="])
    small.set_senses(["<=", "==", ">="])
    assert small.nvars(1) == 1
    # a ragged batch names the LP as well
    rag = _lib.RaggedEngine([(2, 4), (3, 5)])
    bad = np.array([0, 1, 3, 0, 0], dtype=np.int8)
    assert lib.lp_problem_set_senses(rag.h, bad.ctypes.data_as(_lib._P8)) == _lib.BAD_ARG
    assert b"LP 1, row 0" in lib.lp_batch_last_error(rag.h)
    with pytest.raises(ValueError, match="LP 0.*no structural variable"):
        _lib.RaggedEngine([(2, 2), (3, 5)]).set_senses([[0, 1], [2, 2, 2]])


# ---------------------------------------------------------------------------
# 6. k_duals against the host formula
# ---------------------------------------------------------------------------

def duals_check(eng, sense, ns, windows=((1, 2),)):
    """duals() of the whole batch and of the windows against problem_duals on download()"""
    T = eng.download()
    want = np.stack([problem_duals(t, sense, ns) for t in T])
    got = eng.duals()
    assert same_bits(got, want)
    eq = np.asarray(sense) == pc.EQ
    assert (pc.bits(got[:, eq]) == pc.QNAN_BITS).all() and not np.isnan(got[:, ~eq]).any()
    for first, count in windows:
        assert same_bits(eng.duals(first, count), want[first:first + count])
    return got


def test_duals_after_solve():
    P, sense = _mixed_blocks(8, 10, 16)
    eng = problem_engine(P, sense)
    duals_check(eng, sense, 10)             # as uploaded: minus the zero costs of the slacks
    status, _, _ = _solve_all(eng)
    assert (status == _lib.OPTIMAL).all()
    y = duals_check(eng, sense, 10, windows=((0, 1), (15, 1), (3, 5)))
    assert (y <= 1e-9).all() and (y < 0).any()
    z = eng.objective()
    assert np.allclose(np.einsum("bi,bi->b", P[:, 1:, 0], y), z, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", ["ge", "neg"])
def test_duals_after_solve_lp(kind):
    T, sense, ns = pc.stack(kind, 8, 10, range(1, 9))
    eng = problem_engine(pc.block(T, ns), sense)
    status, stage, rows, ninit, _, _ = eng.solve_lp(CAP)
    assert (status == _lib.OPTIMAL).all() and (ninit > 0).any()
    y = duals_check(eng, sense, ns, windows=((0, 8), (7, 1), (2, 3)))
    le = sense == pc.LE
    assert (y[:, le] <= 1e-9).all() and (y[:, ~le] >= -1e-9).all()


def test_duals_with_a_dropped_row_and_an_infeasible_lp():
    P = np.stack([pc.dependent_block(s)[0] for s in range(1, 5)])
    sense = pc.dependent_block(1)[1]
    eng = problem_engine(P, sense)
    status, stage, rows, _, _, _ = eng.solve_lp(CAP)
    assert (rows == 3).all() and (status == _lib.OPTIMAL).all()    # phase 1 dropped the repeated == row
    duals_check(eng, sense, P.shape[2] - 1)
    P, sense = pc.infeasible_block()
    eng = problem_engine(np.stack([P] * 3), sense)
    status, stage, _, _, _, _ = eng.solve_lp(CAP)
    assert (status == _lib.INFEASIBLE).all() and (stage == _lib.STAGE_ARTIFICIAL).all()
    duals_check(eng, sense, 2)


def test_duals_on_a_ragged_batch():
    shapes = pc.E2E_SHAPES
    blocks, senses = pc.ragged_blocks(shapes, seed0=500)
    eng = _lib.RaggedEngine(ragged_shapes(blocks, senses))
    eng.set_senses(senses)
    eng.upload_problems(blocks)
    eng.solve_lp(CAP)           # whatever each LP's outcome: the duals are a read of the stored tableau
    T = eng.download()
    want = [problem_duals(t, s, p.shape[1] - 1) for t, s, p in zip(T, senses, blocks)]
    got = eng.duals()
    assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want))
    for first, count in ((0, 1), (len(shapes) - 1, 1), (2, 3), (5, 7)):
        part = eng.duals(first, count)
        assert len(part) == count and all(same_bits(g, w) for g, w in zip(part, want[first:first + count]))


# ---------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------

def slack_of(x, sense, ns):
    rows = np.nonzero(np.asarray(sense) != pc.EQ)[0]
    out = np.zeros(len(sense))
    out[rows] = x[ns + np.arange(len(rows))]
    return out


def e2e_check(res, ref, T, sense, ns, path):
    assert res.path == path and len(res) == len(T)
    assert same_bits(res.status_code, ref.status_code) and res.status == ref.status
    if path == "plain":
        assert not res.stage.any() and not res.ninit.any() and (res.rows == T.shape[1] - 1).all()
    else:
        assert same_bits(res.stage, ref.stage) and same_bits(res.rows, ref.rows) and same_bits(res.ninit, ref.ninit)
    assert same_bits(res.npiv, ref.npiv) and same_bits(res.nstd, ref.nstd)
    assert same_bits(res.objective, ref.objective) and same_bits(res.basis, ref.basis)
    assert same_bits(res.x, np.ascontiguousarray(ref.x[:, :ns]))
    assert same_bits(res.slack, np.stack([slack_of(x, sense, ns) for x in ref.x]))
    want_y = np.stack([problem_duals(res.tableau(i).toArray(), sense, ns) for i in range(len(T))])
    assert same_bits(res.y, want_y)
    for i in (0, len(T) - 1):
        assert same_bits(res.tableau(i).toArray(), ref.tableau(i).toArray())


E2E = {     # kind, (m, ns), seeds, place, path
    "plain": ("mixed", (8, 10), range(1, 17), "lds", "plain"),
    "neg": ("neg", (8, 10), range(1, 9), "lds", "twophase"),
    "ge": ("ge", (8, 10), range(1, 9), "lds", "twophase"),
    "ge_phased": ("ge", (81, 81), (1, 2), "auto", "twophase"),
}


@pytest.mark.parametrize("name", list(E2E))
def test_solve_problems_end_to_end(name):
    kind, (m, ns), seeds, place, path = E2E[name]
    T, sense, ns = pc.stack(kind, m, ns, seeds)
    c, A, b = pc.parts(T, ns)
    want = assemble_tableaux(pc.block(T, ns), sense)
    res = solve_problems(c, A, b, None if kind in ("mixed", "neg") else sense, max_pivots=CAP, place=place,
                         log_cap=16)
    if path == "plain":
        ref = solve_batch(want, max_pivots=CAP, place=place, result="solution", log_cap=16)
    else:
        ref = solve_lp_batch(want, max_pivots=CAP, place=place, result="solution", log_cap=16)
    if name == "ge_phased":
        assert res._engine.phased_placement(0) == "device"
    assert (res.status_code == _lib.OPTIMAL).all()
    e2e_check(res, ref, T, sense, ns, path)
    assert same_bits(res.log(0), ref.log(0))
    if path == "twophase":
        assert same_bits(res.init_log(0), ref.init_log(0))


@pytest.mark.parametrize("path", ["plain", "twophase"])
def test_solve_problems_ragged_end_to_end(path):
    kind = "mixed" if path == "plain" else "ge"
    lps = [pc.lp(kind, m, ns, 100 + i) for i, (m, ns) in enumerate(pc.E2E_SHAPES)]
    problems = [(*pc.parts(T, ns), None if path == "plain" else s) for T, s, ns in lps]
    want = assemble_tableaux([pc.block(T, ns) for T, _, ns in lps], [s for _, s, _ in lps])
    res = solve_problems_ragged(problems, max_pivots=CAP)
    ref = (solve_ragged if path == "plain" else solve_lp_ragged)(want, max_pivots=CAP, result="solution")
    assert res.path == path and same_bits(res.status_code, ref.status_code)
    if path == "twophase":
        assert same_bits(res.stage, ref.stage) and same_bits(res.rows, ref.rows) and same_bits(res.ninit, ref.ninit)
    else:
        assert not res.stage.any() and not res.ninit.any() and res.rows.tolist() == [m for m, _ in pc.E2E_SHAPES]
    assert same_bits(res.npiv, ref.npiv) and same_bits(res.nstd, ref.nstd) and same_bits(res.objective, ref.objective)
    for i, (T, s, ns) in enumerate(lps):
        assert same_bits(res.basis[i], ref.basis[i])
        assert same_bits(res.x[i], np.ascontiguousarray(ref.x[i][:ns]))
        assert same_bits(res.slack[i], slack_of(ref.x[i], s, ns))
        assert same_bits(res.y[i], problem_duals(res.tableau(i).toArray(), s, ns))
