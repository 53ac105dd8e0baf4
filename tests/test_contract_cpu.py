"""The inputs of the contract tests, checked on the CPU oracle alone (no GPU).

test_gpu_batch_contract.py and test_gpu_engine_contract.py compare the kernels
with oracle/lp_f64.c on the inputs of tests/_contract_cases.py.  Such a
comparison shows something only if the input makes the oracle do what the test
is about, so every condition on the inputs is asserted here:

  * the hand-built cases give the literal status, log and counts written in
    the table, alone and embedded at every shape and placement;
  * the dirty stacks pivot, end in all three ways and never reach the cap;
  * the scaled stacks keep the unscaled log and stay finite;
  * each lp_tol field, set alone, changes the oracle's result on every input a
    GPU test runs it on -- and a result computed with two fields swapped is
    told apart by the comparison the GPU tests use.
"""
import numpy as np
import pytest

import _contract_cases as cc
from lpsol_amd import generators as gen
from oracle.f64 import F64Tableau


# ---------------------------------------------------------------------------
# same_values
# ---------------------------------------------------------------------------

def test_same_values_signs_infinities_and_nan_patterns():
    a = np.array([0.0, 1.0, np.inf, np.nan])
    assert cc.same_values(a, a.copy())
    assert not cc.same_values(a, np.array([-0.0, 1.0, np.inf, np.nan]))
    assert not cc.same_values(a, np.array([0.0, 1.0, -np.inf, np.nan]))
    assert not cc.same_values(a, np.array([0.0, 1.0, np.inf, 2.0]))
    assert not cc.same_values(a, np.array([0.0, np.nan, np.inf, np.nan]))
    assert not cc.same_values(a, a.reshape(2, 2))
    assert not cc.same_values(a, np.array([0.0, np.nextafter(1.0, 2.0), np.inf, np.nan]))
    # the host's default NaN and the device's differ in the sign bit
    pos = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)
    neg = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)
    assert pos.tobytes() != neg.tobytes() and not cc.same_bits(pos, neg)
    assert cc.same_values(pos, neg)


# ---------------------------------------------------------------------------
# hand-built cases: the literal table
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_case_gives_the_tables_literals(name):
    c = cc.case(name)
    with np.errstate(all="ignore"):
        r = cc.oracle_solve(c["T"], c["cap"], c["tol"])
    assert (r["status"], r["log"], r["nstd"]) == (c["status"], c["log"], c["nstd"])
    assert cc.same_values(r["T"], c["T"]) == c["untouched"]


def test_table_holds_every_status_and_an_untouched_tableau():
    assert {c["status"] for c in cc.CASES} == {cc.OPTIMAL, cc.UNBOUNDED, cc.CAP_REACHED,
                                               cc.OBJ_INCREASED}
    assert cc.case("zero_pivot")["nstd"] == 5 and cc.case("zero_pivot")["untouched"]
    assert cc.case("neg_b")["nstd"] == 1


@pytest.mark.parametrize("m,n,row_at", cc.EMBEDDINGS)
@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_embedded_case_gives_the_mapped_log(name, m, n, row_at):
    """the oracle's log on the embedded LP is the small LP's log mapped through
    row_at (zero_pivot: see mapped_log -- with pivot = -1 an added all-zero row
    is as eligible as the case's, so row 0 leaves at (65, 66, 70) too)"""
    c = cc.case(name)
    T = cc.embed(c, m, n, row_at)
    assert T.shape == (m + 1, n + 1)
    with np.errstate(all="ignore"):
        r = cc.oracle_solve(T, c["cap"], c["tol"])
    assert (r["status"], r["nstd"]) == (c["status"], c["nstd"])
    assert r["log"] == cc.mapped_log(c, row_at)
    assert cc.same_values(r["T"], T) == c["untouched"]
    # the embedding leaves the case's own cells where they were
    assert cc.same_values(T[list(row_at), :c["T"].shape[1]], c["T"][1:])
    assert cc.same_values(T[0, :c["T"].shape[1]], c["T"][0])


def test_embeddings_cover_both_kernels():
    elems = [(m + 1) * (n + 1) for m, n, _ in cc.EMBEDDINGS]
    assert elems == [30, 171, 2911, 2911] and elems[1] <= 2048 < elems[2]
    assert cc.EMBEDDINGS[3][2] == (65, 66, 70)


# ---------------------------------------------------------------------------
# dirty stacks
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dirty_results():
    out = {}
    with np.errstate(all="ignore"):
        for m, ns, k in cc.DIRTY_SHAPES:
            S = cc.dirty_stack(m, ns, k, range(1, 201))
            out[m, ns, k] = [cc.oracle_solve(T, cc.DIRTY_CAP) for T in S]
    return out


# (status counts, share with >= 1 pivot, share with >= 4, most pivots) over seeds 1..200
DIRTY_MEASURED = {
    (8, 10, 2): ((193, 4, 3), 0.965, 0.78, 12),
    (31, 32, 4): ((190, 9, 1), 0.985, 0.91, 59),
    (40, 40, 6): ((194, 5, 1), 0.975, 0.85, 88),
}


@pytest.mark.parametrize("shape", cc.DIRTY_SHAPES)
def test_dirty_stack_conditions(dirty_results, shape):
    rs = dirty_results[shape]
    st = [r["status"] for r in rs]
    npiv = np.array([r["npiv"] for r in rs])
    counts = (st.count(cc.OPTIMAL), st.count(cc.UNBOUNDED), st.count(cc.OBJ_INCREASED))
    assert sum(counts) == 200                               # no LP reaches the cap
    assert (counts, (npiv >= 1).mean(), (npiv >= 4).mean(), npiv.max()) == DIRTY_MEASURED[shape]
    assert min(counts) >= 1 and (npiv >= 1).mean() >= 0.9 and (npiv >= 4).mean() >= 0.7
    assert npiv.max() < cc.DIRTY_CAP


@pytest.mark.parametrize("shape", cc.DIRTY_SHAPES)
def test_dirty_stack_first_64_seeds(dirty_results, shape):
    """the GPU test runs the first 64 seeds of each stack.  Measured: they keep
    the pivot shares (100 / 84 %, 100 / 94 %, 98 / 91 %) and hold optimal and
    unbounded LPs at every shape; objective_increased is among them at 8x10
    only (seed 200's at the two larger shapes lies outside)."""
    rs = dirty_results[shape][:64]
    st = {r["status"] for r in rs}
    npiv = np.array([r["npiv"] for r in rs])
    assert (npiv >= 1).mean() >= 0.9 and (npiv >= 4).mean() >= 0.7
    assert cc.CAP_REACHED not in st and {cc.OPTIMAL, cc.UNBOUNDED} <= st
    assert (cc.OBJ_INCREASED in st) == (shape == (8, 10, 2))
    # the dirt is there: non-finite cells in the inputs and in the results
    S = cc.dirty_stack(*shape, range(1, 65))
    assert np.isnan(S).any() and np.isinf(S).any()
    assert any(not np.isfinite(r["T"]).all() for r in rs)


def test_dirty_stack_draw_order():
    """i, then j, then the value's index, k times, from default_rng(1000 + s)"""
    T = gen.tableau("mixed", 8, 10, 3)
    rng = np.random.default_rng(1003)
    for _ in range(2):
        i = rng.integers(0, 9)
        j = rng.integers(0, 19)
        T[i, j] = cc.DIRT[rng.integers(0, 10)]
    assert cc.same_values(cc.dirty_stack(8, 10, 2, [3])[0], T)


# ---------------------------------------------------------------------------
# exponent range
# ---------------------------------------------------------------------------

TINY = np.finfo(np.float64).tiny


@pytest.mark.parametrize("m,ns", cc.SCALED_SHAPES + [(130, 70)])
def test_scaled_rows_keep_the_log_and_stay_finite(m, ns):
    """measured over seeds 1..8: pivot counts 2-9, 33-54, 23-34, 81-180 (and
    167-216 at 130x70); the `down` stacks hold 0-12, 0-102, 0-105, 0-261 and
    0-285 denormal inputs per LP, at least 24 per stack of 8"""
    denormals = 0
    for s in range(1, 9):
        T = gen.tableau("mixed", m, ns, s)
        base = cc.oracle_solve(T, 4096, cc.SCALE_TOL)
        assert base["status"] == cc.OPTIMAL and base["npiv"] >= 2
        for down in (False, True):
            X = cc.scaled(T, s, down)
            assert np.array_equal(X[0], T[0])
            r = cc.oracle_solve(X, 4096, cc.SCALE_TOL)
            assert r["log"] == base["log"] and r["status"] == cc.OPTIMAL
            assert np.isfinite(r["T"]).all()
            if down:
                denormals += int(((np.abs(X) < TINY) & (X != 0.0)).sum())
            else:
                e = np.frexp(X[1:][X[1:] != 0.0])[1]
                assert e.min() < -200 and e.max() > 200        # far outside [2^-6, 2^23]
    assert denormals >= 24


# ---------------------------------------------------------------------------
# tolerance teeth: every (path, input, field) a GPU test uses
# ---------------------------------------------------------------------------

def test_tolerance_values_are_distinct_and_not_the_defaults():
    vals = list(cc.ALL_SIX.values())
    assert len(set(vals)) == 6
    assert cc.ALL_SIX == dict(cost=0.3, cost_tie=0.5, pivot=0.2, zero=0.4, ratio_tie=0.25, stall=1e9)


def _changed(stack, tol, cap=4096):
    return sum(cc.result_differs(cc.oracle_solve(T, cap), cc.oracle_solve(T, cap, tol))
               for T in stack)


# LPs of seeds 1..8 whose result changes, per field in cc.FIELDS order
BATCH_TEETH = {(8, 10): [4, 8, 1, 5, 2], (31, 33): [7, 8, 8, 8, 8], (40, 30): [8, 8, 7, 8, 8]}


@pytest.mark.parametrize("m,ns", list(BATCH_TEETH))
def test_each_field_changes_the_batch_inputs(m, ns):
    stack = gen.mixed_stack(m, ns, range(1, 9))
    got = [_changed(stack, {f: cc.TOL_VALUES[f]}) for f in cc.FIELDS]
    assert got == BATCH_TEETH[m, ns] and min(got) >= 1
    assert _changed(stack, cc.ALL_SIX) == 8
    if (m, ns) != (8, 10):      # zero = 0.4 puts objective_increased on the path
        st = [cc.oracle_solve(T, 4096, dict(zero=0.4))["status"] for T in stack]
        assert st == [cc.OBJ_INCREASED] * 8


def test_stall_inputs():
    """Klee-Minty 8 and its four-wave padding: stall = 1e9 calls every pivot
    stuck, so the rule switches after m + n standard pivots"""
    for T, npiv, nstd in ((gen.klee_minty(8), 89, 24), (cc.km8_padded(), 253, 238)):
        m, n = T.shape[0] - 1, T.shape[1] - 1
        plain = cc.oracle_solve(T, 4096)
        assert (plain["status"], plain["npiv"], plain["nstd"]) == (cc.OPTIMAL, 255, 255)
        r = cc.oracle_solve(T, 4096, dict(stall=cc.STALL))
        assert (r["status"], r["npiv"], r["nstd"]) == (cc.OPTIMAL, npiv, nstd)
        assert nstd == m + n < npiv
        assert cc.result_differs(plain, r)
    assert cc.km8_padded().size == 2079 > 2048


@pytest.mark.parametrize("path", cc.ENGINE_PATHS)
@pytest.mark.parametrize("name,tol", cc.TOL_SETS, ids=cc.TOL_IDS)
def test_each_field_changes_the_engine_inputs(path, name, tol):
    call, rule, k, inputs = cc.engine_plan(path, name)
    assert any(cc.result_differs(cc.oracle_call(call, rule, k, T),
                                 cc.oracle_call(call, rule, k, T, tol)) for T in inputs)


def test_standard_rule_run_does_not_read_cost_on_these_inputs():
    """why engine_plan takes the min-index rule for cost (measured: 40 standard
    pivots of mixed 130x70, seeds 1 and 2, and 12 of tall 6000x8, seeds 1..8,
    are the same with cost = 0.3)"""
    for T, k in ([(gen.tableau("mixed", 130, 70, s), 40) for s in (1, 2)]
                 + [(gen.tableau("tall", 6000, 8, 1), 12)]):
        assert not cc.result_differs(cc.oracle_run(T, 0, k), cc.oracle_run(T, 0, k, dict(cost=0.3)))


@pytest.mark.parametrize("field", cc.SCAN_FIELDS + ["all_six"])
def test_each_field_changes_the_scans(field):
    tol = dict(cc.TOL_SETS)[field]
    T = cc.scan_input()
    plain, _ = cc.scan_walk(T, None)
    walk, _ = cc.scan_walk(T, tol)
    assert len(plain) == len(walk) == 10 and walk != plain


@pytest.mark.parametrize("field", cc.CHECKED_FIELDS + ["all_six"])
def test_checked_pivot_pairs(field):
    """the accepted pivot is one the default lp_tol refuses; the refused one is
    one the default takes (pivot = 0.2 makes its row ineligible) or, where the
    field only widens the band, an eligible row outside it"""
    tol = dict(cc.TOL_SETS)[field]
    T = cc.scan_input()
    acc, ref = cc.checked_pair(T, tol)
    S_tol, S_def = F64Tableau(T, tol).find_all(), F64Tableau(T).find_all()
    assert acc in S_tol and acc not in S_def
    assert ref not in S_tol
    if field in ("pivot", "all_six"):
        assert ref in S_def and 1e-9 < T[1 + ref[0], 1 + ref[1]] <= 0.2
    else:
        assert T[1 + ref[0], 1 + ref[1]] > 1e-9


# ---------------------------------------------------------------------------
# self-check: a kernel that read one lp_tol field for another would be caught
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("field", list(cc.ALL_SIX))
def test_swapped_fields_are_rejected(field):
    """the oracle run with field and SWAP_WITH[field] exchanged stands in for a
    kernel that reads the wrong member of lp_tol: result_differs, the
    comparison of the GPU tests, tells it from the right result"""
    tol = {field: cc.ALL_SIX[field]}
    wrong = cc.swapped(tol, field, cc.SWAP_WITH[field])
    assert wrong[field] != tol[field] and wrong[cc.SWAP_WITH[field]] == tol[field]
    if field == "stall":
        stack = [gen.klee_minty(8)]
    else:
        stack = gen.mixed_stack(31, 33, range(1, 9))
    caught = [cc.result_differs(cc.oracle_solve(T, 4096, tol), cc.oracle_solve(T, 4096, wrong))
              for T in stack]
    assert any(caught)
    # and with all six set, where every field holds a value of its own
    both = cc.swapped(cc.ALL_SIX, field, cc.SWAP_WITH[field])
    stack = [gen.klee_minty(8)] + list(gen.mixed_stack(31, 33, range(1, 9)))
    assert any(cc.result_differs(cc.oracle_solve(T, 4096, cc.ALL_SIX), cc.oracle_solve(T, 4096, both))
               for T in stack)
