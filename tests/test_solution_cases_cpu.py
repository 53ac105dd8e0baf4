"""The inputs of test_gpu_batch_solution.py and
test_gpu_batch_solution_edges.py are what they say they are
(tests/_solution_cases.py): every hand-made scan case and every edge stack
gives, under lpsol_amd.batch._canonical, the basis and the flags written next
to it, the host statement of the solution gather (solution_x) does what
lp_solution_gather is specified to do, and the float64 oracle's statement of a
solve (oracle_solution, report_solution) is what it says.  No GPU."""
import numpy as np
import pytest

import _solution_cases as sc
import _twophase_cases as tc
from lpsol_amd import BatchResult, RaggedResult, solution_x
from lpsol_amd.batch import _canonical, _stack_x, canonical_basis, ragged_canonical_basis


def test_plain_neighbours_are_canonical():
    for seed in (1, 2, 10, 20, 21, 22, 23, 24):
        T = sc.plain(seed)
        assert T.shape == (sc.M + 1, sc.N + 1)
        assert canonical_basis(T[None]).tolist() == [[2, 3, 4]]


@pytest.mark.parametrize("name", sc.HAND_NAMES)
def test_hand_case_gives_its_basis_and_flags(name):
    stack, basis, flags, first_bad = sc.hand_stack(name)
    assert stack.shape == (3, sc.M + 1, sc.N + 1)
    got_basis, got_flags, got_bad = sc.host_canonical(stack)
    assert sc.same_bits(got_basis, basis)
    assert sc.same_bits(got_flags, flags) and got_bad == first_bad
    if first_bad >= 0:
        with pytest.raises(ValueError, match=f"LP {first_bad} of the batch"):
            canonical_basis(stack)


def test_hand_cases_cover_the_list():
    flags = {name: f for name, _, _, f in sc.HAND}
    assert flags["b_negative"] == sc.NEG_B and flags["row_without_basic_column"] == sc.NO_COLUMN
    assert flags["both_bits"] == sc.NEG_B | sc.NO_COLUMN
    assert flags["b_negative_zero"] == flags["b_nan"] == 0
    T = dict((n, t) for n, t, _, _ in sc.HAND)
    assert np.signbit(T["unit_column_cost_negative_zero"][0, 1]) and T["unit_column_cost_negative_zero"][0, 1] == 0.0
    assert np.signbit(T["b_negative_zero"][2, 0]) and np.isnan(T["b_nan"][2, 0])
    assert np.isnan(T["one_then_nan"][2, 1]) and np.isnan(T["nan_then_one"][1, 1])
    assert np.count_nonzero(T["two_ones"][1:, 1] == 1.0) == 2


@pytest.mark.parametrize("at", [0, 2, 4])
def test_position_stacks(at):
    stack, first_bad = sc.position_stack(at)
    _, flags, bad = sc.host_canonical(stack)
    assert bad == first_bad == at and np.count_nonzero(flags) == 1 and flags[at] == 3


@pytest.mark.parametrize("m,ns", sc.EDGE_SHAPES)
def test_edge_stacks(m, ns):
    stack = sc.edge_stack(m, ns)
    assert stack.shape == (5, m + 1, ns + m + 1)
    basis, flags, bad = sc.host_canonical(stack)
    want = sc.edge_want(m, ns)
    assert sc.same_bits(basis, want[0]) and sc.same_bits(flags, want[1]) and bad == want[2]


def test_edge_shapes_reach_the_edges():
    widths = {ns + m + 1 for m, ns in sc.EDGE_SHAPES}
    assert {63, 64, 65} <= widths and max(widths) > 1024
    assert {63, 64, 65} <= {m for m, _ in sc.EDGE_SHAPES}       # the wave's width in rows: all S = 4
    assert {(1, 1), (2, 3), (8, 10)} <= set(sc.EDGE_SHAPES)
    # the row slices' own edges, 16|17 and 128|129, and S = 16 above LDS
    heights = {m for m, _ in sc.EDGE_SHAPES + sc.TALL_SHAPES}
    assert {16, 17, 128, 129} <= heights and max(heights) > 256
    assert {sc.slices(m) for m in heights} == {1, 4, 16}


def test_ragged_items():
    items = sc.ragged_items()
    assert [T.shape for T in items] == [(m + 1, 13 + 1) for m in range(1, 13)]
    basis, flags, bad = sc.host_canonical_list(items)
    assert flags.tolist() == sc.RAGGED_FLAGS and bad == 3
    with pytest.raises(ValueError, match="LP 3 of the batch"):
        ragged_canonical_basis(items)
    items[3][2, 0] = 0.5
    with pytest.raises(ValueError, match="LP 8 of the batch"):
        ragged_canonical_basis(items)


def test_solution_x_is_the_formula():
    T = np.arange(24, dtype=np.float64).reshape(4, 6) + 1.0       # b = 7, 13, 19
    assert solution_x(T, [0, 2, 4]).tolist() == [7.0, 0.0, 13.0, 0.0, 19.0]
    assert solution_x(T, [1, 3, 1]).tolist() == [0.0, 19.0, 0.0, 13.0, 0.0]      # the later row wins
    assert solution_x(T, [-1, 5, 2]).tolist() == [0.0, 0.0, 19.0, 0.0, 0.0]      # -1 and n are skipped
    assert solution_x(T, [4, -1]).tolist() == [0.0, 0.0, 0.0, 0.0, 7.0]          # rows past the basis are not read
    x = solution_x(-T, [-1, -1, -1])
    assert not x.view(np.uint64).any()                                           # +0.0, every bit


def test_stack_x_is_solution_x_per_lp():
    stack = sc.e2e_mixed()[:7]
    basis, _ = _canonical(stack)
    basis[1, 3] = basis[1, 5]           # a duplicate
    basis[2, 0] = -1
    basis[3, 7] = stack.shape[2] - 1    # n
    assert sc.same_bits(_stack_x(stack, basis), sc.host_x(stack, basis))


def test_full_results_compute_x_lazily_on_the_host():
    stack = sc.e2e_mixed()[:5]
    basis, _ = _canonical(stack)
    n = np.zeros(5, dtype=np.int64)
    r = BatchResult(None, np.ones(5, dtype=np.int32), n, n, -stack[:, 0, 0], stack, basis)
    assert r._x is None and sc.same_bits(r.x, sc.host_x(stack, basis)) and r.x is r.x
    items = sc.ragged_items()
    bases = sc.host_canonical_list(items)[0]
    rr = RaggedResult(None, np.ones(12, dtype=np.int32), n, n, None, items, bases)
    assert all(sc.same_bits(a, solution_x(T, b)) for a, T, b in zip(rr.x, items, bases))


def test_e2e_inputs():
    assert sc.e2e_mixed().shape == (64, 9, 19) and sc.e2e_phase1().shape == (16, 10, 20)
    assert len(set(sc.E2E_SHAPES)) == 20
    canonical_basis(sc.e2e_mixed())
    ragged_canonical_basis(sc.e2e_ragged())
    assert all(_canonical(T[None])[1][0] for T in sc.e2e_phase1())      # these need phase 1
    assert any(_canonical(T[None])[1][0] for T in sc.e2e_ragged_phase1())


def test_the_dependent_row_lp_drops_a_row():
    T = sc.dropped_row_lp()
    o = tc.report(T, None, tc.PROBE_CAP)
    assert (o["status"], o["stage"]) == (tc.OPTIMAL, tc.PHASE2)
    assert o["rows"] < T.shape[0] - 1 and o["bfs"][o["rows"]:] == [-1] * (T.shape[0] - 1 - o["rows"])



# ---------------------------------------------------------------------------
# the inputs of test_gpu_batch_solution_edges.py
# ---------------------------------------------------------------------------

def test_slices_restate_plan_scan_slices():
    assert [sc.slices(m) for m in (1, 16, 17, 128, 129, 513)] == [1, 1, 4, 4, 16, 16]


@pytest.mark.parametrize("m,ns", sc.TALL_SHAPES)
def test_tall_edge_stacks(m, ns):
    stack = sc.edge_stack(m, ns)
    basis, flags, bad = sc.host_canonical(stack)
    want = sc.edge_want(m, ns)
    assert sc.same_bits(basis, want[0]) and sc.same_bits(flags, want[1]) and bad == want[2]


def test_tall_shapes_reach_the_slice_edges():
    heights = {m for m, _ in sc.TALL_SHAPES}
    assert {16, 17, 128, 129} <= heights and max(heights) > 256
    assert [sc.slices(m) for m, _ in sc.TALL_SHAPES] == [1, 4, 4, 16, 16, 16]
    # where each lies under place="auto": the assertion of the GPU test, without a GPU
    from lpsol_amd import _lib
    auto = _lib.place_code("auto")
    assert [_lib.placed_on_device(auto, m, ns + m) for m, ns in sc.TALL_SHAPES] == [m > 129 for m, _ in sc.TALL_SHAPES]
    assert not any(_lib.placed_too_large(auto, m, ns + m) for m, ns in sc.TALL_SHAPES)


@pytest.mark.parametrize("m", sc.TALL_HAND_M)
@pytest.mark.parametrize("name", sc.TALL_HAND_NAMES)
def test_tall_hand_case_gives_its_basis_and_flags(name, m):
    stack, basis, flags, first_bad = sc.tall_hand_stack(name, m)
    assert stack.shape == (3, m + 1, m + 3)
    got_basis, got_flags, got_bad = sc.host_canonical(stack)
    assert sc.same_bits(got_basis, basis)
    assert sc.same_bits(got_flags, flags) and got_bad == first_bad


@pytest.mark.parametrize("m", sc.TALL_HAND_M)
def test_tall_hand_cases_put_their_entries_in_different_slices(m):
    S = sc.slices(m)
    assert S == {20: 4, 130: 16}[m]
    T = {name: t for name, t, _, _ in sc.TALL_HAND[m]}
    assert [name for name, *_ in sc.TALL_HAND[m]] == sc.TALL_HAND_NAMES

    def slices_of(name, test):
        return [int(i) % S for i in np.nonzero(test(T[name][1:, 1]))[0]]

    one, nan = (lambda c: c == 1.0), np.isnan
    assert slices_of("one_first_slice_one_last_slice", one) == [0, S - 1]
    assert slices_of("one_last_slice_nan_first_slice", one) == [S - 1]
    assert slices_of("one_last_slice_nan_first_slice", nan) == [0]
    assert slices_of("one_first_slice_nan_last_slice", one) == [0]
    assert slices_of("one_first_slice_nan_last_slice", nan) == [S - 1]
    assert slices_of("one_second_slice_two_last_slice", one) == [1]
    assert slices_of("one_second_slice_two_last_slice", lambda c: c == 2.0) == [S - 1]
    for name in sc.TALL_HAND_NAMES[:6]:
        assert T[name][0, 1] == 0.0, name                       # the cost never decides
    for name in sc.TALL_HAND_NAMES[:4]:
        assert np.count_nonzero(T[name][1:, 1]) == 2, name      # NaN counts
    last = T["unit_last_row_beats_the_slack"]
    assert np.nonzero(last[1:, 1])[0].tolist() == [m - 1] and last[m, 1] == last[m, 1 + 2 + m - 1] == 1.0
    assert slices_of("unit_last_slice_beats_the_slack", lambda c: c != 0.0) == [S - 1]
    neg = T["b_negative_last_slice"][1:, 0]
    assert [int(i) % S for i in np.nonzero(neg < 0.0)[0]] == [S - 1]
    basis = {name: b for name, _, b, _ in sc.TALL_HAND[m]}
    assert [r % S for r, c in enumerate(basis["row_without_basic_column_last_slice"]) if c == -1] == [S - 1]


def test_window_items():
    items = sc.window_items()
    assert [T.shape[0] - 1 for T in items] == [1, 129, 2, 17, 3]
    _, flags, bad = sc.host_canonical_list(items)
    assert flags.tolist() == [0, 0, 0, sc.NO_COLUMN, 0] and bad == sc.WINDOW_BAD
    # the windows of the GPU test: S = 16, 4, 1 and 16
    assert [sc.slices(max(T.shape[0] - 1 for T in items[a:b])) for a, b in ((0, 5), (2, 5), (2, 3), (1, 2))] \
        == [16, 4, 1, 16]
    assert not sc.host_canonical_list(sc.placed_items())[1].any()


def test_many_ragged():
    items, clean = sc.many_ragged(), sc.many_ragged(spoiled=False)
    assert len(items) == sc.MANY and sum(T.size for T in items) == 42000
    assert len({T.shape for T in items}) == 10
    basis, flags, bad = sc.host_canonical_list(items)
    assert sc.same_bits(flags, sc.many_flags()) and bad == sc.MANY_BAD[0]
    assert len(sc.MANY_BAD) == 20 and sc.MANY_BAD == sorted(sc.MANY_BAD) and sc.MANY_BAD[-1] == sc.MANY - 1
    assert np.count_nonzero(flags == sc.NEG_B) == np.count_nonzero(flags == sc.NO_COLUMN) == 10
    assert not sc.host_canonical_list(clean)[1].any()
    # LP 128's column 0 is lane 0 of a wave of the whole batch's scan
    lane = np.concatenate([[0], np.cumsum([T.shape[1] for T in items])])
    assert 128 in sc.MANY_BAD and lane[128] % 64 == 0 and lane[128] > 0
    # more than 64 LPs in every window: plan_lane_lp halves more than 6 times
    first, count = sc.MANY_WINDOWS[0]
    assert first - 1 in sc.MANY_BAD and first + 1 in sc.MANY_BAD and first not in sc.MANY_BAD
    assert sc.MANY_WINDOWS[1] == (sc.MANY - 1, 1)


def test_many_uniform():
    stack = sc.many_uniform()
    assert stack.shape == (sc.UNIFORM_MANY, sc.M + 1, sc.N + 1)
    _, flags, bad = sc.host_canonical(stack)
    assert np.nonzero(flags)[0].tolist() == sc.UNIFORM_BAD and bad == 0
    assert (flags[sc.UNIFORM_BAD] == (sc.NEG_B | sc.NO_COLUMN)).all()
    inside = [[i for i in sc.UNIFORM_BAD if a <= i < a + k] for a, k in sc.UNIFORM_WINDOWS]
    assert inside == [[], [1023], [1023, 1024], sc.UNIFORM_BAD]
    _, flags, bad = sc.host_canonical(sc.all_bad_uniform())
    assert flags.tolist() == [sc.NEG_B, sc.NO_COLUMN] * (sc.UNIFORM_MANY // 2) and bad == 0


def test_oracle_solution_on_a_hand_made_lp():
    # min -x0 - x1 with x0 <= 2, x1 <= 3: two pivots, x = (2, 3), z = -5
    T = np.array([[0.0, -1.0, -1.0, 0.0, 0.0],
                  [2.0, 1.0, 0.0, 1.0, 0.0],
                  [3.0, 0.0, 1.0, 0.0, 1.0]])
    st, basis, x, z = sc.oracle_solution(T, [2, 3], 16)
    assert st == tc.OPTIMAL and sorted(basis.tolist()) == [0, 1] and basis.dtype == np.int32
    assert x.tolist() == [2.0, 3.0, 0.0, 0.0] and z == -5.0
    # the cap binds after one pivot; the fixed-rule run makes exactly one
    st, basis, x, z = sc.oracle_solution(T, [2, 3], 1)
    assert st == tc.CAP_REACHED and sorted(basis.tolist()) in ([0, 3], [1, 2]) and z in (-2.0, -3.0)
    st1, basis1, x1, z1 = sc.oracle_solution(T, [2, 3], 16, rule=0, steps=1)
    assert st1 == tc.PIVOTED and np.count_nonzero(x1[:2]) == 1 and z1 in (-2.0, -3.0)
    # entries outside [0, n) are skipped and leave +0.0, every bit
    st, basis, x, z = sc.oracle_solution(T, [-1, 4], 0)
    assert basis.tolist() == [-1, 4] and not x.view(np.uint64).any()


def test_oracle_solution_agrees_with_the_host_formula():
    """two statements of getBFS written apart: the oracle's loop and solution_x"""
    from oracle.f64 import F64Tableau
    stack = sc.e2e_mixed()[:6]
    start = canonical_basis(stack)
    for T, b0 in zip(stack, start):
        st, basis, x, z = sc.oracle_solution(T, b0, 4096)
        o = F64Tableau(T)
        o.solve(cap=4096, logcap=4096)
        assert st == tc.OPTIMAL and sc.same_bits(x, solution_x(o.T, basis)) and z == -o.T[0, 0]
        assert sc.same_bits(basis, _canonical(o.T[None])[0][0])      # the final tableau is canonical on its basis


def test_report_solution_skips_the_dropped_rows():
    T = sc.dropped_row_lp()
    st, stage, rows, basis, x, z = sc.report_solution(T, 4096)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    assert (st, stage) == (tc.OPTIMAL, tc.PHASE2) and rows < m and (basis[rows:] == -1).all()
    o = tc.report(T, None, 4096)
    assert sc.same_bits(x, solution_x(o["T"], basis[:rows])) and len(x) == n and z == -o["T"][0, 0]
    for T in sc.phased_mix()[:4]:
        st, stage, rows, basis, x, z = sc.report_solution(T, 4096)
        assert (st, stage, rows) == (tc.OPTIMAL, tc.PHASE2, T.shape[0] - 1) and x.any()


def test_the_oracle_stays_below_the_cap():
    """the pivot counts the GPU tests lean on: odd for the teamed LPs"""
    from oracle.f64 import F64Tableau

    def pivots(T):
        st, log, _ = F64Tableau(T).solve(cap=4096, logcap=4096)
        assert st == tc.OPTIMAL
        return len(log)
    assert [pivots(T) for T in sc.teamed_stack()] == [235, 303]
    assert [pivots(T) for T in sc.s16_stack()] == [391, 465]
    assert all(pivots(T) < 4096 for T in sc.placed_items())
    assert all(pivots(T) < 64 for T in sc.many_ragged(spoiled=False))
