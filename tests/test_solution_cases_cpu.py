"""The inputs of test_gpu_batch_solution.py are what they say they are
(tests/_solution_cases.py): every hand-made scan case and every edge stack
gives, under lpsol_amd.batch._canonical, the basis and the flags written next
to it, and the host statement of the solution gather (solution_x) does what
lp_solution_gather is specified to do.  No GPU."""
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
    assert {63, 64, 65} <= {m for m, _ in sc.EDGE_SHAPES}
    assert {(1, 1), (2, 3), (8, 10)} <= set(sc.EDGE_SHAPES)


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

