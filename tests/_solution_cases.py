"""Shared inputs and helpers of the batch-solution tests
(test_solution_cases_cpu.py, test_gpu_batch_solution.py): hand-made LPs for the
device's canonical scan (lp_solution_canonical), each with the basis and the flags
it must give written out, the stacks at the scan's wave and workgroup edges,
and the host statements both calls are compared with: lpsol_amd.batch._canonical
for the scan, lpsol_amd.batch.solution_x for the gather (lp_solution_gather).
A plain module: no fixtures, no GPU."""
import numpy as np

import _twophase_cases as tc
from lpsol_amd import generators as gen
from lpsol_amd.batch import _canonical, solution_x

NAN = float("nan")
M, N, NS = 3, 5, 2          # the hand-made LPs: mixed(3, 2), slack j = 2 + i basic for row i
NEG_B, NO_COLUMN = 1, 2     # the flag bits of lp_solution_canonical


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# the host statement of the scan
# ---------------------------------------------------------------------------

def host_canonical(stack):
    """-> (basis int32 [B, m], flags int32 [B], first_bad) of a [B, m+1, n+1]
    stack: _canonical's basis, bit 0 where some b_r < 0.0, bit 1 where some
    row has no basic column, and the first LP with a flag (or -1)"""
    stack = np.asarray(stack, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        basis, bad = _canonical(stack)
        flags = (NEG_B * np.any(stack[:, 1:, 0] < 0.0, axis=1) + NO_COLUMN * np.any(basis < 0, axis=1)).astype(np.int32)
    assert np.array_equal(bad, flags != 0)
    return basis, flags, (int(np.argmax(bad)) if bad.any() else -1)


def host_canonical_list(items):
    """host_canonical LP by LP for a ragged list -> (list of bases, flags, first_bad)"""
    got = [host_canonical(T[None]) for T in items]
    flags = np.array([g[1][0] for g in got], dtype=np.int32)
    bad = np.nonzero(flags)[0]
    return [g[0][0] for g in got], flags, (int(bad[0]) if len(bad) else -1)


def host_x(stack, basis):
    """solution_x per LP -> [B, n]"""
    return np.stack([solution_x(T, b) for T, b in zip(stack, basis)])


# ---------------------------------------------------------------------------
# hand-made scan cases on a 3 x 5 LP
# ---------------------------------------------------------------------------

def plain(seed):
    """a canonical neighbour: basis [2, 3, 4], no flag"""
    return gen.tableau("mixed", M, NS, seed)


def _column(T, j, entries, cost):
    T[0, 1 + j] = cost
    T[1:, 1 + j] = entries


def _hand():
    """(name, LP, basis, flags): the middle LP of each stack"""
    out = []

    def case(name, basis, flags, edit):
        T = plain(10)
        edit(T)
        out.append((name, T, basis, flags))

    # structural column 1 is a unit column of row 2 as well as slack 4: the lowest wins
    case("two_unit_columns_lowest_wins", [2, 3, 1], 0, lambda T: _column(T, 1, [0.0, 0.0, 1.0], 0.0))
    # a unit column below the slack, but its cost is not zero: the slack keeps the row
    case("unit_column_cost_nonzero", [2, 3, 4], 0, lambda T: _column(T, 0, [0.0, 1.0, 0.0], -1.0))
    case("unit_column_cost_negative_zero", [2, 0, 4], 0, lambda T: _column(T, 0, [0.0, 1.0, 0.0], -0.0))
    case("single_nonzero_is_two", [2, 3, 4], 0, lambda T: _column(T, 0, [0.0, 2.0, 0.0], 0.0))
    case("two_ones", [2, 3, 4], 0, lambda T: _column(T, 0, [1.0, 1.0, 0.0], 0.0))
    case("one_then_nan", [2, 3, 4], 0, lambda T: _column(T, 0, [1.0, NAN, 0.0], 0.0))
    case("nan_then_one", [2, 3, 4], 0, lambda T: _column(T, 0, [NAN, 0.0, 1.0], 0.0))

    def no_column(T):
        T[2, 1 + NS + 1] = 0.0      # row 1 loses its slack's 1.0: the column is all zero

    case("row_without_basic_column", [2, -1, 4], NO_COLUMN, no_column)

    def slack_is_two(T):
        T[1, 1 + NS] = 2.0

    case("slack_is_two", [-1, 3, 4], NO_COLUMN, slack_is_two)

    def b(value):
        def edit(T):
            T[2, 0] = value
        return edit

    case("b_negative", [2, 3, 4], NEG_B, b(-1.0))
    case("b_negative_zero", [2, 3, 4], 0, b(-0.0))
    case("b_nan", [2, 3, 4], 0, b(NAN))

    def both(T):
        no_column(T)
        T[3, 0] = -1.0

    case("both_bits", [2, -1, 4], NEG_B | NO_COLUMN, both)
    return out


HAND = _hand()
HAND_NAMES = [h[0] for h in HAND]


def hand_stack(name):
    """-> (stack [3, 4, 6], basis [3, 3], flags [3], first_bad): the case
    between two plain neighbours"""
    _, T, basis, flags = HAND[HAND_NAMES.index(name)]
    stack = np.stack([plain(1), T, plain(2)])
    want = np.array([[2, 3, 4], basis, [2, 3, 4]], dtype=np.int32)
    return stack, want, np.array([0, flags, 0], dtype=np.int32), (1 if flags else -1)


def position_stack(at):
    """five LPs, the both-bits LP at `at` -> (stack, first_bad)"""
    bad = HAND[HAND_NAMES.index("both_bits")][1]
    return np.stack([bad if i == at else plain(20 + i) for i in range(5)]), at


# ---------------------------------------------------------------------------
# generated stacks at the scan's edges, B = 5, three of the LPs spoiled
# ---------------------------------------------------------------------------

EDGE_SHAPES = ([(1, 1), (2, 3), (8, 10)]                # (m, ns): the small end
               + [(3, 59), (3, 60), (3, 61)]            # n + 1 = 63, 64, 65: the wave's width in columns
               + [(63, 4), (64, 4), (65, 4)]            # m = 63, 64, 65: across the row slices
               + [(2, 1100)])                           # n above any workgroup's thread count


def edge_stack(m, ns):
    """mixed_stack(m, ns, 1..5): LP 1 loses the last row's slack (bit 1), LP 2
    gets structural column 0 as a unit column of the last row (it wins over
    the slack), LP 3 a negative b in row 0 (bit 0); LPs 0 and 4 stay plain"""
    T = gen.mixed_stack(m, ns, range(1, 6)).copy()
    T[1, m, 1 + ns + m - 1] = 0.0
    T[2, 0, 1] = 0.0
    T[2, 1:, 1] = 0.0
    T[2, m, 1] = 1.0
    T[3, 1, 0] = -1.0
    return T


def edge_want(m, ns):
    slack = np.arange(ns, ns + m, dtype=np.int32)
    basis = np.tile(slack, (5, 1))
    basis[1, m - 1] = -1
    basis[2, m - 1] = 0
    return basis, np.array([0, NO_COLUMN, 0, NEG_B, 0], dtype=np.int32), 1


def ragged_items():
    """12 LPs, m = 1..12 and ns = 12..1; LP 3 has a negative b, LP 8 a row
    without a basic column"""
    items = [gen.tableau("mixed", m, 13 - m, m).copy() for m in range(1, 13)]
    items[3][2, 0] = -0.5
    m, ns = 9, 4
    items[8][m, 1 + ns + m - 1] = 0.0
    return items


RAGGED_FLAGS = [0, 0, 0, NEG_B, 0, 0, 0, 0, NO_COLUMN, 0, 0, 0]


# ---------------------------------------------------------------------------
# end to end: the inputs of result="solution" against result="full"
# ---------------------------------------------------------------------------

def e2e_mixed():
    """8 x 10 x 64: m = 8, 10 structural columns"""
    return gen.mixed_stack(8, 10, range(1, 65))


def e2e_phase1():
    return np.stack([gen.phase1_lp("ge", 8, 10, s) for s in range(1, 17)])


E2E_SHAPES = [(1 + (3 * i) % 11, 1 + (5 * i) % 7) for i in range(20)]      # (m, ns)


def e2e_ragged():
    """20 canonical LPs of 20 shapes"""
    return [gen.tableau("mixed", m, ns, 100 + i) for i, (m, ns) in enumerate(E2E_SHAPES)]


def e2e_ragged_phase1():
    """20 LPs of the same (m, ns) that need phase 1"""
    return [gen.phase1_lp("ge", m, ns, 100 + i) for i, (m, ns) in enumerate(E2E_SHAPES)]


def dropped_row_lp():
    """the dependent-row LP of _twophase_cases' phase1_failed_zero batch: at
    the default tolerances phase 1 drops its dependent row, so the basis ends
    with a -1 entry past rows[i]"""
    batch = next(b for b in tc.outcome_batches() if b["name"] == "phase1_failed_zero")
    return batch["stack"][3]
