"""Shared inputs and helpers of the batch-solution tests
(test_solution_cases_cpu.py, test_gpu_batch_solution.py,
test_gpu_batch_solution_edges.py): hand-made LPs for the
device's canonical scan (lp_solution_canonical), each with the basis and the flags
it must give written out, the stacks at the scan's wave and workgroup edges,
and the host statements both calls are compared with: lpsol_amd.batch._canonical
for the scan, lpsol_amd.batch.solution_x for the gather (lp_solution_gather),
and the float64 oracle's statement of a whole solve (oracle_solution,
report_solution), which uses neither.
A plain module: no fixtures, no GPU."""
import numpy as np

import _twophase_cases as tc
from lpsol_amd import generators as gen
from lpsol_amd.batch import _canonical, solution_x
from oracle.f64 import F64Tableau

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
               + [(63, 4), (64, 4), (65, 4)]            # m = 63, 64, 65: the wave's width in rows (one slice count, S = 4)
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


# ---------------------------------------------------------------------------
# the scan's row slices: wave s of a workgroup reads rows s, s + S, ...
# (plan_scan_slices: S = 1 up to 16 rows, 4 up to 128, 16 above)
# ---------------------------------------------------------------------------

def slices(m):
    """plan_scan_slices, restated"""
    return 1 if m <= 16 else 4 if m <= 128 else 16


# (m, ns) of edge_stack at the slice edges 16|17 and 128|129 and above: 129, 257
# and 513 rows run S = 16; 257 and 513 rows do not fit one CU's LDS
TALL_SHAPES = [(16, 4), (17, 4), (128, 4), (129, 4), (257, 3), (513, 1)]

TALL_HAND_M = (20, 130)         # S = 4 and S = 16; ns = 2, so n = m + 2 and row i's slack is column 2 + i


def _tall_hand(m):
    """(name, LP, basis, flags) on mixed(m, 2), seed 10: _hand()'s edits with
    the entries that matter in different row slices.  row(s, k) is the k-th
    row of slice s."""
    S = slices(m)
    assert S > 1 and 2 * S <= m

    def row(s, k=1):
        return s + k * S

    first, second, last = row(0), row(1), row(S - 1)
    slack = list(range(2, 2 + m))
    out = []

    def case(name, basis, flags, edit):
        T = gen.tableau("mixed", m, 2, 10)
        edit(T)
        out.append((name, T, basis, flags))

    def but(r, c):
        b = list(slack)
        b[r] = c
        return b

    def column(entries, cost=0.0):
        def edit(T):
            T[:, 1] = 0.0
            T[0, 1] = cost
            for r, v in entries.items():
                T[1 + r, 1] = v
        return edit

    # not unit columns: the second entry is in another slice than the 1.0
    case("one_first_slice_one_last_slice", slack, 0, column({first: 1.0, last: 1.0}))
    case("one_last_slice_nan_first_slice", slack, 0, column({last: 1.0, first: NAN}))
    case("one_first_slice_nan_last_slice", slack, 0, column({first: 1.0, last: NAN}))
    case("one_second_slice_two_last_slice", slack, 0, column({second: 1.0, last: 2.0}))
    # unit columns: column 0 is below every slack, so it wins the row
    case("unit_last_row_beats_the_slack", but(m - 1, 0), 0, column({m - 1: 1.0}))
    case("unit_last_slice_beats_the_slack", but(last, 0), 0, column({last: 1.0}))

    def b_negative(T):
        T[1 + last, 0] = -1.0

    case("b_negative_last_slice", slack, NEG_B, b_negative)

    def no_column(T):
        T[1 + last, 1 + 2 + last] = 0.0

    case("row_without_basic_column_last_slice", but(last, -1), NO_COLUMN, no_column)
    return out


TALL_HAND = {m: _tall_hand(m) for m in TALL_HAND_M}
TALL_HAND_NAMES = [h[0] for h in TALL_HAND[TALL_HAND_M[0]]]


def tall_hand_stack(name, m):
    """-> (stack [3, m+1, m+3], basis [3, m], flags [3], first_bad): the case
    between two plain neighbours, as hand_stack"""
    _, T, basis, flags = TALL_HAND[m][TALL_HAND_NAMES.index(name)]
    stack = np.stack([gen.tableau("mixed", m, 2, 1), T, gen.tableau("mixed", m, 2, 2)])
    slack = list(range(2, 2 + m))
    want = np.array([slack, basis, slack], dtype=np.int32)
    return stack, want, np.array([0, flags, 0], dtype=np.int32), (1 if flags else -1)


WINDOW_SHAPES = [(1, 1), (129, 4), (2, 3), (17, 4), (3, 60)]       # (m, ns): a window's S follows its tallest LP
WINDOW_BAD = 3


def window_items():
    """five LPs of 1, 129, 2, 17 and 3 rows; LP 3 loses the slack of its last
    row (row 16: slice 0 of 4 in a window without LP 1, slice 0 of 16 with it)"""
    items = [gen.tableau("mixed", m, ns, 30 + k) for k, (m, ns) in enumerate(WINDOW_SHAPES)]
    m, ns = WINDOW_SHAPES[WINDOW_BAD]
    items[WINDOW_BAD][m, 1 + ns + m - 1] = 0.0
    return items


def placed_items():
    """the five LPs of test_scan_ragged_placed_and_mixed_heights, unspoiled:
    the 100 x 200 one is device-placed under "auto", the others fit LDS"""
    return [gen.tableau("mixed", m, ns, 1 + k)
            for k, (m, ns) in enumerate([(1, 1), (100, 100), (2, 3), (65, 4), (3, 60)])]


# ---------------------------------------------------------------------------
# many LPs in one window
# ---------------------------------------------------------------------------

MANY = 1500
# LP 128 begins on lane 6528 = 102 * 64 of the whole batch's scan; 1499 is the
# last; 699 and 701 lie either side of the window (700, 800)'s first LP
MANY_BAD = [5, 128, 131, 256, 389, 512, 640, 699, 701, 777, 850, 901, 1023, 1024, 1100, 1249, 1250, 1333,
            1420, 1499]
MANY_WINDOWS = [(700, 800), (1499, 1)]


def many_shape(i):
    return 1 + (7 * i) % 5, 1 + (3 * i) % 6


def many_kind(i):
    """the flag LP i of MANY_BAD gets: bit 0 and bit 1 alternate down the list"""
    return (NEG_B, NO_COLUMN)[MANY_BAD.index(i) % 2]


def many_ragged(spoiled=True):
    """1500 canonical LPs of 10 shapes, 42,000 doubles; spoiled: the LPs of
    MANY_BAD get a negative b in their last row (k_canon_scan raises bit 0) or
    lose their last row's slack (k_canon_finish raises bit 1)"""
    items = [gen.tableau("mixed", *many_shape(i), 1000 + i) for i in range(MANY)]
    if spoiled:
        for i in MANY_BAD:
            m, ns = many_shape(i)
            if many_kind(i) == NEG_B:
                items[i][m, 0] = -0.25
            else:
                items[i][m, 1 + ns + m - 1] = 0.0
    return items


def many_flags():
    flags = np.zeros(MANY, dtype=np.int32)
    for i in MANY_BAD:
        flags[i] = many_kind(i)
    return flags


UNIFORM_MANY = 2048
UNIFORM_BAD = [0, 1023, 1024, 2047]
# (first, count): none of the bad LPs, one, two across the middle, all four
UNIFORM_WINDOWS = [(1, 1000), (1000, 24), (1023, 2), (0, 2048)]


def many_uniform():
    """2048 LPs of the 3 x 5 hand shape, the both-bits LP at UNIFORM_BAD"""
    stack = gen.mixed_stack(M, NS, range(1, UNIFORM_MANY + 1)).copy()
    stack[UNIFORM_BAD] = HAND[HAND_NAMES.index("both_bits")][1]
    return stack


def all_bad_uniform():
    """2048 LPs of the 3 x 5 shape, every one bad: a negative b in the even
    LPs, a lost slack in the odd ones, so every workgroup of k_canon_scan and of
    k_canon_finish takes part in the first-bad minimum"""
    stack = gen.mixed_stack(M, NS, range(1, UNIFORM_MANY + 1)).copy()
    stack[0::2, 2, 0] = -1.0
    stack[1::2, 3, 1 + NS + 2] = 0.0
    return stack


# ---------------------------------------------------------------------------
# the float64 oracle's statement of a solve: status, basis, x and z
# ---------------------------------------------------------------------------

def _loop_x(T, basis, rows, n):
    """x of a tableau and its basis, the first `rows` rows ascending"""
    x = [0.0] * n
    for r in range(rows):
        c = int(basis[r])
        if 0 <= c < n:
            x[c] = float(T[1 + r][0])
    return np.array(x, dtype=np.float64)


def oracle_solution(T0, basis0, cap, rule=None, steps=None):
    """Simplex.solve under `cap` (or `steps` pivots of `rule`) by the float64
    oracle on T0, its log replayed onto basis0 -> (status, basis int32 [m], x
    [n], z)"""
    o = F64Tableau(T0)
    if rule is None:
        status, log, _ = o.solve(cap=cap, logcap=max(cap, 1))
    else:
        status, log = o.run(rule, steps)
    b = [int(c) for c in basis0]
    for r, c in log.tolist():
        b[r] = c
    return int(status), np.array(b, dtype=np.int32), _loop_x(o.T, b, o.m, o.n), float(o.objective())


def report_solution(T, cap, tol=None):
    """the same of a two-phase solve, from the reporting oracle's record
    (tc.report): x reads the rows phase 1 kept -> (status, stage, rows, basis
    int32 [m], x [n], z)"""
    o = tc.report(T, tol, cap)
    n = T.shape[1] - 1
    x = _loop_x(o["T"], o["bfs"], o["rows"], n)
    return o["status"], o["stage"], o["rows"], np.array(o["bfs"], dtype=np.int32), x, float(o["objective"])


def teamed_stack():
    """two LPs of 100 x 200: above LDS, 235 and 303 pivots -- both odd, so a
    team's solve ends in its second buffer"""
    return gen.mixed_stack(100, 100, (2, 3))


def s16_stack():
    """two LPs of 129 x 260: device-placed, scanned with S = 16; 391 and 465 pivots"""
    return gen.mixed_stack(129, 131, (1, 2))


def phased_mix():
    """four LPs that need phase 1 and two whose dependent row phase 1 drops"""
    return list(e2e_phase1()[:4]) + [dropped_row_lp(), dropped_row_lp()]
