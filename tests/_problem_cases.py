"""Shared inputs and helpers of the problem-form tests
(test_problem_cases_cpu.py, test_batch_problem_cpu.py,
test_gpu_batch_problem.py): LPs as problem blocks with one sense per row, all
built from lpsol_amd.generators, and the host statements the device is
compared with (lpsol_amd.problem.assemble_tableaux, problem_duals).
A plain module: no fixtures, no GPU."""
import numpy as np

from lpsol_amd import generators as gen
from lpsol_amd._lib import SENSE_EQ, SENSE_GE, SENSE_LE

LE, GE, EQ = SENSE_LE, SENSE_GE, SENSE_EQ
QNAN_BITS = 0x7FF8000000000000
KINDS = ("mixed", "neg", "eq", "ge")
CPU_SHAPES = [(3, 5), (8, 10), (24, 24)]        # (m, ns) of the generator call
CPU_SEEDS = range(1, 9)
MIXED_SENSE = [GE, EQ, LE, LE, GE]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------
# the generators' LPs in problem form
# ---------------------------------------------------------------------------

def lp(kind, m, ns, seed):
    """-> (tableau, senses int8, ns): the generator's tableau and the senses
    and structural-variable count that give it back"""
    if kind == "mixed":
        return gen.tableau("mixed", m, ns, seed), np.full(m, LE, dtype=np.int8), ns
    T = gen.phase1_lp(kind, m, ns, seed)
    if kind == "neg":
        return T, np.full(m + 1, LE, dtype=np.int8), ns
    if kind == "ge":
        return T, np.array([GE] * m + [LE], dtype=np.int8), ns
    if kind == "eq":
        return T, np.full(m + 1, EQ, dtype=np.int8), ns
    raise ValueError(kind)


def block(T, ns):
    """the problem block of a tableau: its first ns + 1 columns"""
    return np.ascontiguousarray(T[..., :ns + 1])


def parts(T, ns):
    """-> (c, A, b) of a tableau or a stack of them"""
    return T[..., 0, 1:ns + 1], T[..., 1:, 1:ns + 1], T[..., 1:, 0]


def stack(kind, m, ns, seeds):
    """-> (tableaux [B, ...], senses, ns) of lp() over the seeds"""
    got = [lp(kind, m, ns, s) for s in seeds]
    return np.stack([g[0] for g in got]), got[0][1], ns


def mixed_sense_block(seed, ns=4):
    """a 5-row LP under MIXED_SENSE with x0 >= 0 a feasible point: row 3 is
    sum x <= sum x0 + 1 (bounds it); values dyadic -> (block [6, ns+1], senses)"""
    m, Q = len(MIXED_SENSE), 64
    A = gen.uint_range(seed, gen.S_A, np.arange(m * ns, dtype=np.uint64), -Q, Q).reshape(m, ns) / Q
    x0 = gen.uint_range(seed, 7, np.arange(ns, dtype=np.uint64), 0, 4) / 4.0
    d = gen.uint_range(seed, gen.S_B, np.arange(m, dtype=np.uint64), 0, 2) / 4.0
    A[3] = 1.0
    d[3] = 1.0
    b = A @ x0 + np.array([-1.0, 0.0, 1.0, 1.0, -1.0]) * d
    P = np.zeros((m + 1, ns + 1))
    P[0, 1:] = -gen.uint_range(seed, gen.S_C, np.arange(ns, dtype=np.uint64), 1, Q) / Q
    P[1:, 0] = b
    P[1:, 1:] = A
    return P, np.array(MIXED_SENSE, dtype=np.int8)


def dependent_block(seed, ns=4):
    """two <= rows (the first bounds the LP) and one == row given twice: phase
    1 drops one of the two, so rows < m -> (block [5, ns+1], senses)"""
    P5, _ = mixed_sense_block(seed, ns)
    P = np.zeros((5, ns + 1))
    P[0] = P5[0]
    P[1] = P5[4]            # sum x <= sum x0 + 1
    P[2] = P5[3]            # a <= row with slack in b
    P[3] = P5[2]            # the == row ...
    P[4] = P5[2]            # ... again
    return P, np.array([LE, LE, EQ, EQ], dtype=np.int8)


def infeasible_block():
    """x0 + x1 <= 1 and x0 + x1 >= 2"""
    P = np.array([[0.0, -1.0, -1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 1.0]])
    return P, np.array([LE, GE], dtype=np.int8)


def special_block():
    """a 2 x 3 block of cells a copy must keep: a NaN with a payload, -0.0,
    both infinities, a denormal -> (block [3, 4], senses)"""
    P = np.array([[-0.0, 1.0, -2.0, 3.0], [4.0, 5.0, 6.0, 7.0], [8.0, 9.0, 10.0, 11.0]])
    u = P.view(np.uint64)
    u[0, 1] = 0x7FF8000000ABCDEF        # quiet NaN, payload
    u[1, 0] = 0xFFF0000000000001        # signalling NaN, sign set
    P[1, 2] = np.inf
    P[2, 1] = -np.inf
    u[2, 3] = 0x0000000000000003        # denormal
    P[2, 0] = -0.0
    return P, np.array([GE, LE], dtype=np.int8)


# ---------------------------------------------------------------------------
# hand-built all-integer LPs whose duals are known exactly: every pivot is on
# an entry +-1, so the float64 values are the exact ones
# ---------------------------------------------------------------------------

def hand_lps():
    """-> [(block, senses, x, z, y)]"""
    nan = float("nan")
    out = []
    # min -x0 - 2 x1:  x0 + x1 <= 4,  x0 >= 1,  x1 == 2   ->  x = (2, 2), z = -6
    P = np.array([[0.0, -1.0, -2.0], [4.0, 1.0, 1.0], [1.0, 1.0, 0.0], [2.0, 0.0, 1.0]])
    out.append((P, np.array([LE, GE, EQ], dtype=np.int8), [2.0, 2.0], -6.0, [-1.0, 0.0, nan]))
    # min 2 x0 + 3 x1:  x0 + x1 >= 4,  x0 <= 3   ->  x = (3, 1), z = 9, y = (3, -1)
    P = np.array([[0.0, 2.0, 3.0], [4.0, 1.0, 1.0], [3.0, 1.0, 0.0]])
    out.append((P, np.array([GE, LE], dtype=np.int8), [3.0, 1.0], 9.0, [3.0, -1.0]))
    return out


# ---------------------------------------------------------------------------
# the ragged list of the lane-lookup tests, as (m, ns), and its windows
# ---------------------------------------------------------------------------

RAGGED_SHAPES = [(m, 13) for m in range(1, 13)] + [(1, 1), (1, 1), (70, 200), (1, 1), (3, 1)]
RAGGED_WINDOWS = [(0, len(RAGGED_SHAPES)), (0, 1), (len(RAGGED_SHAPES) - 1, 1), (2, 3), (11, 4), (13, 4)]


def cycled_senses(i, m):
    """LP i's senses: all <=, all >=, all ==, mixed, by i mod 4"""
    if i % 4 == 3:
        return np.array([(LE, GE, EQ)[r % 3] for r in range(m)], dtype=np.int8)
    return np.full(m, (LE, GE, EQ)[i % 4], dtype=np.int8)


def ragged_blocks(shapes=RAGGED_SHAPES, seed0=300):
    """-> (blocks, senses): LP i the first ns + 1 columns of mixed(m, ns, seed0 + i)"""
    blocks = [block(gen.tableau("mixed", m, ns, seed0 + i), ns) for i, (m, ns) in enumerate(shapes)]
    return blocks, [cycled_senses(i, m) for i, (m, _) in enumerate(shapes)]


E2E_SHAPES = [(1 + (3 * i) % 11, 1 + (5 * i) % 7) for i in range(12)]      # (m, ns)
