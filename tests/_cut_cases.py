"""Shared oracle and inputs of the warm-cut tests (test_cut_cases_cpu.py,
test_batch_cut_cpu.py, test_gpu_batch_cut.py, test_gpu_batch_cut_edges.py).

The oracle of lp_cut_extend is extend() below: the header's loop, plain
float64 `acc - c * t`, one scalar at a time.  What follows it is
_dual_cases.walk.  Nothing here comes from the device.  A plain module: no
fixtures, no GPU."""
import math
import os
import re

import numpy as np

import _dual_cases as dc
import _reopt_cases as rc
from lpsol_amd import _lib, solution_x
from lpsol_amd import generators as gen
from lpsol_amd import problem as pr
from oracle.f64 import F64Tableau

same_bits = dc.same_bits
LE, GE = _lib.SENSE_LE, _lib.SENSE_GE
S_CUT = 31                          # cut k draws from stream 31 + k (the other modules use 1..3, 7, 11..13, 21, 23)
SMALL, MID, LARGE = (8, 10), (24, 24), (40, 40)         # (m, ns) of the generator call
SEEDS = {SMALL: range(1, 65), MID: range(1, 33), LARGE: range(1, 17)}
WORKLOADS = ("le", "lege")
CAP_FACTOR = 10                     # the cap of a warm walk: 10 * (m' + n')


# ------------------------------------------------------------------ the loop
def extend(T, basis, rows, sense):
    """-> (D, basis'): the stored (m+1) x (n+1) tableau T with q more rows:
    acc = row_k[j]; for r: c = basis[r]; if 0 <= c < n: acc = acc - row_k[1+c] * T[1+r][j];
    D[1+m+k][j] = acc, its sign bit flipped iff sense_k is GE"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, n + 1)
    q = rows.shape[0]
    sense = list(sense)
    assert len(sense) == q and len(basis) == m and all(s in (LE, GE) for s in sense)
    D = np.zeros((m + q + 1, n + q + 1))
    D.view(np.uint64)[:m + 1, :n + 1] = T.view(np.uint64)
    sign = np.uint64(1 << 63)
    with np.errstate(all="ignore"):
        for k in range(q):
            for j in range(n + 1):
                acc = rows[k, j]
                for r in range(m):
                    c = int(basis[r])
                    if c < 0 or c >= n:
                        continue
                    prod = rows[k, 1 + c] * T[1 + r, j]
                    acc = acc - prod
                D[1 + m + k, j] = acc
            if sense[k] == GE:
                D.view(np.uint64)[1 + m + k, :n + 1] ^= sign
            D[1 + m + k, 1 + n + k] = 1.0
    return D, np.concatenate([np.asarray(basis, dtype=np.int32), np.arange(n, n + q, dtype=np.int32)])


# ------------------------------------------------------------------ the cuts
def coefficients(seed, k, ns):
    """a_j = U{0..8} / 8 over the ns structural columns, stream 31 + k"""
    return gen.uint_range(2000 + seed, S_CUT + k, np.arange(ns, dtype=np.uint64), 0, 8) / 8.0


def dot(a, x):
    """a . x summed in index order"""
    s = 0.0
    for aj, xj in zip(a, x):
        s += float(aj) * float(xj)
    return s


def cuts(workload, seed, ns, x, q=2):
    """-> (a [q, ns], beta [q], sense [q]) at the optimum x: `le` cuts are a.x <= floor(48 a.x*) / 64; under
    `lege` every odd cut is a.x >= ceil(64 a.x*) / 64 + 0.25"""
    a = np.stack([coefficients(seed, k, ns) for k in range(q)]) if q else np.zeros((0, ns))
    beta, sense = np.zeros(q), np.full(q, LE, dtype=np.int8)
    for k in range(q):
        ax = dot(a[k], x)
        if workload == "lege" and k % 2 == 1:
            beta[k], sense[k] = math.ceil(64 * ax) / 64 + 0.25, GE
        else:
            beta[k] = math.floor(48 * ax) / 64
    return a, beta, sense


def stated(a, beta, n):
    """the cuts as lp_cut_extend takes them: beta, a, +0.0 under the slack columns"""
    a = np.asarray(a, dtype=np.float64)
    rows = np.zeros((a.shape[0], n + 1))
    rows[:, 0] = beta
    rows[:, 1:a.shape[1] + 1] = a
    return rows


_CASES = {}


def case(m, ns, seed, workload, q=2):
    """the `mixed` LP solved by lpf_solve, then cut -> dict: T0 the LP, opt / basis the oracle's optimal
    tableau and basis, x its x, a / beta / sense the cuts, rows as stated, D / basis2 what extend() makes,
    cold0 the LP assembled with the extra rows, warm the walk of D; computed once"""
    key = (m, ns, seed, workload, q)
    if key not in _CASES:
        T0 = gen.tableau("mixed", m, ns, seed)
        o = F64Tableau(T0)
        st, log, _ = o.solve()
        assert st == _lib.OPTIMAL
        basis = rc.basis_of(np.arange(ns, ns + m), log)
        x = solution_x(o.T, basis)[:ns]
        a, beta, sense = cuts(workload, seed, ns, x, q)
        rows = stated(a, beta, ns + m)
        D, basis2 = extend(o.T, basis, rows, sense)
        P = np.zeros((m + q + 1, ns + 1))
        P[:m + 1] = T0[:, :ns + 1]
        P[m + 1:, 0] = beta
        P[m + 1:, 1:] = a
        joined = np.concatenate([np.full(m, LE, dtype=np.int8), sense])
        cold0 = pr.assemble_tableaux([P], [joined])[0]
        for v in (D, cold0, o.T):
            v.setflags(write=False)
        cap = CAP_FACTOR * (D.shape[0] - 1 + D.shape[1] - 1)
        _CASES[key] = dict(T0=T0, opt=o.T, basis=basis, x=x, a=a, beta=beta, sense=sense, rows=rows, D=D,
                           basis2=basis2, cold0=cold0, joined=joined, cap=cap, warm=dc.walk(D, cap),
                           cold_pivots0=len(log))
    return _CASES[key]


def warm_answer(c):
    """(status, npiv, x of all columns, objective) of a case's walk"""
    w = c["warm"]
    basis = rc.basis_of(c["basis2"], w["log"])
    return w["status"], w["npiv"], solution_x(w["T"], basis), -w["T"][0, 0]


def cold(c, workload):
    """the cold verdict and optimum of a case: F64Tableau.solve for `le` (-> pivots too), the two-phase oracle
    for `lege` (pivots None)"""
    if workload == "le":
        o = F64Tableau(c["cold0"])
        st, log, _ = o.solve()
        return int(st), -o.T[0, 0], len(log)
    from oracle.phase1 import solve_lp
    rep = solve_lp(np.array(c["cold0"]), report=True)
    return int(rep["status"]), float(rep["objective"]), None


# ------------------------------------------------------------------ ragged batches: q cycling 0, 1, 3
Q_CYCLE = (0, 1, 3)
RAGGED_SHAPES = [SMALL, MID, (1, 1), SMALL, (1, 1), MID, SMALL, (1, 1), MID]      # (m, ns)


def ragged_cases(workload="lege"):
    """-> [case]: LP i of RAGGED_SHAPES with q = Q_CYCLE[i % 3] cuts, seed 1 + i"""
    return [case(m, ns, 1 + i, workload, Q_CYCLE[i % 3]) for i, (m, ns) in enumerate(RAGGED_SHAPES)]


# ------------------------------------------------------------------ the flat kernels across workgroups
# (test_gpu_batch_cut_edges.py; the shapes are vetted by test_cut_cases_cpu.py)
FLAT = dc.FLAT      # PLAN_FLAT_THREADS: lanes per workgroup of k_cut_copy, k_cut_rows, k_cut_basis
GROUP = int(re.search(r"define LPK_CUT_GROUP (\d+)",
                      open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                                        "linear-program-solver_amd", "csrc", "knobs.h")).read()).group(1))


def copy_lanes(m, ns, q):
    """destination elements: k_cut_copy's lanes"""
    return (m + q + 1) * (ns + m + q + 1)


def rows_lanes(m, ns, q):
    """k_cut_rows: one lane per (group of up to GROUP new rows, column 0..n)"""
    return (q + GROUP - 1) // GROUP * (ns + m + 1)


def basis_lanes(m, ns, q):
    """k_cut_basis: one lane per destination basis entry"""
    return m + q


LANE_MAPS = dict(copy=copy_lanes, rows=rows_lanes, basis=basis_lanes)


def lane_starts(batch, which, first, count):
    """the lane of LANE_MAPS[which] each LP of the window begins at, and one past the last"""
    return np.concatenate([[0], np.cumsum([LANE_MAPS[which](*s) for s in batch[first:first + count]])]).tolist()


# (m, ns, q) per LP, seed 1 + i, workload lege
_SMALL = ((1, 1, 1), (1, 2, 3), (1, 1, 1), (1, 1, 5), (2, 1, 1))
BLOCK = ([(8, 10, 2), (1, 1, 0), (1, 1, 0)] + [_SMALL[j % 5] for j in range(60)]
         + [(1, 1, 0)] * 3 + [_SMALL[j % 5] for j in range(24)] + [(260, 3, 1), (40, 40, 9), (8, 10, 9)]
         + [_SMALL[j % 5] for j in range(70)] + [(1, 1, 0)] * 2)
BLOCK_BIG = 90
# k_cut_copy runs over elements: a batch of its own, shapes drawn from _COPY, LP 44 the 18 x 28 one (504 elements)
_COPY = ((1, 1, 0), (1, 1, 1), (1, 2, 1), (2, 1, 1), (1, 2, 3), (1, 2, 0), (2, 1, 0), (1, 1, 3))
COPY_BIG = 44
COPY_BLOCK = [_COPY[int(k)] for k in gen.uint_range(1, 41, np.arange(54, dtype=np.uint64), 0, len(_COPY) - 1)]
COPY_BLOCK[COPY_BIG] = (8, 10, 9)
# the uniform source: 8 x 10 LPs whose q cycles, with runs of q = 0
_Q_UNIFORM = (0, 0, 1, 3, 5, 9, 2, 4, 0, 0, 0, 8, 1, 6)
UNIFORM_BLOCK = [(8, 10, _Q_UNIFORM[i % len(_Q_UNIFORM)]) for i in range(68)] + [(8, 10, 0)] * 2


def block_cases(batch=None, workload="lege"):
    """-> [case] of a batch of (m, ns, q): LP i has seed 1 + i"""
    return [case(m, ns, 1 + i, workload, q) for i, (m, ns, q) in enumerate(BLOCK if batch is None else batch)]


def zero_runs(batch, first, count):
    """the runs of two or more q = 0 LPs of a window -> [(first LP, count)], window-relative"""
    runs, at = [], None
    for k in range(count + 1):
        zero = k < count and batch[first + k][2] == 0
        if zero and at is None:
            at = k
        if not zero and at is not None:
            if k - at >= 2:
                runs.append((at, k - at))
            at = None
    return runs


# ------------------------------------------------------------------ a constructed tableau with odd cells
def odd_case():
    """a 3 x 4 stored tableau (m = 3, n = 4) with an inf, a NaN and a -0.0, a basis holding -1 and an entry
    out of range, and three cuts: a <= one, a >= one whose priced cells are +0.0 on a zero column (stored
    -0.0), and a >= one through the NaN -> (T, basis, rows, sense)"""
    T = np.array([[0.0, 0.5, 0.0, 0.0, 1.0],
                  [2.0, 1.0, 0.0, np.inf, 0.25],
                  [1.0, -0.0, 0.0, np.nan, 3.0],
                  [4.0, 0.5, 0.0, 2.0, 1.0]])
    basis = np.array([0, -1, 7], dtype=np.int32)
    rows = np.array([[1.0, 1.0, 0.0, 2.0, 0.0],
                     [0.0, 0.0, 0.0, 0.0, 0.0],
                     [3.0, 0.5, 0.0, 1.0, 1.0]])
    return T, basis, rows, np.array([LE, GE, GE], dtype=np.int8)


# ------------------------------------------------------------------ windows of the batches above
# (first, count).  BLOCK: the whole batch, windows that begin later and still span three workgroups, one that ends
# with the middle run of q = 0 LPs, one that begins with it, that run alone (every LP has q = 0), the large LP
# alone, an LP that lies wholly in the second workgroup of both maps, the last LP (q = 0)
BLOCK_ZEROS = (63, 3)
BLOCK_WINDOWS = [(0, 165), (1, 164), (2, 163), (4, 161), (25, 140), (29, 136), (38, 127), (10, 56), (63, 40),
                 BLOCK_ZEROS, (BLOCK_BIG, 1), (80, 1), (164, 1)]
BLOCK_EDGES = dict(rows={0: (255,), 1: (256,), 4: (257,), 25: (513,)},
                   basis={0: (255,), 2: (256,), 1: (257,), 29: (512,), 38: (511,)})
BLOCK_INSIDE = 80
BLOCK_WALKED = (1, 164)             # begins and ends with a run of q = 0 LPs, the third in its middle
COPY_WINDOWS = [(0, 54), (8, 46), (12, 42), (15, 39), (19, 35), (COPY_BIG, 1), (20, 1)]
COPY_EDGES = {8: (255,), 12: (256,), 15: (257,), 19: (512,)}
COPY_INSIDE = 20
UNIFORM_WINDOWS = [(0, 70), (3, 67), (8, 3), (14, 30), (68, 2)]
UNIFORM_ZEROS = (8, 3)


# the batch of the windows without a row: runs of two q = 0 LPs first, in the middle and last from LP 1 on
ZERO_BATCH = [(8, 10, 0), (1, 1, 0), (1, 1, 0), (8, 10, 2), (1, 1, 0), (1, 1, 0), (24, 24, 3), (3, 5, 0), (1, 1, 0)]


def window_cost(batch, first, count):
    """what lp_cut_extend stages for a window: (table entries, senses, row doubles)"""
    w = batch[first:first + count]
    return count + 1, sum(q for _, _, q in w), sum(q * (ns + m + 1) for m, ns, q in w)


# ------------------------------------------------------------------ shapes at the kernels' thresholds
ONE_WAVE_ELEMS = dc.ONE_WAVE_ELEMS
THRESHOLD = (30, 30)                # 31 x 61 = 1891 elements; with two more rows 33 x 63 = 2079
LDS_EDGE = (99, 99)                 # batch_lds_bytes(99, 198) fits a CU's LDS; batch_lds_bytes(101, 200) does not
GROUP_QS = (2 * GROUP + 1, 3 * GROUP)


def group_cases(shape, q):
    """the batch of the three-group tests: seeds 1..4 under le, 5..8 under lege"""
    return [case(*shape, s, "le" if s <= 4 else "lege", q) for s in range(1, 9)]


# ------------------------------------------------------------------ stated rows near overflow and underflow
EXTREME_ROWS = ("1e308", "5e-324", "mixed")


def extreme_rows(rows, how):
    """the stated rows scaled by 1e308, by 5e-324, or the even columns by the one and the odd by the other"""
    rows = np.array(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        if how == "1e308":
            return rows * 1e308
        if how == "5e-324":
            return rows * 5e-324
        rows[:, ::2] *= 1e308
        rows[:, 1::2] *= 5e-324
    return rows
