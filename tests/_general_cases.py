"""Shared inputs and helpers of the general-form tests
(test_general_cases_cpu.py, test_batch_general_cpu.py,
test_gpu_batch_general.py): LPs with bounds, free variables and a direction,
built from _problem_cases, and the oracle's answer in the caller's terms
through the host statements of lpsol_amd.problem (general_standard_form,
general_recover, general_duals).  A plain module: no fixtures, no GPU."""
import numpy as np

import _problem_cases as pc
from lpsol_amd import generators as gen
from lpsol_amd import problem as pr
from lpsol_amd._lib import VAR_BOXED, VAR_FREE, VAR_LOWER, VAR_PLAIN, VAR_UPPER

PLAIN, LOWER, BOXED, UPPER, FREE = VAR_PLAIN, VAR_LOWER, VAR_BOXED, VAR_UPPER, VAR_FREE
INF = float("inf")
SEEDS = range(1, 41)
NS = 5


def bounds_of(kind, x0):
    """lb = x0 - 0.5 and ub = x0 + 0.75 where the kind has the bound; 0 and
    +inf for PLAIN; x0 stays feasible"""
    kind = np.asarray(kind)
    lb = np.where(np.isin(kind, (LOWER, BOXED)), x0 - 0.5, np.where(kind == PLAIN, 0.0, -INF))
    ub = np.where(np.isin(kind, (BOXED, UPPER)), x0 + 0.75, INF)
    return lb, ub


def general_lp(seed, ns=NS, kinds=None):
    """mixed_sense_block(seed, ns) with kinds (seed + j) % 5 and the bounds of
    bounds_of around its feasible point -> (P, senses, kind, lb, ub)"""
    P, sense = pc.mixed_sense_block(seed, ns)
    x0 = gen.uint_range(seed, 7, np.arange(ns, dtype=np.uint64), 0, 4) / 4.0
    kind = np.array([(seed + j) % 5 for j in range(ns)] if kinds is None else kinds, dtype=np.int8)
    lb, ub = bounds_of(kind, x0)
    return P, sense, kind, lb, ub


def slack_of(T_final_x, sense, kind):
    """the m original rows' slack values from the standard form's x'"""
    ns, nf = len(kind), int(np.count_nonzero(np.asarray(kind) == FREE))
    rows, cols, _ = pr._slack_columns(np.asarray(sense), ns + nf)
    out = np.zeros(len(sense))
    out[rows] = np.asarray(T_final_x)[cols]
    return out


def xstd_of(rep, n):
    """the standard form's x' of an oracle report: Simplex.getBFS"""
    x = np.zeros(n)
    T = rep["T"]
    for r, j in enumerate(rep["bfs"][:rep["rows"]]):
        if 0 <= j < n:
            x[j] = T[1 + r, 0]
    return x


def oracle_solve(P, sense, kind, lb, ub, maximise):
    """the LP through general_standard_form and oracle.phase1.solve_lp ->
    dict(status, rep, T0 (the standard form), x, z, y, r) in the caller's terms"""
    from oracle.phase1 import solve_lp
    T0 = pr.general_standard_form(P, lb, ub, sense, kind, maximise)
    rep = solve_lp(T0.copy(), report=True)
    T = rep["T"]
    xs = xstd_of(rep, T0.shape[1] - 1)
    x, z = pr.general_recover(xs, T[0, 0], lb, ub, kind, maximise)
    y, r = pr.general_duals(T, sense, kind, maximise)
    return dict(status=rep["status"], rep=rep, T0=T0, xstd=xs, x=x, z=float(z), y=y, r=r)


# ---------------------------------------------------------------------------
# hand-built all-integer LPs whose answers are known exactly: every pivot is on
# an entry +-1, so the float64 values are the exact ones
# ---------------------------------------------------------------------------

def hand_lps():
    """-> [dict(c, A, b, sense, lb, ub, maximize, c0, x, z, y, r, status)]"""
    out = []
    # max x0 + 2 x1:  x0 + x1 <= 4,  0 <= x0 <= 3,  1 <= x1 <= 2  ->  x1 ends at its upper bound
    out.append(dict(c=[1.0, 2.0], A=[[1.0, 1.0]], b=[4.0], sense=[pc.LE], lb=[0.0, 1.0], ub=[3.0, 2.0],
                    maximize=True, c0=0.0, x=[2.0, 2.0], z=6.0, y=[1.0], r=[0.0, 1.0], status="optimal"))
    # min x0 + x1:  x0 >= -3 as a row, x0 free, x1 >= -2  ->  a free variable negative, a negative lb
    out.append(dict(c=[1.0, 1.0], A=[[1.0, 0.0]], b=[-3.0], sense=[pc.GE], lb=[-INF, -2.0], ub=[INF, INF],
                    maximize=False, c0=0.0, x=[-3.0, -2.0], z=-5.0, y=[1.0], r=[0.0, 1.0], status="optimal"))
    # min -2 x0 + x1 + 10:  x0 - x1 <= 1,  x0 <= 5 (UPPER),  x1 >= 0  ->  x0 ends at its only bound
    out.append(dict(c=[-2.0, 1.0], A=[[1.0, -1.0]], b=[1.0], sense=[pc.LE], lb=[-INF, 0.0], ub=[5.0, INF],
                    maximize=False, c0=10.0, x=[5.0, 4.0], z=4.0, y=[-1.0], r=[-1.0, 0.0], status="optimal"))
    # lb > ub: min x0,  x0 + x1 <= 4,  2 <= x0 <= 1
    out.append(dict(c=[1.0, 0.0], A=[[1.0, 1.0]], b=[4.0], sense=[pc.LE], lb=[2.0, 0.0], ub=[1.0, INF],
                    maximize=False, c0=0.0, x=None, z=None, y=None, r=None, status="infeasible"))
    return out


def hand_block(h):
    """-> (P, sense, kind, lb, ub) of a hand LP"""
    P = pr.pack_problems(np.array([h["c"]]), np.array([h["A"]]), np.array([h["b"]]), np.array([-h["c0"]]))[0]
    lb, ub = np.array(h["lb"]), np.array(h["ub"])
    return P, np.array(h["sense"], dtype=np.int8), pr.general_kinds(lb, ub), lb, ub


# ---------------------------------------------------------------------------
# ragged lists: the lane-lookup shapes of _problem_cases with kinds cycling per
# LP and directions alternating
# ---------------------------------------------------------------------------

def ragged_general(shapes=pc.RAGGED_SHAPES, seed0=300):
    """-> per LP (P, sense, kind, lb, ub, maximise): the blocks and senses of
    pc.ragged_blocks, kinds (i + j) % 5, dyadic bounds, max on odd LPs"""
    blocks, senses = pc.ragged_blocks(shapes, seed0)
    out = []
    for i, (P, s) in enumerate(zip(blocks, senses)):
        ns = P.shape[1] - 1
        kind = np.array([(i + j) % 5 for j in range(ns)], dtype=np.int8)
        x0 = gen.uint_range(seed0 + i, 7, np.arange(ns, dtype=np.uint64), 0, 8) / 4.0 - 1.0
        lb, ub = bounds_of(kind, x0)
        out.append((P, s, kind, lb, ub, i % 2 == 1))
    return out


def pivot_entries(T0, rep):
    """the entries an oracle report's pivots were made on: phase 1 replayed as
    oracle.phase1.find_bfs lays it out (rows with b < 0 negated, one artificial
    column per row without a basic column), then phase 2 on the restored
    tableau -> (entries, the replayed final tableau)"""
    from oracle.phase1 import basic_columns

    def pivot(W, r, c):
        p = W[1 + r, 1 + c]
        W[1 + r] = W[1 + r] / p
        for i in range(W.shape[0]):
            if i != 1 + r:
                W[i] = W[i] - W[i, 1 + c] * W[1 + r]
        return p

    T = np.array(T0, dtype=np.float64)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    T[1:][T[1:, 0] < 0.0] *= -1.0
    ok, bfs = basic_columns(T)
    entries = []
    if not ok:
        missing = [i for i, j in enumerate(bfs) if j == -1]
        W = np.zeros((m + 1, n + 1 + len(missing)))
        W[:, :n + 1] = T
        W[0] = 0.0
        for ind, i in enumerate(missing):
            W[0, 1 + n + ind] = 1.0
            W[1 + i, 1 + n + ind] = 1.0
            W[0] = W[0] - W[1 + i]
            bfs[i] = n + ind
        for r, c in rep["init_seq"]:
            entries.append(pivot(W, r, c))
            bfs[r] = c
        keep = [0] + [1 + i for i in range(m) if bfs[i] < n]
        c_row = T[0].copy()
        T = np.ascontiguousarray(W[keep, :n + 1])
        T[0] = c_row
        for i, j in enumerate(b for b in bfs if b < n):
            T[0] = T[0] - T[0, 1 + j] * T[1 + i]
    for r, c in rep["seq"]:
        entries.append(pivot(T, r, c))
    return entries, T
