"""Shared oracle, inputs and device helpers of the dual-rule and warm re-solve
tests (test_dual_cases_cpu.py, test_gpu_batch_dual.py, test_gpu_batch_rhs.py).

The oracle of lp_batch_run(b, LP_RULE_DUAL, k, ...) is the host walk below: the
selection exactly as include/lpgpu.h states it, in numpy float64 and in index
order, then oracle.f64.F64Tableau.pivot (oracle/lp_f64.c: lpf_pivot).  The
oracle of lp_resolve_set_rhs is set_rhs() below: the header's loop, plain
float64 `acc + t * b`.  Nothing here comes from the device.  A plain module: no
fixtures; nothing touches the GPU until a device helper is called."""
import numpy as np

import _maxinc_cases as mc
from lpsol_amd import _lib
from lpsol_amd import generators as gen
from oracle.f64 import DEFAULT_TOL, F64Tableau

DUAL = 3            # LP_RULE_DUAL
CAP = 512           # no input of these tests takes more than 68 dual pivots (test_dual_cases_cpu.py)
LOG_CAP = 128
INF = float("inf")

same_bits, start_basis, basis_after, shape_of = mc.same_bits, mc.start_basis, mc.basis_after, mc.shape_of


# ------------------------------------------------------------------ the walk
def dual_infeasible(T, t):
    """the start of a call: some cost below -tol.cost"""
    return bool((T[0, 1:] < -t["cost"]).any())


def select(T, t):
    """one selection in tableau indices -> (R, C), or the status the LP ends with"""
    m, n = T.shape[0] - 1, T.shape[1] - 1
    rows = [i for i in range(1, m + 1) if T[i, 0] < -t["zero"]]
    if not rows:
        return _lib.OPTIMAL
    g = INF
    for i in rows:
        if T[i, 0] < g:
            g = T[i, 0]
    thr = g + t["cost_tie"] * abs(g)
    R = next((i for i in rows if T[i, 0] <= thr), None)
    if R is None:
        return _lib.BAD_PIVOT
    cols = [j for j in range(1, n + 1) if T[R, j] < -t["pivot"]]
    if not cols:
        return _lib.INFEASIBLE
    q = {}
    for j in cols:
        c = T[0, j]
        q[j] = np.float64(0.0 if abs(c) <= t["cost"] else c) / np.float64(-T[R, j])
    g = INF
    for j in cols:
        if q[j] < g:
            g = q[j]
    thr = g + t["ratio_tie"] * abs(g)
    C = next((j for j in cols if q[j] <= thr), None)
    if C is None:
        return _lib.BAD_PIVOT
    return R, C


_WALKS = {}


def walk(T, k=CAP, tol=None):
    """one lp_batch_run(LP_RULE_DUAL, k) of a copy of T -> dict(status, log, T, npiv); computed once per input"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    key = (T.shape, T.tobytes(), int(k), tuple(sorted((tol or {}).items())))
    if key not in _WALKS:
        t = dict(DEFAULT_TOL, **(tol or {}))
        o = F64Tableau(T, tol)
        log, status = [], None
        with np.errstate(all="ignore"):
            if dual_infeasible(o.T, t):
                status = _lib.BAD_ARG
            while status is None:
                if len(log) >= k:
                    status = _lib.PIVOTED
                    break
                got = select(o.T, t)
                if not isinstance(got, tuple):
                    status = got
                    break
                R, C = got
                o.pivot(R - 1, C - 1)           # (a zero pivot is counted, not applied: lpf_pivot returns first)
                log.append([R - 1, C - 1])
        o.T.setflags(write=False)
        _WALKS[key] = dict(status=status, log=log, T=o.T, npiv=len(log))
    return _WALKS[key]


# ------------------------------------------------------------------ set_rhs
def slack_table(sense, ns):
    """+(1 + j) / -(1 + j) per row, j = ns + t for the t-th row: no equalities here"""
    s = np.asarray(sense)
    assert not (s == _lib.SENSE_EQ).any()
    return [int((1 + ns + t) * (1 if s[t] == _lib.SENSE_LE else -1)) for t in range(len(s))]


def set_rhs(T, slack, rhs):
    """a copy of the stored tableau T with the new column 0:
    acc = (i == 0 ? rhs[0] : +0.0); for k: acc = acc + (s_k * T[i][1+j_k]) * rhs[1+k]
    (rows side by side: each is the same scalar float64 loop)"""
    T = np.array(T, dtype=np.float64)
    rhs = np.asarray(rhs, dtype=np.float64)
    acc = np.zeros(T.shape[0])
    acc[0] = rhs[0]
    with np.errstate(all="ignore"):
        for k, s in enumerate(slack):
            t = T[:, abs(s)] if s > 0 else -T[:, abs(s)]
            acc = acc + t * rhs[1 + k]
    T[:, 0] = acc
    return T


# ------------------------------------------------------------------ perturbations
S_SCALE, S_SHIFT, S_PICK = 11, 12, 13       # streams of their own (the generators use 1..3 and 7)


def scale(b, seed):
    """b_i * U{0..128}/64: stays >= 0"""
    i = np.arange(len(b), dtype=np.uint64)
    return b * (gen.uint_range(seed, S_SCALE, i, 0, 128) / 64.0)


def shift(b, seed):
    """b_i - U{0..64}/64 on the rows where a second draw U{0..3} is 0: some b go negative"""
    i = np.arange(len(b), dtype=np.uint64)
    pick = gen.uint_range(seed, S_PICK, i, 0, 3) == 0
    return np.where(pick, b - gen.uint_range(seed, S_SHIFT, i, 0, 64) / 64.0, b)


PERTURB = dict(scale=scale, shift=shift)
SMALL, LARGE = (8, 10), (40, 40)            # (m, ns) of the generator call: 9 x 19 and 41 x 81 tableaux
SMALL_SEEDS, LARGE_SEEDS = range(1, 65), range(1, 33)
LARGE_GPU_SEEDS = range(1, 17)

_WARM = {}


def warm(m, ns, seed, how):
    """the `mixed` LP solved by lpf_solve, then given new right-hand sides -> dict:
    T0 the LP with the new b in column 0 (what a cold solve gets), b the new b,
    opt the oracle's optimal tableau of the original LP, basis its basis,
    T the warm tableau set_rhs() makes of opt; computed once"""
    key = (m, ns, seed, how)
    if key not in _WARM:
        T0 = gen.tableau("mixed", m, ns, seed)
        o = F64Tableau(T0)
        st, log, _ = o.solve()
        assert st == _lib.OPTIMAL
        basis = np.arange(ns, ns + m, dtype=np.int32)
        for r, c in log:
            basis[r] = c
        b = PERTURB[how](T0[1:, 0], seed)
        slack = slack_table([_lib.SENSE_LE] * m, ns)
        T = set_rhs(o.T, slack, np.concatenate([[T0[0, 0]], b]))
        cold = T0.copy()
        cold[1:, 0] = b
        for a in (T, cold, o.T):
            a.setflags(write=False)
        _WARM[key] = dict(T0=cold, b=b, opt=o.T, basis=basis, T=T, cold_pivots=len(log))
    return _WARM[key]


def warm_stack(shape, seeds, how):
    return np.stack([warm(*shape, s, how)["T"] for s in seeds])


# ------------------------------------------------------------------ constructed tableaux
def lp(rows):
    return np.array(rows, dtype=np.float64)


# rows 1 and 2 tie for the most negative b: the first wins, under cost_tie = 0 as well
ROW_TIE = lp([[0, 1, 2, 0, 0], [-2, -1, -1, 1, 0], [-2, -1, -2, 0, 1]])
# row 1 is inside the band of row 2's minimum: the first wins, under cost_tie = 0 the exact minimum does
ROW_BAND = lp([[0, 1, 2, 0, 0], [-2 + 2.0 ** -42, -1, -1, 1, 0], [-2, -1, -2, 0, 1]])
# columns 1 and 2 tie in the ratio (1 / 1 and 2 / 2): the first wins
COL_TIE = lp([[0, 1, 2, 3, 0], [-2, -1, -2, -1, 1], [4, 1, 1, 1, 0]])


def col_band(eps):
    T = COL_TIE.copy()
    T[0, 1] = 1 + eps
    return T


# column 1's ratio is above column 2's by less / more than ratio_tie: inside the band it wins as the first
COL_BAND_IN, COL_BAND_OUT = col_band(2.0 ** -42), col_band(2.0 ** -33)
# both costs are within tol.cost of 0 and clamp to ratio 0, a tie the first wins; under cost = 0 the ratios
# are 2e-10 and 1e-10 and the second wins
COST_CLAMP = lp([[0, 2e-10, 1e-10, 0], [-1, -1, -1, 1], [3, 1, 2, 0]])
# column 1's entry is between -tol.pivot and 0: not eligible, though its ratio would be the minimum
A_SMALL = lp([[0, 0, 5, 0], [-1, -1e-10, -1, 1], [3, 1, 2, 0]])
# b is between -tol.zero and 0: optimal at once
B_SMALL = lp([[0, 1, 2, 0], [-1e-10, -1, -1, 1], [3, 1, 2, 0]])
# x1 + x2 <= 1 and -x1 - x2 <= -2: one pivot, then row 1 has b = -1 and no negative entry
INFEASIBLE = lp([[0, 1, 1, 0, 0], [1, 1, 1, 1, 0], [-2, -1, -1, 0, 1]])
# b < 0 and no negative entry at once
INFEASIBLE_NOW = lp([[0, 1, 1, 0], [-1, 1, 0, 2], [3, 1, 2, 0]])
# a negative cost at the start of the call: not dual feasible
NEG_COST = lp([[0, -1, 2, 0], [-1, -1, -1, 1], [3, 1, 2, 0]])
# a NaN in the leaving row: not eligible there, and the pivot spreads it down its column
NAN_CELL = lp([[0, 1, 2, 0, 0], [-2, np.nan, -1, 1, 0], [-1, 1, -2, 0, 1]])
# the only eligible column has a NaN cost: its ratio is NaN, never taken, and no column is in the band
NAN_RATIO = lp([[0, np.nan, 2, 0], [-1, -1, 1, 1], [3, 1, 2, 0]])
# b = -inf: the band of the minimum is NaN and holds no row
NEG_INF_B = lp([[0, 1, 2, 0], [-np.inf, -1, -1, 1], [3, 1, 2, 0]])

CASES = dict(row_tie=ROW_TIE, row_band=ROW_BAND, col_tie=COL_TIE, col_band_in=COL_BAND_IN, col_band_out=COL_BAND_OUT,
             cost_clamp=COST_CLAMP, a_small=A_SMALL, b_small=B_SMALL, infeasible=INFEASIBLE,
             infeasible_now=INFEASIBLE_NOW, neg_cost=NEG_COST, nan_cell=NAN_CELL, nan_ratio=NAN_RATIO,
             neg_inf_b=NEG_INF_B)
TOLS = (None, dict(cost_tie=0.0), dict(ratio_tie=0.0), dict(cost=0.0))
TOL_IDS = ["default", "cost_tie=0", "ratio_tie=0", "cost=0"]


def edge_lp(m, n):
    """the only negative b in the last row, the only eligible column the last one: a lane mapping that
    loses the tail of either scan ends 'optimal' or 'infeasible' with no pivot.  Dyadic, dual feasible;
    the pivot changes every row"""
    i = np.arange(m * n, dtype=np.uint64)
    T = np.zeros((m + 1, n + 1))
    T[1:, 1:] = (gen.uint_range(m * 1000 + n, gen.S_A, i, 1, 64) / 64.0).reshape(m, n)
    T[0, 1:] = gen.uint_range(m * 1000 + n, gen.S_C, np.arange(n, dtype=np.uint64), 1, 64) / 64.0
    T[1:, 0] = 2.0 + gen.uint_range(m * 1000 + n, gen.S_B, np.arange(m, dtype=np.uint64), 0, 64) / 64.0
    T[m, 0] = -1.0
    T[m, n] = -1.0
    return T


EDGE_ROWS = [(m, n) for m in (63, 64, 65) for n in (4, 4 + m)]      # ns = 4 alone, and with the m slack columns
EDGE_COLS = [(3, w - 1) for w in (63, 64, 65, 255, 256, 257)]       # n + 1 = w


# ------------------------------------------------------------------ device
def device_run(stack, k=CAP, **kw):
    """one lp_batch_run(LP_RULE_DUAL, k) of a uniform stack or a list of LPs -> one record per LP"""
    kw.setdefault("log_cap", LOG_CAP)
    return mc.device_run(stack, k, rule=DUAL, **kw)


def assert_record(rec, T0, k=CAP, tol=None, tag=None):
    """status, done, the whole log, the basis and the final tableau against the walk"""
    w = walk(T0, k, tol)
    assert rec["status"] == w["status"], (tag, rec["status"], w["status"])
    assert rec["npiv"] == w["npiv"], (tag, rec["npiv"], w["npiv"])
    assert rec["log"] == w["log"], tag
    assert rec["basis"] == basis_after(shape_of(T0)[0], w["log"]), tag
    assert same_bits(rec["T"], w["T"]), tag


def assert_records(recs, stack, k=CAP, tol=None):
    assert len(recs) == len(stack)
    for i, rec in enumerate(recs):
        assert_record(rec, stack[i], k, tol, tag=i)


# ------------------------------------------------------------------ covering LPs
def covering(m, ns, seed):
    """min c.x, A x >= b, x >= 0 with A >= 0, b > 0, c > 0, dyadic -> (c [ns], A [m, ns], b [m]).
    Written as -A x <= -b it is dual feasible at the slack basis and primal infeasible: the cold start
    of the dual simplex"""
    A = gen.uint_range(seed, gen.S_A, np.arange(m * ns, dtype=np.uint64), 0, 64).reshape(m, ns) / 64.0
    b = gen.uint_range(seed, gen.S_B, np.arange(m, dtype=np.uint64), 1, 64) / 64.0
    c = gen.uint_range(seed, gen.S_C, np.arange(ns, dtype=np.uint64), 1, 64) / 64.0
    return c, A, b


def covering_tableau(m, ns, seed):
    """the assembled tableau of the negated form: columns 0..ns the problem block, then the m slacks"""
    c, A, b = covering(m, ns, seed)
    T = np.zeros((m + 1, ns + m + 1))
    T[0, 1:ns + 1] = c
    T[1:, 0] = -b
    T[1:, 1:ns + 1] = -A
    T[1:, ns + 1:] = np.eye(m)
    return T
