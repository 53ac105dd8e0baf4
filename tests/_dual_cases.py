"""Shared oracle, inputs and device helpers of the dual-rule and warm re-solve
tests (test_dual_cases_cpu.py, test_gpu_batch_dual.py, test_gpu_batch_rhs.py and
the two *_edges.py files next to them).

The oracle of lp_batch_run(b, LP_RULE_DUAL, k, ...) is the host walk below: the
selection exactly as include/lpgpu.h states it, in numpy float64 and in index
order, then oracle.f64.F64Tableau.pivot (oracle/lp_f64.c: lpf_pivot).  The
oracle of lp_resolve_set_rhs is set_rhs() below: the header's loop, plain
float64 `acc + t * b`.  Nothing here comes from the device.  A plain module: no
fixtures; nothing touches the GPU until a device helper is called."""
import numpy as np

import _maxinc_cases as mc
import _problem_cases as pc
from lpsol_amd import _lib, solution_x
from lpsol_amd import generators as gen
from oracle.f64 import DEFAULT_TOL, F64Tableau

DUAL = 3            # LP_RULE_DUAL
CAP = 512           # no input of these tests takes more than 68 dual pivots (test_dual_cases_cpu.py); the
                    # tolerance batches, one of which goes round under cost = 2, run under FIELD_CAP
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

# the same LPs where a lane of the wider kernels takes a second or third trip through `i += NT`: above the
# one-wave bound of 2048 elements the LDS kernel has NT = 256 lanes, the device-placed one NT = 1024
ONE_WAVE_ELEMS = 2048
LATER_LDS = [(3, 599), (3, 600), (3, 767), (3, 768), (300, 8), (511, 6), (513, 6)]
LATER_DEV = [(3, 1100), (3, 2047), (3, 2049), (1030, 4), (2049, 3)]


def elems(T):
    return T.shape[0] * T.shape[1]


# ------------------------------------------------------------------ two candidates in one lane
# edge_lp with two more candidates lo < hi; hi = lo + NT puts both into one lane of a kernel NT lanes wide.
# Columns: both are made eligible in the leaving row (the last) at a cost below every other, 1/128 against
# >= 1/64, so the last column is out of every band.  Rows: both get b = -2 against the last row's -1, and
# an eligible entry in the last column, the only one of their rows.
def lane_cols(m, n, lo, hi, band=False):
    """tie: the ratios of lo and hi are equal and lo wins.  band: hi holds the exact minimum and lo is
    above it by 2^-42 of it, inside ratio_tie = 1e-12: lo wins, and hi under ratio_tie = 0"""
    T = edge_lp(m, n)
    T[m, lo] = T[m, hi] = -1.0
    T[0, lo] = T[0, hi] = 2.0 ** -7
    if band:
        T[0, lo] = 2.0 ** -7 * (1 + 2.0 ** -42)
    return T


def lane_rows(m, n, lo, hi, band=False):
    """the same for rows lo and hi of column 0, under cost_tie"""
    T = edge_lp(m, n)
    T[lo, 0] = T[hi, 0] = -2.0
    T[lo, n] = T[hi, n] = -1.0
    if band:
        T[lo, 0] = -2.0 + 2.0 ** -42
    return T


LANE_LO = 6
# name -> (NT, place, (m, n) of the column cases, (m, n) of the row cases).  nt256_one_wave is below the
# one-wave bound, so its pair 6 / 262 shares a lane of the 64-lane kernel four trips apart; nt256 has six
# rows (columns) so that 7 x 337 is above the bound and the four-wave kernel runs
LANE_GROUPS = dict(nt64=(64, "lds", (3, 144), (144, 4)),
                   nt256_one_wave=(256, "lds", (3, 336), (336, 4)),
                   nt256=(256, "lds", (6, 336), (336, 6)),
                   nt1024=(1024, "device", (3, 1104), (1104, 4)))
LANE_TOLS = (None, dict(ratio_tie=0.0), dict(cost_tie=0.0))
LANE_TOL_IDS = ["default", "ratio_tie=0", "cost_tie=0"]


def lane_cases(group):
    """-> dict name -> (tableau, first log entry at the default, under ratio_tie = 0, under cost_tie = 0).
    *_lanes: lo = NT + 6 is one lane's second trip and hi = NT + 11 another lane's: a tie lo wins"""
    NT, _, (mc_, nc), (mr, nr) = LANE_GROUPS[group]
    lo, hi = LANE_LO, LANE_LO + NT
    lo2, hi2 = NT + 6, NT + 11
    R, C = mc_ - 1, nr - 1
    return dict(
        col_tie=(lane_cols(mc_, nc, lo, hi), [R, lo - 1], [R, lo - 1], [R, lo - 1]),
        col_band=(lane_cols(mc_, nc, lo, hi, band=True), [R, lo - 1], [R, hi - 1], [R, lo - 1]),
        col_lanes=(lane_cols(mc_, nc, lo2, hi2), [R, lo2 - 1], [R, lo2 - 1], [R, lo2 - 1]),
        row_tie=(lane_rows(mr, nr, lo, hi), [lo - 1, C], [lo - 1, C], [lo - 1, C]),
        row_band=(lane_rows(mr, nr, lo, hi, band=True), [lo - 1, C], [lo - 1, C], [hi - 1, C]),
        row_lanes=(lane_rows(mr, nr, lo2, hi2), [lo2 - 1, C], [lo2 - 1, C], [lo2 - 1, C]))


# ------------------------------------------------------------------ each tolerance field, both directions
# zero: B_SMALL's b = -1e-10 takes part only under zero = 0; b = -0.5 takes part up to zero = 0.5
B_HALF = lp([[0, 1, 2, 0], [-0.5, -1, -1, 1], [3, 1, 2, 0]])
# pivot: A_SMALL's -1e-10 is eligible only under pivot = 0, where its ratio 0 wins.  PIVOT_STEPS: the ratios
# are 1 / 0.5 = 2 and 8 / 2 = 4, so column 1 wins; pivot = 1 leaves column 2 alone, pivot = 4 none
PIVOT_STEPS = lp([[0, 1, 8, 0], [-1, -0.5, -2, 1], [3, 1, 2, 0]])
# cost at the start of a call: -1e-10 is inside the default 1e-9 (and clamps to ratio 0), and below -cost for
# cost = 0 and cost = 1e-11; NEG_COST's -1 is dual feasible only from cost = 1 up
COST_SMALL = lp([[0, -1e-10, 2, 0], [-1, -1, -1, 1], [3, 1, 2, 0]])

TOL_CASES = dict(b_small=B_SMALL, b_half=B_HALF, a_small=A_SMALL, pivot_steps=PIVOT_STEPS, cost_small=COST_SMALL,
                 neg_cost=NEG_COST)
FIELD_TOLS = (None, dict(zero=0.0), dict(zero=1.0), dict(pivot=0.0), dict(pivot=1.0), dict(pivot=4.0),
              dict(cost=0.0), dict(cost=1e-11), dict(cost=2.0))
FIELD_TOL_IDS = ["default", "zero=0", "zero=1", "pivot=0", "pivot=1", "pivot=4", "cost=0", "cost=1e-11", "cost=2"]


FIELD_CAP = LOG_CAP         # the cap of these batches: the whole log of every LP is kept


def field_lps():
    """the ragged batch of the tolerance tests: TOL_CASES, CASES and warm LPs of both kernel widths"""
    lps = list(TOL_CASES.values()) + list(CASES.values())
    lps[4:4] = list(warm_stack(SMALL, range(1, 4), "shift"))
    return lps + list(warm_stack(LARGE, range(1, 3), "scale"))


def tol_key(tol):
    return tuple(sorted((tol or {}).items()))


# (status, log) of each TOL_CASES entry at the default and under the sets of its own field: each field has a
# case that changes when it goes to 0 and one that changes when it is raised above a value that took part
TOL_WANT = dict(
    b_small={(): (_lib.OPTIMAL, []), (("zero", 0.0),): (_lib.OPTIMAL, [[0, 0]]), (("zero", 1.0),): (_lib.OPTIMAL, [])},
    b_half={(): (_lib.OPTIMAL, [[0, 0]]), (("zero", 0.0),): (_lib.OPTIMAL, [[0, 0]]), (("zero", 1.0),): (_lib.OPTIMAL, [])},
    a_small={(): (_lib.OPTIMAL, [[0, 1]]), (("pivot", 0.0),): (_lib.OPTIMAL, [[0, 0], [1, 1]]),
             (("pivot", 1.0),): (_lib.INFEASIBLE, []), (("pivot", 4.0),): (_lib.INFEASIBLE, [])},
    pivot_steps={(): (_lib.OPTIMAL, [[0, 0]]), (("pivot", 0.0),): (_lib.OPTIMAL, [[0, 0]]),
                 (("pivot", 1.0),): (_lib.OPTIMAL, [[0, 1]]), (("pivot", 4.0),): (_lib.INFEASIBLE, [])},
    cost_small={(): (_lib.OPTIMAL, [[0, 0]]), (("cost", 0.0),): (_lib.BAD_ARG, []),
                (("cost", 1e-11),): (_lib.BAD_ARG, []), (("cost", 2.0),): (_lib.OPTIMAL, [[0, 0]])},
    neg_cost={(): (_lib.BAD_ARG, []), (("cost", 0.0),): (_lib.BAD_ARG, []), (("cost", 1e-11),): (_lib.BAD_ARG, []),
              (("cost", 2.0),): (_lib.OPTIMAL, [[0, 0]])})


def tol_want(name, tol):
    """the stated outcome, or None where the set moves another field than the case's"""
    return TOL_WANT[name].get(tol_key(tol))


# ------------------------------------------------------------------ k_rhs across workgroups
FLAT = 256          # PLAN_FLAT_THREADS: a lane of k_rhs is one (LP, row) pair of the window, rows 0..m_i


def _item(kind, m, ns, seed):
    T, sense, _ = pc.lp(kind, m, ns, seed)
    return (*pc.parts(T, ns), sense)


def _one_by_one(i):
    """a 1 x 1 LP, two lanes; every fifth is min x, x >= b"""
    if i % 5 == 4:
        return np.array([1.0]), np.array([[1.0]]), np.array([0.5 + i / 64.0]), np.array([pc.GE], dtype=np.int8)
    return _item("mixed", 1, 1, 500 + i)


BLOCK_BIG = 131     # the LP whose 261 lanes lie in two workgroups, whatever window holds it


def block_problems():
    """(c, A, b, sense) of 173 LPs, 613 lanes: 9 (>= rows), 130 x 2 up to lane 269, 261 (m = 260), 3 (a >=
    row), 40 x 2.  In the whole batch LPs begin at lanes 255 and 257; from LP 1 on one begins at 256; from
    LP 6 on the large LP ends at 511 and the next begins there; from LP 7 on the three-lane LP ends at 512"""
    items = [_item("ge", 7, 10, 41)] + [_one_by_one(i) for i in range(130)]
    items += [_item("mixed", 260, 3, 42), _item("ge", 1, 2, 43)] + [_one_by_one(130 + i) for i in range(40)]
    return items


def lane_starts(items, first, count):
    """the lane each LP of the window begins at, and one past the last: cumulative m_i + 1"""
    return np.concatenate([[0], np.cumsum([len(it[2]) + 1 for it in items[first:first + count]])]).tolist()


# (first, count): the whole batch, three windows that begin later and still span three workgroups, the large
# LP alone, an LP that lies wholly in the second workgroup of the whole batch (lanes 257, 258), the last LP
BLOCK_WINDOWS = [(0, 173), (1, 171), (6, 167), (7, 166), (BLOCK_BIG, 1), (125, 1), (172, 1)]
BLOCK_EDGES = {0: (255, 257), 1: (256,), 6: (511,), 7: (512,)}      # first -> lanes at which an LP of the window begins
UNIFORM_BLOCKS = dict(m=6, ns=8, B=80, windows=[(0, 80), (37, 43), (36, 2)])      # 7 lanes per LP: 256 = 36 * 7 + 4


# ------------------------------------------------------------------ batches that are not all optimal
def unbounded_parts():
    """(c, A, b) of six 3 x 5 `mixed` LPs, LP 2 replaced by one that is unbounded along x0"""
    T, _, ns = pc.stack("mixed", 3, 5, range(1, 7))
    c, A, b = (np.array(a) for a in pc.parts(T, ns))
    c[2] = [-1, 0, 0, 0, 0]
    A[2] = [[-1, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 1]]
    b[2] = 1.0
    return c, A, b


UNBOUNDED_AT = 2
INFEASIBLE_AT = 1


def infeasible_problems():
    """a ragged list whose LP 1 is pc.infeasible_block()"""
    P, s = pc.infeasible_block()
    return [_item("mixed", 8, 10, 40), (P[0, 1:], P[1:, 1:], P[1:, 0], s), _item("ge", 3, 5, 42), _item("neg", 5, 4, 43)]


# x0 + x1 <= 4 and x0 = 2 twice, the two equalities with zeros where the senses put their slack columns:
# phase 1 gives each an artificial column and drops one of the two rows
DEPENDENT = lp([[0, -1, -1, 0, 0, 0], [4, 1, 1, 1, 0, 0], [2, 1, 0, 0, 0, 0], [2, 1, 0, 0, 0, 0]])
SHORT_AT = 1


def short_uniform():
    """four 4 x 6 tableaux (m = 3, ns = 2 under three <= senses), LP 1 DEPENDENT"""
    stack = gen.mixed_stack(3, 2, range(1, 5))
    stack[SHORT_AT] = DEPENDENT
    return stack


def short_ragged():
    """the same with LPs of three shapes around it; n_i = ns_i + m_i, every sense <="""
    return [gen.tableau("mixed", 2, 3, 5), DEPENDENT.copy(), gen.tableau("mixed", 5, 1, 6), gen.tableau("mixed", 3, 2, 7)]


def full_rank(seed=9):
    """what replaces DEPENDENT: a canonical LP of its shape"""
    return gen.tableau("mixed", 3, 2, seed)


# ------------------------------------------------------------------ non-finite and extreme right-hand sides
EXTREME = ["+inf", "-inf", "nan", "-0.0", "5e-324", "1e308 twice", "1e-320"]


def overflow_pair(T, slack):
    """the first two rows k1 < k2 for which some tableau row's products with 1e308 are both finite and their
    sum is not; (0, 1) where there is none"""
    with np.errstate(all="ignore"):
        cols = [np.where(s > 0, 1.0, -1.0) * T[:, abs(s)] * 1e308 for s in slack]
        for k1 in range(len(cols)):
            for k2 in range(k1 + 1, len(cols)):
                if (np.isfinite(cols[k1]) & np.isfinite(cols[k2]) & np.isinf(cols[k1] + cols[k2])).any():
                    return k1, k2
    return 0, 1


def extreme_rhs(b, k, pair=(0, 1)):
    """[z, b] with variation k of EXTREME written over rows of b (m >= 5)"""
    r = np.concatenate([[0.0], np.asarray(b, dtype=np.float64)])
    name = EXTREME[k % len(EXTREME)]
    if name == "+inf":
        r[1] = np.inf
    elif name == "-inf":
        r[2] = -np.inf
    elif name == "nan":
        r[3] = np.nan
    elif name == "-0.0":
        r[0] = r[1] = r[4] = -0.0
    elif name == "5e-324":
        r[4] = 5e-324
    elif name == "1e308 twice":
        r[1 + pair[0]] = r[1 + pair[1]] = 1e308
    else:
        r[5] = 1e-320
    return r


EXTREME_BATCHES = dict(small=(SMALL, 14, "lds"), large=(LARGE, 7, "device"))     # (m, ns), LPs, place
# what run(RULE_DUAL) ends with after each, LP by LP (test_dual_cases_cpu.py walks them on the oracle)
EXTREME_STATUS = dict(small=[1, -5, 1, 1, 1, 1, 1, 1, -5, 1, 1, 1, -5, 1], large=[-5, -5, 1, 1, 1, -5, 1])


def extreme_host(which):
    """the oracle's optimal tableaux of the batch's LPs under their extreme right-hand sides -> [(T, rhs)]"""
    (m, ns), B, _ = EXTREME_BATCHES[which]
    slack = slack_table([_lib.SENSE_LE] * m, ns)
    out = []
    for i in range(B):
        wm = warm(m, ns, 1 + i, "scale")
        b = gen.tableau("mixed", m, ns, 1 + i)[1:, 0]                   # the LP's own b underneath
        rhs = extreme_rhs(b, i, overflow_pair(wm["opt"], slack))
        out.append((set_rhs(wm["opt"], slack, rhs), rhs))
    return out


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


# ------------------------------------------------------------------ device: set_rhs and resolve
def snapshot(eng):
    T = eng.download()
    return dict(T=[np.array(t) for t in T], basis=[np.array(v) for v in eng.get_basis()],
                log=[eng.log(i).tolist() for i in range(eng.count)] if eng.log_cap else None)


def assert_untouched(after, before, lps):
    for i in lps:
        assert same_bits(after["T"][i], before["T"][i]), i
    assert all(np.array_equal(a, b) for a, b in zip(after["basis"], before["basis"]))
    assert after["log"] == before["log"]


def assert_set_rhs(eng, slacks, rhs, first=0):
    """set_rhs on LPs [first, first + len(rhs)) against the host loop on the downloaded tableaux"""
    before = snapshot(eng)
    eng.set_rhs(rhs, first)
    after = snapshot(eng)
    window = range(first, first + len(rhs))
    for k, i in enumerate(window):
        want = set_rhs(before["T"][i], slacks[i], rhs[k])
        assert same_bits(after["T"][i][:, 0], want[:, 0]), i
        assert same_bits(after["T"][i][:, 1:], before["T"][i][:, 1:]), i
    assert_untouched(after, before, [i for i in range(eng.count) if i not in window])
    return before, after


def host_resolve(T, basis, slack, rhs, cap):
    """the host loop, then the host walk -> (status, npiv, x of all n columns, objective)"""
    w = walk(set_rhs(T, slack, rhs), cap)
    basis = np.array(basis)
    for r, c in w["log"]:
        basis[r] = c
    return w["status"], w["npiv"], solution_x(w["T"], basis), -w["T"][0, 0]


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
