"""Shared oracle and inputs of the warm re-optimisation tests
(test_reopt_cases_cpu.py, test_batch_reopt_cpu.py, test_gpu_batch_reopt.py).

The oracle of lp_reopt_set_costs is reprice() below: the header's loop, plain
float64 `acc - c * t`, one scalar at a time.  The oracle of lp_reopt_set_general
is general_standard_form's column 0 pushed through _dual_cases.set_rhs.  What
follows either is _dual_cases.walk (the dual side) or F64Tableau.solve (the
primal side).  Nothing here comes from the device.  A plain module: no fixtures,
no GPU."""
import numpy as np

import _dual_cases as dc
import _general_cases as gc
import _problem_cases as pc
from lpsol_amd import _lib, solution_x
from lpsol_amd import generators as gen
from lpsol_amd import problem as pr
from oracle.f64 import F64Tableau

same_bits = dc.same_bits
S_TILT, S_SWING = 21, 23            # streams of their own (the generators use 1..3 and 7, _dual_cases 11..13)
SMALL, MID, LARGE = (8, 10), (24, 24), (40, 40)         # (m, ns) of the generator call
SEEDS = {SMALL: range(1, 65), MID: range(1, 33), LARGE: range(1, 33)}
FRACTION = 1e-6


# ------------------------------------------------------------------ the cost loop
def reprice(T, basis, costs):
    """a copy of the stored tableau T with the new row 0:
    acc = costs[j]; for r: k = basis[r]; if 0 <= k < n: acc = acc - costs[1+k] * T[1+r][j]"""
    T = np.array(T, dtype=np.float64)
    costs = np.asarray(costs, dtype=np.float64)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    assert costs.shape == (n + 1,) and len(basis) == m
    with np.errstate(all="ignore"):
        for j in range(n + 1):
            acc = costs[j]
            for r in range(m):
                k = int(basis[r])
                if k < 0 or k >= n:
                    continue
                prod = costs[1 + k] * T[1 + r, j]
                acc = acc - prod
            T[0, j] = acc
    return T


def basis_of(start, log):
    basis = np.array(start, dtype=np.int32)
    for r, c in log:
        basis[r] = c
    return basis


# ------------------------------------------------------------------ cost perturbations
def tilt(c, seed):
    """c_j * U{0..128}/64: the sign stays, the order of the ratios does not"""
    i = np.arange(len(c), dtype=np.uint64)
    return c * (gen.uint_range(1000 + seed, S_TILT, i, 0, 128) / 64.0)


def swing(c, seed):
    """-c_j where U{0..3} is 0: a quarter of the costs change sign"""
    i = np.arange(len(c), dtype=np.uint64)
    return np.where(gen.uint_range(1000 + seed, S_SWING, i, 0, 3) == 0, -c, c)


PERTURB = dict(tilt=tilt, swing=swing)
_COST = {}


def cost_row(T0, ns, c):
    """the new row 0 as lp_reopt_set_costs takes it: the stored _z cell, c, +0.0 under the slacks"""
    row = np.zeros(T0.shape[1])
    row[0] = T0[0, 0]
    row[1:ns + 1] = c
    return row


def cost_case(m, ns, seed, how):
    """the `mixed` LP solved by lpf_solve, then given new costs -> dict: opt and basis the oracle's optimal
    tableau and basis, c the new costs, row the new row 0, T the warm tableau reprice() makes of opt, warm
    and cold the (status, log, nstd, T) of lpf_solve on T and on the LP uploaded with c; computed once"""
    key = (m, ns, seed, how)
    if key not in _COST:
        T0 = gen.tableau("mixed", m, ns, seed)
        o = F64Tableau(T0)
        st, log, _ = o.solve()
        assert st == _lib.OPTIMAL
        basis = basis_of(np.arange(ns, ns + m), log)
        c = PERTURB[how](T0[0, 1:ns + 1], seed)
        row = cost_row(T0, ns, c)
        T = reprice(o.T, basis, row)
        cold0 = T0.copy()
        cold0[0] = row
        out = dict(T0=T0, opt=o.T, basis=basis, c=c, row=row, T=T, cold_pivots0=len(log))
        for name, start in (("warm", T), ("cold", cold0)):
            w = F64Tableau(start)
            wst, wlog, wnstd = w.solve()
            out[name] = dict(status=wst, log=[list(map(int, p)) for p in wlog], nstd=wnstd, T=w.T,
                             objective=-w.T[0, 0])
        _COST[key] = out
    return _COST[key]


def host_primal(T, basis, row, cap=-1):
    """the host loop, then lpf_solve -> (status, npiv, nstd, log, x of all n columns, objective, T)"""
    w = F64Tableau(reprice(T, basis, row))
    st, log, nstd = w.solve(cap)
    basis = basis_of(basis, log)
    return st, len(log), nstd, [list(map(int, p)) for p in log], solution_x(w.T, basis), -w.T[0, 0], w.T


# ------------------------------------------------------------------ branch workloads
_BRANCH = {}


def boxed_lp(m, ns, seed):
    """`mixed` m x ns with every variable BOXED [0, 2], minimising -> (P, sense, kind, lb, ub)"""
    T0 = gen.tableau("mixed", m, ns, seed)
    return (pc.block(T0, ns), np.full(m, pc.LE, dtype=np.int8), np.full(ns, gc.BOXED, dtype=np.int8), np.zeros(ns),
            np.full(ns, 2.0))


def general_slack(sense, kind):
    """the slack table of the standard form's m' rows (no equalities here)"""
    kind = np.asarray(kind)
    nf, nb = int((kind == gc.FREE).sum()), int((kind == gc.BOXED).sum())
    return dc.slack_table(list(sense) + [pc.LE] * nb, len(kind) + nf)


def branch_bounds(x, lb, ub, way):
    """the branching variable (the first fractional x_j, or None) and the new bounds"""
    lb, ub = np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)
    frac = np.nonzero(np.abs(x - np.round(x)) > FRACTION)[0]
    if len(frac) == 0:
        return None, lb, ub
    j = int(frac[0])
    if way == "down":
        ub[j] = np.floor(x[j])
    else:
        lb[j] = np.ceil(x[j])
    return j, lb, ub


def host_general_rhs(T, P, sense, kind, lb, ub, maximise=False):
    """the stored standard-form tableau T with the column 0 lp_reopt_set_general leaves: the new standard
    form's column 0 pushed through the host set_rhs"""
    col0 = pr.general_standard_form(P, lb, ub, sense, kind, maximise)[:, 0]
    return dc.set_rhs(T, general_slack(sense, kind), col0)


def host_general_dual(T, basis, P, sense, kind, lb, ub, maximise=False, cap=dc.CAP):
    """that, the host dual walk and general_recover -> dict(status, npiv, log, T, x, z, xstd)"""
    w = dc.walk(host_general_rhs(T, P, sense, kind, lb, ub, maximise), cap)
    xs = solution_x(w["T"], basis_of(basis, w["log"]))
    x, z = pr.general_recover(xs, w["T"][0, 0], lb, ub, kind, maximise)
    return dict(status=w["status"], npiv=w["npiv"], log=w["log"], T=w["T"], x=x, z=float(z), xstd=xs)


def branch_case(m, ns, seed, way):
    """boxed_lp solved cold, then branched -> dict: T0 the standard form, opt / basis the oracle's optimal
    tableau and basis, x its x, j the branching variable, lb / ub the new bounds, warm the host chain's
    answer, cold the two-phase oracle's on the new standard form; computed once"""
    key = (m, ns, seed, way)
    if key not in _BRANCH:
        from oracle.phase1 import solve_lp
        P, sense, kind, lb, ub = boxed_lp(m, ns, seed)
        T0 = pr.general_standard_form(P, lb, ub, sense, kind, False)
        o = F64Tableau(T0)
        st, log, _ = o.solve()
        assert st == _lib.OPTIMAL
        mp = T0.shape[0] - 1
        basis = basis_of(np.arange(ns, ns + mp), log)
        x, _ = pr.general_recover(solution_x(o.T, basis), o.T[0, 0], lb, ub, kind, False)
        j, lb2, ub2 = branch_bounds(x, lb, ub, way)
        warm = host_general_dual(o.T, basis, P, sense, kind, lb2, ub2)
        rep = solve_lp(pr.general_standard_form(P, lb2, ub2, sense, kind, False), report=True)
        cold = dict(status=int(rep["status"]), z=float(rep["objective"]))
        _BRANCH[key] = dict(P=P, sense=sense, kind=kind, T0=T0, opt=o.T, basis=basis, x=x, j=j, lb=lb2, ub=ub2,
                            warm=warm, cold=cold)
    return _BRANCH[key]


# ------------------------------------------------------------------ the hand LP
# min x1 + x2 subject to x1 - x2 <= 1: optimal 0 at the origin
HAND_C, HAND_A, HAND_B = np.array([1.0, 1.0]), np.array([[1.0, -1.0]]), np.array([1.0])
HAND_NEW = [(np.array([-1.0, 1.0]), "optimal", -1.0, [1.0, 0.0]), (np.array([-1.0, -1.0]), "unbounded", None, None)]

# ------------------------------------------------------------------ the ragged batch of the set_costs tests
RAGGED_SHAPES = [(8, 10), (1, 1), (3, 5), (40, 40), (1, 6), (5, 4), (24, 24), (2, 1)]     # (m, ns)


def ragged_tableaux(seed0=700):
    return [gen.tableau("mixed", m, ns, seed0 + i) for i, (m, ns) in enumerate(RAGGED_SHAPES)]


def some_costs(n, seed):
    """n + 1 dyadic values of both signs"""
    return (gen.uint_range(seed, S_TILT, np.arange(n + 1, dtype=np.uint64), 0, 256) - 128.0) / 32.0


# ------------------------------------------------------------------ kinds cycling, to be maximised
def cycled_lp(m, ns, seed):
    """`mixed` m x ns with the costs negated, to be maximised, kinds cycling LOWER, BOXED, UPPER with
    lb = 1/8 and ub = 3/2 where the kind has the bound -> (P, sense, kind, lb, ub)"""
    P = pc.block(gen.tableau("mixed", m, ns, seed), ns).copy()
    P[0, 1:] = -P[0, 1:]
    kind = np.array([(gc.LOWER, gc.BOXED, gc.UPPER)[j % 3] for j in range(ns)], dtype=np.int8)
    lb = np.where(kind == gc.UPPER, -gc.INF, 0.125)
    ub = np.where(kind == gc.LOWER, gc.INF, 1.5)
    return P, np.full(m, pc.LE, dtype=np.int8), kind, lb, ub


def tighten(kind, lb, ub, seed):
    """new bounds of the same pattern: every finite ub down by U{0..32}/64, every finite lb up by U{0..8}/64"""
    j = np.arange(len(kind), dtype=np.uint64)
    lb2 = np.where(np.isfinite(lb), lb + gen.uint_range(1000 + seed, S_TILT, j, 0, 8) / 64.0, lb)
    ub2 = np.where(np.isfinite(ub), ub - gen.uint_range(1000 + seed, S_SWING, j, 0, 32) / 64.0, ub)
    return lb2, ub2
