"""Shared oracle and inputs of the warm re-optimisation tests
(test_reopt_cases_cpu.py, test_batch_reopt_cpu.py, test_gpu_batch_reopt.py,
test_gpu_batch_reopt_edges.py).

The oracle of lp_reopt_set_costs is reprice() below: the header's loop, plain
float64 `acc - c * t`, one scalar at a time.  The oracle of lp_reopt_set_general
is general_standard_form's column 0 pushed through _dual_cases.set_rhs.  What
follows either is _dual_cases.walk (the dual side) or F64Tableau.solve (the
primal side).  Nothing expected here comes from the device.  A plain module:
no fixtures; nothing touches the GPU until one of the device helpers at the end
(assert_set_costs, assert_set_general, assert_dual) is called."""
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


# ------------------------------------------------------------------ the flat kernels across workgroups
# (test_gpu_batch_reopt_edges.py; the shapes are vetted by test_reopt_cases_cpu.py)
FLAT = dc.FLAT      # PLAN_FLAT_THREADS: lanes per workgroup of k_cost, k_general_restage, k_general_shift, k_rhs


def starts(lanes, first, count):
    """the lane each LP of the window begins at, and one past the last"""
    return np.concatenate([[0], np.cumsum(lanes[first:first + count])]).tolist()


# k_cost, ragged: a lane is one (LP, column) pair, n_i + 1 = ns_i + m_i + 1 lanes per LP.  189 LPs, 1110 lanes:
# 19, 4, 175 x 3 up to lane 548, 523 (the 2 x 520 LP), 9, 10 x 3
COST_BIG = 177
COST_SHAPES = [(8, 10), (1, 2)] + [(1, 1)] * 175 + [(2, 520), (3, 5)] + [(1, 1)] * 10       # (m, ns)
# (first, count): the whole batch, two that begin later, one that ends before the large LP, the large LP alone,
# an LP that lies wholly in the second workgroup of the whole batch (lanes 317..319), the last LP
COST_WINDOWS = [(0, 189), (1, 188), (2, 187), (2, 175), (COST_BIG, 1), (100, 1), (188, 1)]
COST_EDGES = {0: (257, 512), 1: (256, 511), 2: (255, 513)}      # first -> lanes at which an LP of the window begins
COST_INSIDE = 100
COST_UNIFORM = dict(m=6, ns=8, B=40, windows=[(0, 40), (5, 35), (16, 2)])       # 15 lanes per LP: 256 = 17 * 15 + 1


def cost_lanes(shapes=COST_SHAPES):
    return [m + ns + 1 for m, ns in shapes]


def cost_block_tableaux():
    return [gen.tableau("mixed", m, ns, 900 + i) for i, (m, ns) in enumerate(COST_SHAPES)]


# set_general, ragged: k_general_restage has 3 ns_i + m_i + 1 lanes per LP (the border), k_general_shift and the
# k_rhs after it m'_i + 1 (the standard form's rows).  Kinds: "boxed" is boxed_lp, "cycled" cycled_lp, maximised.
GENERAL_BIG = 107
GENERAL_FORMS = ([("boxed", 8, 10), ("cycled", 2, 1), ("boxed", 2, 1)]
                 + [(("cycled", "boxed")[j % 2], 1, 1) for j in range(104)]
                 + [("boxed", 258, 2), ("cycled", 3, 5)] + [(("boxed", "cycled")[j % 2], 1, 1) for j in range(12)])


GENERAL_SEEDS = {1: 801, 108: 908}          # under seed 300 + i these two are not optimal with every row live


def general_block_lps():
    """-> [(P, sense, kind, lb, ub, maximise)] of GENERAL_FORMS, seed 300 + i but for GENERAL_SEEDS"""
    out = []
    for i, (form, m, ns) in enumerate(GENERAL_FORMS):
        seed = GENERAL_SEEDS.get(i, 300 + i)
        lp = cycled_lp(m, ns, seed) if form == "cycled" else boxed_lp(m, ns, seed)
        out.append((*lp, form == "cycled"))
    return out


def general_rows(kind, m):
    """m' of the standard form: one more row per BOXED variable"""
    return m + int((np.asarray(kind) == gc.BOXED).sum())


def restage_lanes(lps):
    return [3 * len(lp[2]) + len(lp[1]) + 1 for lp in lps]


def shift_lanes(lps):
    return [general_rows(lp[2], len(lp[1])) + 1 for lp in lps]


def border_of(P, lb, ub, c=None):
    """the border lp_reopt_set_general takes: row 0 of P (c replaced where given), b, lb, ub"""
    return np.concatenate([[P[0, 0]], P[0, 1:] if c is None else c, P[1:, 0], lb, ub])


# (first, count): the whole batch, windows that begin later and still span three workgroups of the border map, the
# large LP alone, LPs that lie wholly in the second workgroup of the whole batch (60 of the border map, 100 of the
# row map), the last LP
GENERAL_WINDOWS = [(0, 121), (1, 120), (2, 119), (3, 118), (7, 114), (9, 112), (GENERAL_BIG, 1), (60, 1), (100, 1),
                   (120, 1)]
RESTAGE_EDGES = {0: (256, 511), 1: (257, 512), 3: (255,)}       # first -> lanes at which an LP of the window begins
SHIFT_EDGES = {0: (256,), 1: (257,), 3: (255,), 7: (511,), 9: (512,)}
RESTAGE_INSIDE, SHIFT_INSIDE = 60, 100
GENERAL_WALKED = (1, 120)           # the window whose LPs the GPU test walks, under general_squeezed()


def general_tight(lps, k):
    """the bounds window k of GENERAL_WINDOWS states, for every LP of the batch"""
    return [tighten(lp[2], lp[3], lp[4], 50 * k + i) for i, lp in enumerate(lps)]


_GENERAL = {}


def general_block_optima():
    """-> [(T, basis)] of general_block_lps on the two-phase oracle, every one optimal with all rows live;
    computed once"""
    if "opt" not in _GENERAL:
        from oracle.phase1 import solve_lp
        out = []
        for i, (P, sense, kind, lb, ub, mx) in enumerate(general_block_lps()):
            rep = solve_lp(pr.general_standard_form(P, lb, ub, sense, kind, mx), report=True)
            assert rep["status"] == _lib.OPTIMAL and rep["rows"] == general_rows(kind, len(sense)), i
            out.append((rep["T"], np.array(rep["bfs"], dtype=np.int32)))
        _GENERAL["opt"] = out
    return _GENERAL["opt"]


def squeeze(kind, lb, ub, x):
    """bounds of the same pattern that cut the optimum x off: the first variable with a finite ub that lies more
    than 1/64 above its lower end (lb, or x_j - 1 where lb is infinite) gets ub = the midpoint, rounded down to
    a multiple of 1/64; where there is none, the first variable with a finite lb gets lb = x_j + 1/4"""
    lb, ub = np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)
    for j in range(len(kind)):
        lo = lb[j] if np.isfinite(lb[j]) else x[j] - 1.0
        if np.isfinite(ub[j]) and x[j] > lo + 1.0 / 64.0:
            ub[j] = np.floor(32.0 * (x[j] + lo)) / 64.0
            return lb, ub
    j = int(np.nonzero(np.isfinite(lb))[0][0])
    lb[j] = x[j] + 0.25
    return lb, ub


def general_squeezed(lps):
    """the bounds of the walk of GENERAL_WALKED, for every LP of the batch: squeeze() at the oracle's optimum"""
    out = []
    for (P, sense, kind, lb, ub, mx), (T, basis) in zip(lps, general_block_optima()):
        x, _ = pr.general_recover(solution_x(T, basis), T[0, 0], lb, ub, kind, mx)
        out.append(squeeze(kind, lb, ub, x))
    return out


# ------------------------------------------------------------------ costs and borders near overflow and underflow
EXTREME_COSTS = ["1e308", "all 1e308", "5e-324", "2.2e-308", "mixed"]
TINY, SMALLEST_NORMAL = 5e-324, 2.2250738585072014e-308


def extreme_costs(n, k, seed):
    """n + 1 costs of both signs: variation k of EXTREME_COSTS"""
    sign = np.where(some_costs(n, seed) < 0, -1.0, 1.0)
    name = EXTREME_COSTS[k % len(EXTREME_COSTS)]
    if name == "1e308":
        return sign * 1e308
    if name == "all 1e308":
        return np.full(n + 1, 1e308)
    if name == "5e-324":
        return sign * TINY
    if name == "2.2e-308":
        return sign * 2.2e-308
    return np.where(np.arange(n + 1) % 2 == 0, sign * 1e308, sign * TINY)


def extreme_bounds(P, lb, ub, k):
    """-> (P with b of the extreme size, lb, ub): the finite bounds of a boxed LP scaled likewise"""
    P = np.array(P)
    size = (1e308, TINY, 2.2e-308, 1e308)[k % 4]
    m = P.shape[0] - 1
    sign = np.where(np.arange(m) % 3 == 0, -1.0, 1.0) if k % 4 == 3 else np.ones(m)
    P[1:, 0] = sign * size
    return P, (np.full(len(lb), -size) if k % 4 == 3 else np.zeros(len(lb))), np.full(len(ub), size)


def is_subnormal(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return (a > 0) & (a < SMALLEST_NORMAL)


# ------------------------------------------------------------------ device: set_costs and set_general
def pack(eng, rows):
    return list(rows) if hasattr(eng, "shapes") else np.stack(rows)


def assert_set_costs(eng, rows, first=0):
    """set_costs on LPs [first, first + len(rows)) against the host loop on the downloaded tableaux"""
    before = dc.snapshot(eng)
    eng.set_costs(rows, first)
    after = dc.snapshot(eng)
    window = range(first, first + len(rows))
    for k, i in enumerate(window):
        want = reprice(before["T"][i], before["basis"][i], rows[k])
        assert same_bits(after["T"][i][0], want[0]), i
        assert same_bits(after["T"][i][1:], before["T"][i][1:]), i
    dc.assert_untouched(after, before, [i for i in range(eng.count) if i not in window])
    return before, after


def assert_set_general(eng, lps, borders, bounds, first=0):
    """set_general on LPs [first, first + len(borders)) against the host: column 0 is the new standard
    form's pushed through set_rhs, nothing else moves, and the stored bounds are the new ones"""
    before = dc.snapshot(eng)
    eng.set_general(pack(eng, borders), first)
    after = dc.snapshot(eng)
    window = range(first, first + len(borders))
    for k, i in enumerate(window):
        P, sense, kind, _, _, mx = lps[i]
        want = host_general_rhs(before["T"][i], P, sense, kind, *bounds[k], mx)
        assert same_bits(after["T"][i][:, 0], want[:, 0]), i
        assert same_bits(after["T"][i][:, 1:], before["T"][i][:, 1:]), i
    dc.assert_untouched(after, before, [i for i in range(eng.count) if i not in window])
    # the stored blocks' bounds: what the recovery adds to x'
    xs, _ = eng.solution()
    xg, zg = eng.general_solution()
    for k, i in enumerate(window):
        P, sense, kind, _, _, mx = lps[i]
        x, z = pr.general_recover(np.asarray(xs[i]), after["T"][i][0, 0], *bounds[k], kind, mx)
        assert same_bits(np.asarray(xg[i]), x) and same_bits(zg[i], z), i
    return before, after


def assert_dual(new, before, lps, bounds, cap):
    for i, (P, sense, kind, _, _, mx) in enumerate(lps):
        w = host_general_dual(before["T"][i], before["basis"][i], P, sense, kind, *bounds[i], mx, cap)
        assert (new.status_code[i], new.npiv[i]) == (w["status"], w["npiv"]), i
        assert new.log(i).tolist() == w["log"][:dc.LOG_CAP], i
        assert same_bits(np.asarray(new.x[i]), w["x"]) and same_bits(new.objective[i], np.float64(w["z"])), i
    assert new.path == "dual" and not new.nstd.any() and not new.ninit.any()
    # y and the reduced costs are general_duals of the tableaux as they stand
    final = new._engine.download()
    for i, (P, sense, kind, _, _, mx) in enumerate(lps):
        y, r = pr.general_duals(final[i], sense, kind, mx)
        assert same_bits(np.asarray(new.y[i]), y) and same_bits(np.asarray(new.reduced_costs[i]), r), i
