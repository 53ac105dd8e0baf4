"""Shared inputs of the contract tests (test_contract_cpu.py,
test_gpu_batch_contract.py, test_gpu_engine_contract.py): hand-built LPs with
non-finite cells, negative b and zero pivots, stacks with dirty cells, rows
scaled to the ends of the exponent range, one distinct value per lp_tol field,
and the comparison helpers.  A plain module: no fixtures, no GPU."""
import numpy as np

from lpsol_amd import generators as gen
from oracle.f64 import DEFAULT_TOL, F64Tableau

# lp_status (include/lpgpu.h)
PIVOTED, OPTIMAL, UNBOUNDED, CAP_REACHED, OBJ_INCREASED = 0, 1, 2, -4, -6

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------

def same_bits(a, b):
    """identical shape and bytes (finite inputs: the only comparison used)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_values(a, b):
    """equal shape, NaN in the same cells, identical bytes everywhere else
    (signed zeros and infinities included).  NaN bit patterns are left out: an
    invalid operation gives a differently signed default NaN on the host and on
    the device.  Only for inputs that may hold non-finite values."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# ---------------------------------------------------------------------------
# the oracle, with every result of a call in one record
# ---------------------------------------------------------------------------

def oracle_solve(T, cap, tol=None):
    """lpf_solve with a cap -> dict(status, log, npiv, nstd, T, z)"""
    o = F64Tableau(T, tol)
    st, log, nstd = o.solve(cap=cap, logcap=max(cap, 1))
    return dict(status=st, log=log.tolist(), npiv=len(log), nstd=nstd, T=o.T, z=-o.T[0, 0])


def oracle_run(T, rule, k, tol=None):
    """lpf_run -> dict(status, log, npiv, T, z)"""
    o = F64Tableau(T, tol)
    st, log = o.run(rule, k)
    return dict(status=st, log=log.tolist(), npiv=len(log), nstd=0, T=o.T, z=-o.T[0, 0])


def result_differs(a, b):
    """two records of oracle_solve / oracle_run (or a GPU result in the same
    form) differ in anything a contract test compares"""
    return not (a["status"] == b["status"] and a["log"] == b["log"] and a["nstd"] == b["nstd"]
                and same_values(a["T"], b["T"]))


# ---------------------------------------------------------------------------
# hand-built cases
# ---------------------------------------------------------------------------

def base_lp():
    """3 x 5: min -x1 + x2, column 1 enters; ratios 3, 2, 3 -> row 1 leaves"""
    T = np.zeros((4, 6))
    T[0, 1:3] = [-1.0, 1.0]
    T[1] = [3.0, 1.0, 0.0, 1.0, 0.0, 0.0]
    T[2] = [4.0, 2.0, 0.0, 0.0, 1.0, 0.0]
    T[3] = [9.0, 3.0, 0.0, 0.0, 0.0, 1.0]
    return T


def overflow_lp(all_inf):
    """as tests/test_gpu_batch.py: an eligible ratio overflows to +inf"""
    T = np.zeros((4, 6))
    T[0, 1:3] = [-1.0, 1.0]
    T[1] = [1e308, 1e-3, 0.0, 1.0, 0.0, 0.0]
    T[2] = [4.0, 2.0, 0.0, 0.0, 1.0, 0.0]
    T[3] = [9.0, 3.0, 0.0, 0.0, 0.0, 1.0]
    if all_inf:
        T[2] = [1e308, 2e-3, 0.0, 0.0, 1.0, 0.0]
        T[3] = [1e308, 4e-3, 0.0, 0.0, 0.0, 1.0]
    return T


def _case(name, edit, status, log, nstd, *, tol=None, cap=8, untouched=False, T=None):
    T = base_lp() if T is None else T
    if edit:
        edit(T)
    return dict(name=name, T=T, tol=tol, cap=cap, status=status, log=log, nstd=nstd,
                untouched=untouched)


def _set(i, j, v):
    def edit(T):
        T[i, j] = v
    return edit


def _zero_col(T):
    T[1:, 1] = 0.0


def _a_at_tol(T):
    T[2, 0] = 5e-324
    T[2, 1] = 1e-9


def _neighbour(T):
    T[1, 0] = 1.0


# status, log and nstd are literals: what oracle/lp_f64.c answers with cap 8
CASES = [
    _case("nan_b_first", _set(1, 0, NAN), UNBOUNDED, [], 0, untouched=True),
    _case("nan_b_later", _set(3, 0, NAN), OPTIMAL, [[1, 0]], 1),
    _case("nan_a", _set(2, 1, NAN), OPTIMAL, [[0, 0]], 1),
    _case("nan_cost", _set(0, 2, NAN), OPTIMAL, [[1, 0]], 1),
    _case("neginf_cost", _set(0, 2, -INF), OPTIMAL, [], 0, untouched=True),
    _case("neginf_cost_tie0", _set(0, 2, -INF), OPTIMAL, [], 0, tol=dict(cost_tie=0.0),
          untouched=True),
    _case("neg_b", _set(2, 0, -4.0), OBJ_INCREASED, [[1, 0]], 1),
    _case("tiny_neg_b", _set(2, 0, -1e-10), OBJ_INCREASED, [[1, 0]], 1),
    _case("zero_pivot", _zero_col, CAP_REACHED, [[0, 0]] * 5, 5, tol=dict(pivot=-1.0), cap=5,
          untouched=True),
    _case("a_at_tol", _a_at_tol, OPTIMAL, [[0, 0]], 1),
    _case("overflow_one", None, OPTIMAL, [[1, 0]], 1, T=overflow_lp(False)),
    _case("overflow_all", None, OPTIMAL, [[0, 0]], 1, T=overflow_lp(True)),
    _case("overflow_neighbour", _neighbour, OPTIMAL, [[1, 0]], 1, T=overflow_lp(False)),
]
CASE_NAMES = [c["name"] for c in CASES]


def case(name):
    return CASES[CASE_NAMES.index(name)]


# (m, n, row_at): 4x5 and 8x18 run on one wave, 70x40 (2911 elements) on four,
# once with the case's rows first and once in another wave / stride than thread 0's
EMBEDDINGS = [
    (4, 5, (1, 2, 3)),
    (8, 18, (1, 2, 3)),
    (70, 40, (1, 2, 3)),
    (70, 40, (65, 66, 70)),
]


def embed(c, m, n, row_at):
    """the case's LP inside an (m+1) x (n+1) tableau: its constraint rows at
    tableau rows `row_at`, its columns at 1.., added columns with cost +1 and
    zero entries, added rows with b = 1 and zero entries"""
    S = c["T"]
    ms, ns = S.shape[0] - 1, S.shape[1] - 1
    assert len(row_at) == ms and m >= ms and n >= ns
    T = np.zeros((m + 1, n + 1))
    T[0, :ns + 1] = S[0]
    T[0, ns + 1:] = 1.0
    T[1:, 0] = 1.0
    for k, R in enumerate(row_at):
        T[R, :ns + 1] = S[1 + k]
    return T


def mapped_log(c, row_at):
    """the case's literal log with its rows moved to row_at.  One exception:
    zero_pivot runs with pivot = -1, which makes the added all-zero rows
    eligible too (0 > -1, ratio 1 / 0 = +inf like the case's own rows), so the
    first row of the tableau leaves whether it is the case's or an added one:
    the log is [0, 0] five times at every placement."""
    if c["name"] == "zero_pivot":
        return [list(p) for p in c["log"]]
    return [[row_at[r] - 1, col] for r, col in c["log"]]


def case_stack(m, n, row_at, names=None):
    """every case (or those named) embedded alike -> (cases, [B, m+1, n+1])"""
    cs = CASES if names is None else [case(x) for x in names]
    return cs, np.stack([embed(c, m, n, row_at) for c in cs])


# ---------------------------------------------------------------------------
# dirty stacks
# ---------------------------------------------------------------------------

DIRT = [NAN, INF, -INF, -0.0, 1e308, -1e308, 5e-324, 1e-300, 1e-9, -1e-9]
DIRTY_SHAPES = [(8, 10, 2), (31, 32, 4), (40, 40, 6)]      # (m, ns, cells overwritten)
DIRTY_CAP = 256


def dirty_stack(m, ns, k, seeds):
    out = []
    for s in seeds:
        T = gen.tableau("mixed", m, ns, s)
        rng = np.random.default_rng(1000 + s)
        for _ in range(k):
            i = rng.integers(0, T.shape[0])
            j = rng.integers(0, T.shape[1])
            T[i, j] = DIRT[rng.integers(0, len(DIRT))]
        out.append(T)
    return np.stack(out)


# ---------------------------------------------------------------------------
# exponent range
# ---------------------------------------------------------------------------

SCALE_TOL = dict(pivot=0.0, zero=0.0)        # the two absolute tolerances
SCALED_SHAPES = [(8, 10), (31, 32), (31, 33), (64, 64)]


def scaled(T, s, down):
    """every constraint row times its own power of two: no ratio and no
    normalised pivot row changes.  down reaches into the denormals."""
    T = np.array(T, dtype=np.float64)
    m = T.shape[0] - 1
    rng = np.random.default_rng(77 + s)
    if down:
        k = -np.abs(rng.integers(-1000, 1001, m)) - 40
    else:
        k = rng.integers(-480, 481, m)
    T[1:] = np.ldexp(T[1:], k[:, None])
    return T


def scaled_stack(m, ns, seeds, down):
    return np.stack([scaled(gen.tableau("mixed", m, ns, s), s, down) for s in seeds])


# ---------------------------------------------------------------------------
# one distinct value per lp_tol field
# ---------------------------------------------------------------------------

TOL_VALUES = dict(cost=0.3, cost_tie=0.5, pivot=0.2, zero=0.4, ratio_tie=0.25)
STALL = 1e9
FIELDS = list(TOL_VALUES)
ALL_SIX = dict(TOL_VALUES, stall=STALL)
# each field alone, then all six together
TOL_SETS = [(f, {f: v}) for f, v in TOL_VALUES.items()] + [("all_six", ALL_SIX)]
TOL_IDS = [name for name, _ in TOL_SETS]


def swapped(tol, a, b):
    """the lp_tol a kernel would use if it read field b where it means a"""
    d = dict(DEFAULT_TOL)
    d.update(tol or {})
    d[a], d[b] = d[b], d[a]
    return d


def km8_padded():
    """Klee-Minty d = 8 with 214 inert columns (cost +1, zero entries):
    9 x 231 = 2079 elements, the four-wave kernel"""
    K = gen.klee_minty(8)
    T = np.zeros((9, 231))
    T[:, :17] = K
    T[0, 17:] = 1.0
    return T


# ---------------------------------------------------------------------------
# which input each single-LP path runs per field (test_gpu_engine_contract.py;
# test_contract_cpu.py asserts that the field changes the oracle's result there)
# ---------------------------------------------------------------------------

RULE_STANDARD, RULE_MIN_INDEX = 0, 1
ENGINE_CAP = 400        # all six fields together cycle on 130x70: every engine solve is capped


def engine_plan(path, field):
    """-> (call, rule, k, inputs): call "solve" (k = cap) or "run" (k pivots of rule).

    cost decides only optimality under the standard rule (g < -cost), which a
    run of a few dozen pivots never reaches, so the fixed-rule runs take the
    min-index rule for it (c_j < -cost picks the column); the XCD-shard run
    also takes seed 2 there (at seed 1 the first columns all pass 0.3).
    Measured: the run of 12 on tall 6000x8 ends optimal after 7 pivots at
    seed 1 (5 to 8 with a field set) and after 8 at seed 2, min-index."""
    if path == "kernels":
        return "solve", RULE_STANDARD, ENGINE_CAP, [gen.tableau("mixed", 40, 30, s) for s in (1, 2)]
    if path == "persistent_solve":
        return "solve", RULE_STANDARD, ENGINE_CAP, [gen.tableau("mixed", 130, 70, s) for s in (1, 2)]
    if path in ("persistent_run_8", "persistent_run_64"):
        rule = RULE_MIN_INDEX if field == "cost" else RULE_STANDARD
        return "run", rule, 40, [gen.tableau("mixed", 130, 70, s) for s in (1, 2)]
    if path == "group3":
        return "solve", RULE_STANDARD, ENGINE_CAP, [gen.tableau("mixed", 130, 70, 1)]
    if path == "xcd_shards":
        if field == "cost":
            return "run", RULE_MIN_INDEX, 12, [gen.tableau("tall", 6000, 8, 2)]
        return "run", RULE_STANDARD, 12, [gen.tableau("tall", 6000, 8, 1)]
    raise KeyError(path)


ENGINE_PATHS = ["kernels", "persistent_solve", "persistent_run_8", "persistent_run_64", "group3",
                "xcd_shards"]


def oracle_call(call, rule, k, T, tol=None):
    return oracle_solve(T, k, tol) if call == "solve" else oracle_run(T, rule, k, tol)


# the column scans and pivot_checked: mixed 40x30 seed 2 (at seed 1 cost = 0.3
# changes nothing along the walk and pivot = 0.2 no min-ratio row)
SCAN_FIELDS = ["cost", "pivot", "zero", "ratio_tie"]
CHECKED_FIELDS = ["pivot", "zero", "ratio_tie"]


def scan_input():
    return gen.tableau("mixed", 40, 30, 2)


def scan_walk(T, tol, k=10):
    """the oracle's answers along k max-increase pivots:
    [find_all, find_max_increase] per state"""
    o = F64Tableau(T, tol)
    out = []
    for _ in range(k):
        fa = [list(p) for p in o.find_all()]
        w = o.find_max_increase()
        out.append([fa, list(w) if isinstance(w, tuple) else w])
        if isinstance(w, str):
            break
        o.pivot(*w)
    return out, o.T


def checked_pair(T, tol):
    """-> (accepted, refused): a pivot that Simplex.pivot's min-ratio check
    takes under tol but not under the default lp_tol, and one it refuses under
    tol (one the default takes, where there is one, else the first eligible
    row of the same column outside the band).  Membership of lpf_find_all's
    list is the check: row eligible and q <= g + ratio_tie |g|."""
    S_def = F64Tableau(T).find_all()
    S_tol = F64Tableau(T, tol).find_all()
    acc = next(p for p in S_tol if p not in S_def)
    lost = [p for p in S_def if p not in S_tol]
    if lost:
        return acc, lost[0]
    d = dict(DEFAULT_TOL)
    d.update(tol)
    c = acc[1]
    r = next(i for i in range(T.shape[0] - 1)
             if T[1 + i, 1 + c] > d["pivot"] and (i, c) not in S_tol)
    return acc, (r, c)


# a field b to swap each field a with (the self-check of test_contract_cpu.py)
SWAP_WITH = dict(cost="pivot", cost_tie="ratio_tie", pivot="cost", zero="pivot",
                 ratio_tie="stall", stall="ratio_tie")
