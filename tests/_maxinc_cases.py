"""Shared oracle, inputs and device helpers of the max-increase batch tests
(test_maxinc_cases_cpu.py, test_gpu_batch_maxinc.py).

The oracle of lp_batch_run(b, LP_RULE_MAX_INCREASE, k, ...) is a host loop over
oracle.f64.F64Tableau.find_max_increase() and .pivot(r, c) (oracle/lp_f64.c:
lpf_find_max_increase, lpf_pivot), exactly as include/lpgpu.h states the rule:
'optimal' / 'unbounded' end the LP, c < 0 ends it LP_BAD_PIVOT, r < 0 ends it
LP_UNBOUNDED, else the pivot is applied, logged and counted.  A plain module:
no fixtures; nothing here touches the GPU until a device helper is called."""
import numpy as np

from lpsol_amd import _lib
from lpsol_amd import generators as gen
from oracle.f64 import F64Tableau

MAXINC = 2          # LP_RULE_MAX_INCREASE
CAP = 128           # every generator LP of these tests ends 'optimal' in at most 104 pivots

# ------------------------------------------------------------------ oracle
_WALKS = {}


def walk(T, k=CAP, tol=None):
    """k steps of the rule on a copy of T -> dict(status, log, T, npiv); computed once per input"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    key = (T.shape, T.tobytes(), int(k), tuple(sorted((tol or {}).items())))
    if key not in _WALKS:
        o = F64Tableau(T, tol)
        log, status = [], _lib.PIVOTED
        with np.errstate(all="ignore"):
            while len(log) < k:
                got = o.find_max_increase()
                if got == "optimal":
                    status = _lib.OPTIMAL
                    break
                if got == "unbounded":
                    status = _lib.UNBOUNDED
                    break
                r, c = got
                if c < 0:
                    status = _lib.BAD_PIVOT
                    break
                if r < 0:
                    status = _lib.UNBOUNDED
                    break
                o.pivot(r, c)
                log.append([r, c])
        o.T.setflags(write=False)
        _WALKS[key] = dict(status=status, log=log, T=o.T, npiv=len(log))
    return _WALKS[key]


def start_basis(m):
    """a starting basis that names no column: every row keeps its own mark until a pivot writes it"""
    return -1 - np.arange(m, dtype=np.int32)


def basis_after(m, log):
    b = start_basis(m)
    for r, c in log:
        b[r] = c
    return b.tolist()


def same_bits(a, b):
    """bit for bit, a NaN matching any NaN (the sign and payload of a NaN an
    operation makes are the hardware's, not the contract's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ------------------------------------------------------------------ inputs
def lp(rows):
    return np.array(rows, dtype=np.float64)


TIE = lp([[0, -2, -1, -2, 0, 0], [4, 1, 0, 0, 1, 0], [4, 0, 1, 1, 0, 1]])


def band(eps):
    T = TIE.copy()
    T[0, 1] = -2 + eps
    return T


BAND_IN, BAND_OUT = band(1e-12), band(1e-10)
NOT_STANDARD = lp([[0, -3, -2, 0, 0], [1, 1, 0, 1, 0], [9, 0, 1, 0, 1]])
TOL_COST = lp([[0, -1e-10, -2, 0, 0], [1e12, 1, 0, 1, 0], [1, 0, 1, 0, 1]])
UNBOUNDED_WINS = lp([[0, -5, -1, -1e-3, 0, 0], [4, 1, 0, -1, 1, 0], [4, 0, 1, 0, 0, 1]])
# the one eligible ratio of column 0 is 1e301 / 1e-8 = +inf
OVERFLOW = lp([[0, -1, 0, 0], [1e301, 1e-8, 1, 0], [4, 0, 0, 1]])
NO_COLUMN = lp([[0, -1e300, -1, 0, 0], [1e300, 1e-8, 1, 1, 0], [4, 0, 1, 0, 1]])
NAN_COST = lp([[0, np.nan, -1, 0, 0], [4, 1, 1, 1, 0], [4, 1, 2, 0, 1]])
NAN_CELL = lp([[0, -1, -1, 0, 0], [4, np.nan, 1, 1, 0], [6, 2, 1, 0, 1]])

# name -> tableau; the constructed cases of the GPU suite, as one ragged batch per tolerance set
CASES = dict(tie=TIE, band_in=BAND_IN, band_out=BAND_OUT, not_standard=NOT_STANDARD, tol_cost=TOL_COST,
             unbounded_wins=UNBOUNDED_WINS, overflow=OVERFLOW, no_column=NO_COLUMN, nan_cost=NAN_COST,
             nan_cell=NAN_CELL)
TOLS = (None, dict(ratio_tie=0.0), dict(cost=0.0))

# the shapes at the edges of the lane mapping: (kind, m, ns); 3 seeds each
EDGES = [("tall", 64, 16), ("tall", 1, 1), ("mixed", 1, 1), ("mixed", 63, 63), ("mixed", 31, 32), ("mixed", 31, 33),
         ("mixed", 3, 197), ("mixed", 8, 292), ("mixed", 1, 70), ("mixed", 62, 1)]
EDGE_SEEDS = (1, 2, 3)


def shape_of(T):
    return T.shape[0] - 1, T.shape[1] - 1


def small_stack():
    return gen.mixed_stack(8, 10, range(1, 65))


def large_stack():
    return gen.mixed_stack(40, 40, range(1, 9))


# ------------------------------------------------------------------ device
def make_engine(stack, *, place="lds", team=1, log_cap=CAP):
    if isinstance(stack, np.ndarray):
        return _lib.BatchEngine(stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1, log_cap=log_cap, place=place,
                                team=team)
    return _lib.RaggedEngine([shape_of(T) for T in stack], log_cap=log_cap, place=place, team=team)


def load(eng, stack):
    """upload and attach start_basis to every LP"""
    eng.upload(stack)
    b = [start_basis(shape_of(T)[0]) for T in stack]
    eng.set_basis(np.stack(b) if isinstance(stack, np.ndarray) else b)


def records(eng, st, done):
    T, bs = eng.download(), eng.get_basis()
    return [dict(status=int(st[i]), npiv=int(done[i]), log=eng.log(i).tolist(), T=T[i], basis=list(map(int, bs[i])))
            for i in range(eng.count)]


def device_run(stack, k=CAP, *, rule=MAXINC, tol=None, chunk=None, place="lds", team=1, log_cap=CAP):
    """one lp_batch_run of a uniform stack or a list of LPs -> one record per LP"""
    eng = make_engine(stack, place=place, team=team, log_cap=log_cap)
    try:
        if tol:
            eng.set_tol(**tol)
        if chunk is not None:
            eng.set_chunk(chunk)
        load(eng, stack)
        return records(eng, *eng.run(rule, k))
    finally:
        eng.close()


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
