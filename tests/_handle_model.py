"""A model of one lp_handle between calls (include/lpgpu.h), for
test_handle_model_cpu.py, test_gpu_handle_state.py and _handle_state_worker.py.

HandleModel answers what each C-ABI call must return and leaves its tableau as
the call must leave it, on top of oracle/lp_f64.c (oracle.f64.F64Tableau) and,
for the form checks, the host numpy predicates of lpsol_amd.Tableau.
sequence() draws a seeded list of calls over the whole ABI with the model's
answer recorded per call; replay() drives an engine (or an in-process shard
group) through such a list and compares bit for bit.  A plain module: no
fixtures, and nothing here needs a GPU until replay() is given an engine."""
import functools

import numpy as np

from lpsol_amd import Tableau
from lpsol_amd import generators as gen
from oracle.f64 import DEFAULT_TOL, F64Tableau, _tol

import _contract_cases as cc

# lp_status (include/lpgpu.h)
PIVOTED, OPTIMAL, UNBOUNDED = 0, 1, 2
ZERO_PIVOT, BAD_ARG, CAP_REACHED, BAD_PIVOT = -1, -2, -4, -5

RUN_K = (0, 1, 3, 17, 64, 70)
SOLVE_CAPS = (0, 5, -1)
BLOCKS = (1, 7, 48, 64, 0)
SCANS = ("find_all", "find_max_increase", "form_checks")
PUTS = ("put_row0", "put_one", "put_window", "put_last")
# every kind of call a sequence holds ("upload": the whole re-upload of a
# fresh seed once the LP is optimal or unbounded)
KINDS = ("run", "solve", "find", "pivot", "pivot_zero", "checked_ok", "checked_bad") + SCANS + PUTS + (
    "rows", "set_tol", "set_block", "objective")


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def window_status(m, n, row0, nrows, ldh, rb=0, rc=None):
    """lp_upload_rows / lp_download_rows: LP_BAD_ARG for a window outside the
    tableau, a leading dimension below n + 1 or, on a shard holding the
    constraint rows [rb, rb + rc), a row that is neither row 0 nor one of
    them; else LP_PIVOTED"""
    rc = m if rc is None else rc
    if row0 < 0 or nrows < 0 or row0 + nrows > m + 1 or ldh < n + 1:
        return BAD_ARG
    for R in range(row0, row0 + nrows):
        if R != 0 and not (1 + rb <= R < 1 + rb + rc):
            return BAD_ARG
    return PIVOTED


def host_checks(D):
    """the form checks as Engine.form_checks() returns them, from the host
    (numpy) predicates of lpsol_amd.Tableau on the same bits"""
    t = Tableau.fromArray(D)
    bc = [-2] * (D.shape[0] - 1)
    out = dict(canonical=t.isCanonical(bc), optimal=t.isOptimal(), unbounded=t.isUnbounded(),
               infeasible=t.isInfeasible(), degenerate=t.isDegenerate())
    out["bcols"] = None if all(x == -2 for x in bc) else bc     # untouched where some b < 0
    return out


class HandleModel:
    def __init__(self, T, tol=None):
        self.tol = dict(tol or {})
        self.o = F64Tableau(T, self.tol)
        self.m, self.n = self.o.m, self.o.n

    @property
    def T(self):
        return self.o.T

    def upload(self, T):
        assert np.shape(T) == (self.m + 1, self.n + 1)
        self.o = F64Tableau(T, self.tol)

    def set_tol(self, tol):
        """the whole lp_tol: the defaults with `tol`'s fields"""
        self.tol = dict(tol or {})
        self.o.tol = _tol(self.tol)

    # -- pivots
    def run(self, rule, k):
        """-> (status, pivots done, log)"""
        st, log = self.o.run(rule, k)
        return st, len(log), log.tolist()

    def solve(self, cap):
        """-> (status, npiv, nstd, log)"""
        st, log, nstd = self.o.solve(cap=cap, logcap=max(cap, 1) if cap >= 0 else 1 << 16)
        return st, len(log), nstd, log.tolist()

    def find(self, rule, do_pivot):
        w = self.o.find(rule)
        if do_pivot and not isinstance(w, str):
            self.o.pivot(*w)
        return w

    def pivot(self, r, c):
        return self.o.pivot(r, c)

    def pivot_checked(self, r, c):
        """Simplex.pivot: taken iff (r, c) is one of findPivotAll's pairs"""
        if (r, c) in self.o.find_all():
            return self.o.pivot(r, c)
        return ZERO_PIVOT if self.T[1 + r, 1 + c] == 0.0 else BAD_PIVOT

    # -- scans
    def find_all(self):
        return self.o.find_all()

    def find_max_increase(self, do_pivot):
        w = self.o.find_max_increase()
        if do_pivot and not isinstance(w, str):
            self.o.pivot(*w)
        return w

    def form_checks(self):
        return host_checks(self.T)

    # -- data
    def put_rows(self, row0, rows, rb=0, rc=None):
        rows = np.asarray(rows, dtype=np.float64)
        st = window_status(self.m, self.n, row0, rows.shape[0], rows.shape[1], rb, rc)
        if st == PIVOTED:
            self.T[row0:row0 + rows.shape[0]] = rows[:, :self.n + 1]
        return st

    def rows(self, row0, nrows, rb=0, rc=None):
        st = window_status(self.m, self.n, row0, nrows, self.n + 1, rb, rc)
        return st if st != PIVOTED else self.T[row0:row0 + nrows].copy()

    def objective(self):
        return self.o.objective()

    def finished(self):
        """optimal, or unbounded under one of the two rules: nothing left to pivot on"""
        return isinstance(self.o.find(0), str) or isinstance(self.o.find(1), str)


# ---------------------------------------------------------------------------
# call sequences
# ---------------------------------------------------------------------------

def _deck(rng):
    d = [("run", int(rng.integers(0, 2)), k) for k in RUN_K]
    d += [("solve", cap) for cap in SOLVE_CAPS]
    d += [("find", rule, dp) for rule in (0, 1) for dp in (False, True)]
    d += [(k,) for k in ("pivot", "pivot_zero", "checked_ok", "checked_bad", "find_all", "form_checks",
                         "rows", "set_tol", "objective") + PUTS for _ in range(2)]
    d += [("find_max_increase", dp) for dp in (False, True)]
    d += [("set_block", b) for b in BLOCKS]
    return [d[i] for i in rng.permutation(len(d))]


@functools.lru_cache(maxsize=None)
def sequence(kind, m, ns, seed, tol_name):
    """-> list of ops: dict(kind, args, ret, T, log, skipped).

    ret is what the call must return, T the tableau it must leave (None: the
    call cannot change it), log the pivot log (run / solve only).  The deck
    holds every call of the alphabet (each k of run, each cap of solve, both
    rules and do_pivot of find, each block depth, ...) in a seeded order.
    Added to it: a scan after the first upload of row 0 alone, lp_run(rule, 0)
    after the first upload of one constraint row, and -- whenever the model
    says the LP is finished -- a whole upload of a fresh seed followed by
    lp_run(rule, 0).  A solve without a cap waits for the default lp_tol (the
    stand-ins of cc.TOL_SETS can cycle).  skipped is set where the state offers
    no cell for the call (no zero cell, no refusable pivot): the CPU test
    asserts that no sequence in use has one."""
    rng = np.random.default_rng(seed)
    tol_set = dict(cc.TOL_SETS)[tol_name]
    fresh = [0]

    def fresh_T():
        fresh[0] += 1
        return gen.tableau(kind, m, ns, 1000 * seed + fresh[0])

    M = HandleModel(gen.tableau(kind, m, ns, seed))
    mm, n = M.m, M.n
    ops = [dict(kind="upload", args=(M.T.copy(),), ret=PIVOTED, T=M.T.copy())]
    deck = _deck(rng)
    extra_scan = extra_run0 = True
    tol_on = False
    pos = 0

    def emit(kind_, args, ret, changed, log=None, skipped=False):
        ops.append(dict(kind=kind_, args=args, ret=ret, T=M.T.copy() if changed else None, log=log,
                        skipped=skipped))

    def do(op):
        nonlocal tol_on
        k = op[0]
        if k == "run":
            st, done, log = M.run(op[1], op[2])
            emit(k, op[1:], (st, done), True, log)
        elif k == "solve":
            st, npiv, nstd, log = M.solve(op[1])
            emit(k, op[1:], (st, npiv, nstd), True, log)
        elif k == "find":
            emit(k, op[1:], M.find(op[1], op[2]), True)
        elif k == "pivot":
            r, c = M.o.find(int(rng.integers(0, 2)))
            emit(k, (r, c), M.pivot(r, c), True)
        elif k == "pivot_zero":
            zr, zc = np.nonzero(M.T[1:, 1:] == 0.0)
            if len(zr) == 0:
                return emit(k, (), None, False, skipped=True)
            i = int(rng.integers(0, len(zr)))
            emit(k, (int(zr[i]), int(zc[i])), M.pivot(int(zr[i]), int(zc[i])), True)
        elif k == "checked_ok":
            S = M.find_all()
            if not S:
                return emit(k, (), None, False, skipped=True)
            r, c = S[int(rng.integers(0, len(S)))]
            emit(k, (r, c), M.pivot_checked(r, c), True)
        elif k == "checked_bad":
            # an eligible row of a column with a minimum that is outside its band
            S = set(M.find_all())
            piv = dict(DEFAULT_TOL, **M.tol)["pivot"]
            cand = [(i, c) for c in sorted({c for _, c in S}) for i in range(mm)
                    if M.T[1 + i, 1 + c] > piv and (i, c) not in S]
            if not cand:
                return emit(k, (), None, False, skipped=True)
            r, c = cand[int(rng.integers(0, len(cand)))]
            emit(k, (r, c), M.pivot_checked(r, c), True)
        elif k == "find_all":
            emit(k, (), M.find_all(), False)
        elif k == "find_max_increase":
            emit(k, op[1:], M.find_max_increase(op[1]), True)
        elif k == "form_checks":
            emit(k, (), M.form_checks(), False)
        elif k in PUTS:
            F = fresh_T()
            if k == "put_row0":
                r0, w = 0, 1
            elif k == "put_one":
                r0, w = int(rng.integers(1, mm)), 1
            elif k == "put_last":
                r0, w = mm, 1
            else:
                w = int(rng.integers(2, 6))
                r0 = int(rng.integers(0, mm + 2 - w))
            rows = F[r0:r0 + w].copy()
            emit(k, (r0, rows), M.put_rows(r0, rows), True)
        elif k == "rows":
            w = int(rng.integers(1, 6))
            r0 = int(rng.integers(0, mm + 2 - w))
            emit(k, (r0, w), M.rows(r0, w), False)
        elif k == "set_tol":
            tol_on = not tol_on
            M.set_tol(tol_set if tol_on else None)
            emit(k, (dict(DEFAULT_TOL, **M.tol),), None, False)
        elif k == "set_block":
            emit(k, op[1:], None, False)
        elif k == "objective":
            emit(k, (), M.objective(), False)
        else:
            raise KeyError(k)

    while pos < len(deck):
        op = deck[pos]
        pos += 1
        if op == ("solve", -1) and tol_on:
            deck.append(op)                 # after the set_tol that restores the defaults
            continue
        do(op)
        if op[0] == "put_row0" and extra_scan:
            extra_scan = False
            s = SCANS[int(rng.integers(0, 3))]
            do((s, False) if s == "find_max_increase" else (s,))
        elif op[0] == "put_one" and extra_run0:
            extra_run0 = False
            do(("run", int(rng.integers(0, 2)), 0))
        if M.finished():
            T = fresh_T()
            M.upload(T)
            ops.append(dict(kind="upload", args=(T,), ret=PIVOTED, T=M.T.copy()))
            do(("run", int(rng.integers(0, 2)), 0))
            do(("find", int(rng.integers(0, 2)), False))
    return ops


# (kind, m, ns, seed, the cc.TOL_SETS entry set_tol switches to): the sequences
# test_gpu_handle_state.py replays, each condition on them asserted by
# test_handle_model_cpu.py
SMALL = ("mixed", 40, 30, 1, "pivot")
MID = ("mixed", 300, 191, 2, "cost_tie")
TALL = ("tall", 6000, 40, 3, "cost")
GROUP = ("mixed", 130, 70, 4, "ratio_tie")
SEQUENCES = (SMALL, MID, TALL, GROUP)
K_GROUP_OPS = 24        # the k_group leg: this prefix of TALL's sequence, see k_group_ops()


def k_group_ops():
    """the k_group leg's calls: a prefix of TALL's sequence without its
    lp_set_block calls (no result depends on them), so that every run takes the
    automatic depth -- the one at which the XCD shards would run if they were on"""
    return [o for o in sequence(*TALL)[:K_GROUP_OPS] if o["kind"] != "set_block"]


def seq_id(spec):
    return "{}_{}x{}_s{}_{}".format(*spec)


# ---------------------------------------------------------------------------
# replay on an engine
# ---------------------------------------------------------------------------

def group_state(grp):
    """the whole tableau: the single engine's, or row 0 and every member's rows"""
    if len(grp) == 1:
        return grp[0].download()
    return np.concatenate([grp[0].rows(0, 1)] + [g.rows(1 + g.row_begin, g.row_count) for g in grp])


def group_put(grp, row0, rows):
    """a window of global rows: row 0 to every member, each constraint row to
    the member that holds it (one lp_upload_rows per member and run of rows)"""
    for g in grp:
        lo, hi = max(row0, 1 + g.row_begin), min(row0 + len(rows), 1 + g.row_begin + g.row_count)
        if row0 == 0:
            g.put_rows(0, rows[:1])
        if lo < hi:
            g.put_rows(lo, rows[lo - row0:hi - row0])


def group_rows(grp, row0, nrows):
    out = np.empty((nrows, grp[0].n + 1))
    for k in range(nrows):
        R = row0 + k
        g = grp[0] if R == 0 else next(x for x in grp if 1 + x.row_begin <= R < 1 + x.row_begin + x.row_count)
        out[k] = g.rows(R, 1)[0]
    return out


def _norm(x):
    return list(x) if isinstance(x, tuple) else x


def _took(e):
    geo = e.geometry()
    return dict(block=e.get_block(), path=e.exchange_path()[0], kernel=geo["kernel"], xcd_shards=geo["xcd_shards"],
                xcd_shards_engaged=geo["xcd_shards_engaged"])


def _assert_state(grp, T, where):
    assert bits(group_state(grp), T), where
    for g in grp[1:]:                      # row 0 is replicated on every member
        assert bits(g.rows(0, 1), T[:1]), (where, "row 0 of the member at", g.row_begin)


def replay(ops, grp, every=1):
    """drive grp (one engine, or the members of an in-process shard group)
    through ops; after every call compare what it returned, after every
    `every`-th call that can change the tableau (and after the last) the whole
    tableau, bit for bit.  -> the path taken by every lp_run / lp_solve that
    enqueued pivots: [dict(block, path, kernel, xcd_shards, xcd_shards_engaged)]
    (the selection kernel depends on the pivots per sweep in force)."""
    e = grp[0]
    changing = 0
    last = None
    took = []
    for i, op in enumerate(ops):
        k, a = op["kind"], op["args"]
        where = f"op {i}: {k} {'' if k == 'upload' else a[:1] if k in PUTS else a}"
        assert not op.get("skipped"), where
        if k == "upload":
            for g in grp:
                g.upload(a[0])
        elif k == "run":
            got = e.run(*a)
            assert got == op["ret"], (where, got)
            assert e.log().tolist() == op["log"], where
            if op["ret"][1] > 0:
                took.append(_took(e))
        elif k == "solve":
            got = e.solve(a[0])
            assert got == op["ret"], (where, got)
            assert e.log().tolist() == op["log"], where
            if op["ret"][1] > 0:
                took.append(_took(e))
        elif k == "find":
            assert _norm(e.find(*a)) == _norm(op["ret"]), where
        elif k in ("pivot", "pivot_zero"):
            assert e.pivot(*a) == op["ret"], where
        elif k in ("checked_ok", "checked_bad"):
            assert e.pivot_checked(*a) == op["ret"], where
        elif k == "find_all":
            assert e.find_all() == op["ret"], where
        elif k == "find_max_increase":
            assert _norm(e.find_max_increase(*a)) == _norm(op["ret"]), where
        elif k == "form_checks":
            assert e.form_checks() == op["ret"], where
        elif k in PUTS:
            group_put(grp, a[0], a[1])
        elif k == "rows":
            assert bits(group_rows(grp, *a), op["ret"]), where
        elif k == "set_tol":
            e.set_tol(**a[0])
        elif k == "set_block":
            e.set_block(a[0])
        elif k == "objective":
            z = e.objective()
            assert bits([z], [op["ret"]]), where
        else:
            raise KeyError(k)
        if op["T"] is not None:
            changing += 1
            last = None if changing % every == 0 else (op["T"], where)
            if last is None:
                _assert_state(grp, op["T"], where)
    if last is not None:
        _assert_state(grp, *last)
    assert e.exchange_path()[1] == 0
    return took
