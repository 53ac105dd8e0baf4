"""Batched solve: many small LPs in one call.

``solve_batch`` runs Simplex.solve (simplex.py:110-148) on every LP of a
``[B, m+1, n+1]`` stack of engine-layout tableaux, one GPU workgroup per LP
with the LP's tableau in LDS (csrc/batch.hip).  Each LP gets exactly the
operations a single ``Simplex(t).solve()`` gives it.  All LPs share one shape
and one device.  ``solve_batch`` starts from a basic feasible tableau;
``solve_lp_batch`` runs phase 1 (Simplex._find_bfs, simplex.py:36-108) on the
device first, so its LPs may have negative b_i, ``>=`` and ``==`` rows.
``solve_ragged`` and ``solve_lp_ragged`` are the two for LPs of different
shapes (lp_ragged_*): one call, every LP solved as a batch of its own shape
would solve it.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .tableau import Tableau


def _canonical(T: np.ndarray):
    """-> (basis int32 [B, m], bad bool [B]) of canonical_basis"""
    B, m = T.shape[0], T.shape[1] - 1
    A = T[:, 1:, 1:]
    ones = A == 1.0
    unit = (T[:, 0, 1:] == 0.0) & (np.count_nonzero(A, axis=1) == 1) & ones.any(axis=1)   # [B, n]
    row = np.argmax(ones, axis=1)                                                        # [B, n]
    basis = np.full((B, m), -1, dtype=np.int32)
    # lowest column wins a row (isCanonical keeps the first it meets): write columns in descending order
    for j in range(T.shape[2] - 2, -1, -1):
        lp = np.nonzero(unit[:, j])[0]
        basis[lp, row[lp, j]] = j
    return basis, np.any(T[:, 1:, 0] < 0.0, axis=1) | np.any(basis < 0, axis=1)


def canonical_basis(T: np.ndarray) -> np.ndarray:
    """Tableau.isCanonical's basic column per row for every LP of a
    [B, m+1, n+1] stack -> int32 [B, m].  ValueError names the first LP that
    is not canonical (some b_i < 0, or a row without a unit column whose cost
    is zero)."""
    basis, bad = _canonical(T)
    if bad.any():
        raise ValueError(f"LP {int(np.argmax(bad))} of the batch is not canonical "
                         "(phase 1 is not part of the batch path: use solve_lp_batch)")
    return basis


RESULTS = ("full", "solution")


def _check_result(result) -> bool:
    """-> result == "solution"; ValueError for an unknown one, before any device call"""
    if result not in RESULTS:
        raise ValueError(f"result must be one of {RESULTS}, not {result!r}")
    return result == "solution"


def solution_x(T: np.ndarray, basis: np.ndarray) -> np.ndarray:
    """Simplex.getBFS (simplex.py:166-173) of one LP on the host: n entries
    +0.0, then x[basis[r]] = T[1+r][0] for r in row order (a later row
    overwrites an earlier one with the same column); an entry of the basis
    outside [0, n) is skipped.  The rows of T past len(basis) are not read."""
    x = np.zeros(T.shape[1] - 1, dtype=np.float64)
    for r, c in enumerate(np.asarray(basis).tolist()):
        if 0 <= c < len(x):
            x[c] = T[1 + r, 0]
    return x


def _stack_x(T: np.ndarray, basis: np.ndarray) -> np.ndarray:
    """solution_x for every LP of a [B, m+1, n+1] stack with its [B, m] basis -> [B, n]"""
    B, n = T.shape[0], T.shape[2] - 1
    x = np.zeros((B, n), dtype=np.float64)
    for r in range(basis.shape[1]):         # row order: the later row wins
        c = basis[:, r]
        lp = np.nonzero((c >= 0) & (c < n))[0]
        x[lp, c[lp]] = T[lp, 1 + r, 0]
    return x


def _stack(tableaux) -> np.ndarray:
    if isinstance(tableaux, np.ndarray):
        T = tableaux
    else:
        items = [t.toArray() if isinstance(t, Tableau) else np.asarray(t, dtype=np.float64)
                 for t in tableaux]
        if not items:
            raise ValueError("empty batch")
        if any(a.ndim != 2 or a.shape != items[0].shape for a in items):
            raise ValueError("every LP of a batch must have the same shape (m+1, n+1); "
                             "solve_ragged / solve_lp_ragged take LPs of different shapes")
        T = np.stack(items)
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.ndim != 3 or T.shape[0] < 1 or T.shape[1] < 2 or T.shape[2] < 2:
        raise ValueError("tableaux must be [B, m+1, n+1] with B, m, n >= 1")
    return T


class BatchResult:
    """What solve_batch returns: per-LP arrays plus the engine (for the logs).
    x is Simplex.getBFS per LP, [B, n].  Under result="solution" it was
    gathered on the device and tableaux is None: tableau(i) then downloads LP i
    alone from the live engine."""

    def __init__(self, engine, status, npiv, nstd, objective, tableaux, basis, x=None):
        self._engine = engine
        self._x = x
        self.status_code = status
        self.status = [_lib.STATUS_NAMES.get(int(s), str(int(s))) for s in status]
        self.npiv, self.nstd = npiv, nstd
        self.objective = objective
        self.tableaux = tableaux
        self.basis = basis

    def __len__(self) -> int:
        return len(self.status)

    def log(self, i: int) -> np.ndarray:
        """(r, c) pairs of LP i, oldest first (at most log_cap of them)"""
        return self._engine.log(i)

    @property
    def x(self):
        if self._x is None:     # result="full": the same formula on the host
            self._x = _stack_x(self.tableaux, self.basis)
        return self._x

    def _stored(self, i: int) -> np.ndarray:
        """LP i's final tableau as the engine keeps it, all m + 1 rows"""
        if self.tableaux is None:
            return self._engine.download(first=int(i), count=1)[0]
        return self.tableaux[i]

    def tableau(self, i: int) -> Tableau:
        return Tableau.fromArray(self._stored(i))


def solve_batch(tableaux, *, basis=None, max_pivots=None, tol=None, log_cap=0, device=0,
                rule=None, steps=None, place="lds", team=1, result="full") -> BatchResult:
    """Simplex.solve on every LP of the batch (or, with rule and steps, `steps`
    pivots of one fixed rule per LP).  tableaux: float64 [B, m+1, n+1] in
    engine layout, or a sequence of Tableau objects of one shape.  Every LP
    must be canonical already (ValueError otherwise); solve_lp_batch takes the
    others.  place: "lds" refuses a shape above one CU's LDS, "auto" solves
    such a shape with its tableau in device memory, "device" does so for
    every shape; the results are the same bits.  team: workgroups per
    device-placed LP, 1, a forced G or "auto" (several per LP where the batch
    is too small to fill the chip; lp_teamed_create); again the same bits.
    result: "full" downloads every final tableau; "solution" derives the
    starting basis on the device (unless `basis` is given), downloads no
    tableau and gathers x and the objective on the device instead
    (lp_solution_canonical, lp_solution_gather): the same bits, tableaux=None.
    rule: _lib.RULE_STANDARD, RULE_MIN_INDEX or RULE_MAX_INCREASE
    (findPivotMaxIncrease, simplex.py:286-328; not with a team above 1:
    ValueError).  With a large `steps`, RULE_MAX_INCREASE is a solve to
    optimality under that rule: status is "optimal" / "unbounded", "pivoted"
    when the cap was hit, or "bad_pivot" where the increases are so large that
    no column lies in the tie band; nstd is zeros, as for min-index."""
    slim = _check_result(result)
    T = _stack(tableaux)
    B, m, n = T.shape[0], T.shape[1] - 1, T.shape[2] - 1
    if (rule is None) != (steps is None):
        raise ValueError("rule and steps go together (the fixed-rule run)")
    if basis is None:
        basis = None if slim else canonical_basis(T)
    else:
        basis = np.ascontiguousarray(basis, dtype=np.int32)
        if basis.shape != (B, m):
            raise ValueError(f"basis must be ({B}, {m})")
    eng = _lib.BatchEngine(B, m, n, log_cap=log_cap, device=device, place=place, team=team)
    if tol:
        eng.set_tol(**tol)
    eng.upload(T)
    if basis is None:       # result="solution": canonical_basis on the device
        _, bad = eng.derive_basis()
        if bad >= 0:
            raise ValueError(f"LP {bad} of the batch is not canonical "
                             "(phase 1 is not part of the batch path: use solve_lp_batch)")
    else:
        eng.set_basis(basis)
    if rule is not None:
        status, npiv = eng.run(int(rule), int(steps))
        nstd = npiv.copy() if int(rule) == _lib.RULE_STANDARD else np.zeros_like(npiv)
    else:
        status, npiv, nstd = eng.solve(-1 if max_pivots is None else int(max_pivots))
    if slim:
        x, z = eng.solution()
        return BatchResult(eng, status, npiv, nstd, z, None, eng.get_basis(), x=x)
    out = eng.download()
    return BatchResult(eng, status, npiv, nstd, -out[:, 0, 0], out, eng.get_basis())


class LPBatchResult(BatchResult):
    """What solve_lp_batch returns: BatchResult plus, per LP, the stage it
    ended in (_lib.STAGE_*), the rows phase 1 left (m minus the dropped ones)
    and the number of phase-1 pivots.  npiv / nstd count phase 2 only."""

    def __init__(self, engine, status, stage, rows, ninit, npiv, nstd, objective, tableaux, basis, x=None):
        super().__init__(engine, status, npiv, nstd, objective, tableaux, basis, x=x)
        self.stage, self.rows, self.ninit = stage, rows, ninit

    def init_log(self, i: int) -> np.ndarray:
        """phase-1 (r, c) pairs of LP i: the artificial solve, then the
        drive-out pivots; artificial columns are n, n + 1, ..."""
        return self._engine.log(i)[:int(self.ninit[i])]

    def log(self, i: int) -> np.ndarray:
        """phase-2 (r, c) pairs of LP i (rows index the compacted tableau)"""
        return self._engine.log(i)[int(self.ninit[i]):]

    def tableau(self, i: int) -> Tableau:
        return Tableau.fromArray(self._stored(i)[:int(self.rows[i]) + 1])


def solve_lp_batch(tableaux, *, max_pivots=None, tol=None, log_cap=0, device=0, place="lds",
                   result="full") -> LPBatchResult:
    """Simplex(t) followed by solve() on every LP of the batch: phase 1
    (simplex.py:36-108) and phase 2 (simplex.py:110-148) on the device, one
    workgroup per LP (lp_twophase_solve).  Same input forms as solve_batch; the
    LPs need not be canonical.  max_pivots caps each of the two solves.
    place: "lds" refuses a shape whose tableau, widened by its m artificial
    columns, is above one CU's LDS, "auto" solves such a shape with its
    working tableau in device memory (lp_phased_solve), "device" does so for
    every shape; the results are the same bits.  result as in solve_batch."""
    slim = _check_result(result)
    T = _stack(tableaux)
    B, m, n = T.shape[0], T.shape[1] - 1, T.shape[2] - 1
    placed = _lib.place_code(place) != _lib.PLACE_LDS
    eng = _lib.BatchEngine(B, m, n, log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.upload(T)
    solve = eng.solve_lp_placed if placed else eng.solve_lp
    status, stage, rows, ninit, npiv, nstd = solve(-1 if max_pivots is None else int(max_pivots))
    if slim:
        x, z = eng.solution()
        return LPBatchResult(eng, status, stage, rows, ninit, npiv, nstd, z, None, eng.get_basis(), x=x)
    out = eng.download()
    return LPBatchResult(eng, status, stage, rows, ninit, npiv, nstd, -out[:, 0, 0], out,
                         eng.get_basis())


# ---------------------------------------------------------------------------
# ragged batches: LPs of different shapes in one call (lp_ragged_*)
# ---------------------------------------------------------------------------

def _ragged_items(tableaux) -> list:
    items = [np.ascontiguousarray(t.toArray() if isinstance(t, Tableau) else t, dtype=np.float64)
             for t in tableaux]
    if not items:
        raise ValueError("empty batch")
    for i, a in enumerate(items):
        if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 2:
            raise ValueError(f"LP {i} must be a 2-D (m+1, n+1) tableau with m, n >= 1")
    return items


def ragged_canonical_basis(items) -> list:
    """canonical_basis for a list of tableaux of any shapes, one stack per
    shape group; ValueError names the first LP that is not canonical by its
    position in the list"""
    groups = {}
    for i, a in enumerate(items):
        groups.setdefault(a.shape, []).append(i)
    out, bad = [None] * len(items), []
    for idx in groups.values():
        got, wrong = _canonical(np.stack([items[i] for i in idx]))
        bad += [i for k, i in enumerate(idx) if wrong[k]]
        for k, i in enumerate(idx):
            out[i] = got[k]
    if bad:
        raise ValueError(f"LP {min(bad)} of the batch is not canonical "
                         "(phase 1 is not part of this path: use solve_lp_ragged)")
    return out


class RaggedResult:
    """What solve_ragged returns: per-LP arrays as in BatchResult; tableaux,
    basis and x are lists of per-LP arrays, in the caller's order."""

    def __init__(self, engine, status, npiv, nstd, objective, tableaux, basis, x=None):
        self._engine = engine
        self._x = x
        self.status_code = status
        self.status = [_lib.STATUS_NAMES.get(int(s), str(int(s))) for s in status]
        self.npiv, self.nstd = npiv, nstd
        self.objective = objective
        self.tableaux = tableaux
        self.basis = basis

    def __len__(self) -> int:
        return len(self.status)

    def log(self, i: int) -> np.ndarray:
        """(r, c) pairs of LP i, oldest first (at most log_cap of them)"""
        return self._engine.log(i)

    @property
    def x(self):
        if self._x is None:     # result="full": the same formula on the host
            self._x = [solution_x(t, b) for t, b in zip(self.tableaux, self.basis)]
        return self._x

    def _stored(self, i: int) -> np.ndarray:
        """LP i's final tableau as the engine keeps it, all m_i + 1 rows"""
        if self.tableaux is None:
            return self._engine.download(first=int(i), count=1)[0]
        return self.tableaux[i]

    def tableau(self, i: int) -> Tableau:
        return Tableau.fromArray(self._stored(i))

    def plan(self, twophase: bool = False) -> list:
        """the launch bins the call used (RaggedEngine.plan)"""
        return self._engine.plan(twophase)


def solve_ragged(tableaux, *, basis=None, max_pivots=None, tol=None, log_cap=0, device=0,
                 rule=None, steps=None, place="lds", team=1, result="full") -> RaggedResult:
    """solve_batch for LPs of any shapes: Simplex.solve on every LP (or, with
    rule and steps, `steps` pivots of one fixed rule per LP), each LP exactly
    as a batch of its own shape would solve it.  tableaux: a sequence of 2-D
    float64 arrays in engine layout or of Tableau objects; order is kept.
    Every LP must be canonical already (ValueError names the first that is
    not); solve_lp_ragged takes the others.  place as in solve_batch, LP by
    LP: under "auto" the LPs above one CU's LDS run from device memory, the
    others from LDS.  team as in solve_batch, or one request per LP.  result
    as in solve_batch; x is then a list of per-LP arrays.  rule as in
    solve_batch, RULE_MAX_INCREASE included."""
    slim = _check_result(result)
    items = _ragged_items(tableaux)
    if (rule is None) != (steps is None):
        raise ValueError("rule and steps go together (the fixed-rule run)")
    shapes = [(a.shape[0] - 1, a.shape[1] - 1) for a in items]
    if basis is None:
        basis = None if slim else ragged_canonical_basis(items)
    else:
        basis = [np.ascontiguousarray(b, dtype=np.int32) for b in basis]
        if len(basis) != len(items) or any(b.shape != (s[0],) for b, s in zip(basis, shapes)):
            raise ValueError("basis must hold one array of m_i entries per LP")
    eng = _lib.RaggedEngine(shapes, log_cap=log_cap, device=device, place=place, team=team)
    if tol:
        eng.set_tol(**tol)
    eng.upload(items)
    if basis is None:       # result="solution": ragged_canonical_basis on the device
        _, bad = eng.derive_basis()
        if bad >= 0:
            raise ValueError(f"LP {bad} of the batch is not canonical "
                             "(phase 1 is not part of this path: use solve_lp_ragged)")
    else:
        eng.set_basis(basis)
    if rule is not None:
        status, npiv = eng.run(int(rule), int(steps))
        nstd = npiv.copy() if int(rule) == _lib.RULE_STANDARD else np.zeros_like(npiv)
    else:
        status, npiv, nstd = eng.solve(-1 if max_pivots is None else int(max_pivots))
    if slim:
        x, z = eng.solution()
        return RaggedResult(eng, status, npiv, nstd, z, None, eng.get_basis(), x=x)
    out = eng.download()
    return RaggedResult(eng, status, npiv, nstd, np.array([-a[0, 0] for a in out]), out, eng.get_basis())


class LPRaggedResult(RaggedResult):
    """What solve_lp_ragged returns: RaggedResult plus stage, rows and ninit
    per LP, as in LPBatchResult.  npiv / nstd count phase 2 only."""

    def __init__(self, engine, status, stage, rows, ninit, npiv, nstd, objective, tableaux, basis, x=None):
        super().__init__(engine, status, npiv, nstd, objective, tableaux, basis, x=x)
        self.stage, self.rows, self.ninit = stage, rows, ninit

    def init_log(self, i: int) -> np.ndarray:
        """phase-1 (r, c) pairs of LP i; its artificial columns are n_i, n_i + 1, ..."""
        return self._engine.log(i)[:int(self.ninit[i])]

    def log(self, i: int) -> np.ndarray:
        """phase-2 (r, c) pairs of LP i (rows index the compacted tableau)"""
        return self._engine.log(i)[int(self.ninit[i]):]

    def tableau(self, i: int) -> Tableau:
        return Tableau.fromArray(self._stored(i)[:int(self.rows[i]) + 1])

    def plan(self, twophase: bool = True) -> list:
        return self._engine.plan(twophase)


def solve_lp_ragged(tableaux, *, max_pivots=None, tol=None, log_cap=0, device=0, place="lds",
                    result="full") -> LPRaggedResult:
    """solve_lp_batch for LPs of any shapes: phase 1 and phase 2 on the device
    for every LP (lp_twophase_solve on a ragged batch), each LP exactly as a
    batch of its own shape would solve it.  max_pivots caps each of the two
    solves.  place as in solve_lp_batch, LP by LP: under "auto" the LPs whose
    widened tableau is above one CU's LDS run from device memory, the others
    from LDS.  result as in solve_ragged."""
    slim = _check_result(result)
    items = _ragged_items(tableaux)
    shapes = [(a.shape[0] - 1, a.shape[1] - 1) for a in items]
    placed = _lib.place_code(place) != _lib.PLACE_LDS
    eng = _lib.RaggedEngine(shapes, log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.upload(items)
    solve = eng.solve_lp_placed if placed else eng.solve_lp
    status, stage, rows, ninit, npiv, nstd = solve(-1 if max_pivots is None else int(max_pivots))
    if slim:
        x, z = eng.solution()
        return LPRaggedResult(eng, status, stage, rows, ninit, npiv, nstd, z, None, eng.get_basis(), x=x)
    out = eng.download()
    return LPRaggedResult(eng, status, stage, rows, ninit, npiv, nstd, np.array([-a[0, 0] for a in out]),
                          out, eng.get_basis())
