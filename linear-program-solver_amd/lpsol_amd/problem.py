"""Problem-form batches: LPs given as ``min c.x, A x {<=, >=, ==} b, x >= 0``.

The caller keeps c, A, b and one sense per row; the slack and surplus columns
of the simplex tableau are laid out on the device (lp_problem_upload,
csrc/batch.hip k_assemble), so the upload carries only the first ns + 1
columns of each tableau, and the dual values are read back from row 0 of the
final tableaux without downloading them (lp_problem_duals, k_duals).

The *problem block* of an LP with m rows and ns structural variables is the
``(m+1, ns+1)`` float64 array P of its tableau's first ns + 1 columns:
``P[0, 0]`` the stored ``_z`` cell, ``P[0, 1+j] = c_j``, ``P[1+i, 0] = b_i``,
``P[1+i, 1+j] = a_ij``.  ``assemble_tableaux`` and ``problem_duals`` are the
host statements of what the two kernels compute; ``solve_problems`` and
``solve_problems_ragged`` need a GPU (there is no host fallback).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .tableau import Tableau

QUIET_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def problem_columns(sense, ns: int) -> int:
    """n = ns + k, k the senses that are not "==" (lp_problem_columns)"""
    s = _lib.sense_codes(sense)
    if len(s) < 1 or int(ns) < 1:
        raise ValueError("an LP needs m >= 1 senses and ns >= 1 structural variables")
    return int(ns) + int(np.count_nonzero(s != _lib.SENSE_EQ))


def _slack_columns(s: np.ndarray, ns: int):
    """-> (rows that are not "==", the variable column ns + t each owns, +1.0 / -1.0)"""
    rows = np.nonzero(s != _lib.SENSE_EQ)[0]
    return rows, ns + np.arange(len(rows)), np.where(s[rows] == _lib.SENSE_LE, 1.0, -1.0)


def _assemble_one(P: np.ndarray, s: np.ndarray) -> np.ndarray:
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim != 2 or P.shape[0] < 2 or P.shape[1] < 2:
        raise ValueError("a problem block must be (m+1, ns+1) with m, ns >= 1")
    if len(s) != P.shape[0] - 1:
        raise ValueError(f"sense must hold {P.shape[0] - 1} entries, one per row, not {len(s)}")
    ns = P.shape[1] - 1
    rows, cols, ones = _slack_columns(s, ns)
    T = np.zeros((P.shape[0], 1 + ns + len(rows)), dtype=np.float64)
    T.view(np.uint64)[:, :ns + 1] = P.view(np.uint64)      # the 64 bits: NaN payloads survive
    T[1 + rows, 1 + cols] = ones
    return T


def assemble_tableaux(P, sense):
    """The host formula of k_assemble.  P ``[B, m+1, ns+1]`` with one sense
    vector shared by every LP -> ``[B, m+1, n+1]``; or a list of blocks with a
    list of per-LP senses -> a list of tableaux.  Columns 0..ns are P's bits;
    the t-th row that is not "==" owns column ns + t, +1.0 for "<=" and -1.0
    for ">="; every other cell is +0.0."""
    if isinstance(P, np.ndarray) and P.ndim == 3:
        s = _lib.sense_codes(sense)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if P.shape[0] < 1 or P.shape[1] < 2 or P.shape[2] < 2:
            raise ValueError("problem blocks must be [B, m+1, ns+1] with B, m, ns >= 1")
        if len(s) != P.shape[1] - 1:
            raise ValueError(f"sense must hold {P.shape[1] - 1} entries, one per row, not {len(s)}")
        ns = P.shape[2] - 1
        rows, cols, ones = _slack_columns(s, ns)
        T = np.zeros((P.shape[0], P.shape[1], 1 + ns + len(rows)), dtype=np.float64)
        T.view(np.uint64)[:, :, :ns + 1] = P.view(np.uint64)
        T[:, 1 + rows, 1 + cols] = ones
        return T
    items = list(P)
    senses = list(sense)
    if len(items) != len(senses):
        raise ValueError("sense must hold one sequence per LP")
    return [_assemble_one(p, _lib.sense_codes(s)) for p, s in zip(items, senses)]


def problem_duals(T, sense, ns: int) -> np.ndarray:
    """The host formula of k_duals on one LP's stored tableau: y[r] =
    -T[0, 1+j] on a "<=" row that owns column j (a flip of the sign bit),
    T[0, 1+j] on a ">=" row, the quiet NaN on an "==" row.  Only row 0 of T is
    read, so the rows phase 1 dropped do not matter."""
    s = _lib.sense_codes(sense)
    row0 = np.asarray(T, dtype=np.float64)[0]
    rows, cols, ones = _slack_columns(s, int(ns))
    if 1 + int(ns) + len(rows) != len(row0):
        raise ValueError(f"the tableau has {len(row0) - 1} columns, the senses and ns give {int(ns) + len(rows)}")
    y = np.full(len(s), QUIET_NAN, dtype=np.float64)
    c = row0[1 + cols]
    y[rows] = np.where(ones > 0, -c, c)
    return y


def pack_problems(c, A, b, z0=None) -> np.ndarray:
    """c ``[B, ns]``, A ``[B, m, ns]``, b ``[B, m]`` (and the stored ``_z``
    cells z0 ``[B]``, default +0.0) -> problem blocks ``[B, m+1, ns+1]``"""
    c = np.asarray(c, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if A.ndim != 3 or A.shape[0] < 1 or A.shape[1] < 1 or A.shape[2] < 1:
        raise ValueError("A must be [B, m, ns] with B, m, ns >= 1")
    B, m, ns = A.shape
    if c.shape != (B, ns):
        raise ValueError(f"c must be ({B}, {ns}), not {c.shape}")
    if b.shape != (B, m):
        raise ValueError(f"b must be ({B}, {m}), not {b.shape}")
    P = np.zeros((B, m + 1, ns + 1), dtype=np.float64)
    if z0 is not None:
        z0 = np.asarray(z0, dtype=np.float64)
        if z0.shape != (B,):
            raise ValueError(f"z0 must be ({B},), not {z0.shape}")
        P[:, 0, 0] = z0
    P[:, 0, 1:] = c
    P[:, 1:, 0] = b
    P[:, 1:, 1:] = A
    return P


def _pack_one(c, A, b) -> np.ndarray:
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError("A of an LP must be [m, ns]")
    return pack_problems(np.asarray(c, dtype=np.float64)[None], A[None], np.asarray(b, dtype=np.float64)[None])[0]


class ProblemResult:
    """What solve_problems returns: per-LP arrays and the live engine.  x is
    ``[B, ns]`` (the structural variables), slack ``[B, m]`` the value of each
    row's slack or surplus variable (+0.0 on "==" rows), y ``[B, m]`` the dual
    values, fetched from the device on first use.  path is "plain" (every
    sense "<=" and every LP canonical: Simplex.solve alone) or "twophase".  On
    the plain path stage / rows / ninit are zeros / m / zeros."""

    def __init__(self, engine, path, sense, ns, status, stage, rows, ninit, npiv, nstd, objective, basis, xall):
        self._engine = engine
        self._y = None
        self.path = path
        self.sense, self.ns = sense, ns
        self.status_code = status
        self.status = [_lib.STATUS_NAMES.get(int(s), str(int(s))) for s in status]
        self.stage, self.rows, self.ninit = stage, rows, ninit
        self.npiv, self.nstd = npiv, nstd
        self.objective = objective
        self.basis = basis
        self.x, self.slack = self._split(xall)

    def _split(self, xall):
        rows, cols, _ = _slack_columns(self.sense, self.ns)
        slack = np.zeros((xall.shape[0], len(self.sense)), dtype=np.float64)
        slack[:, rows] = xall[:, cols]
        return np.ascontiguousarray(xall[:, :self.ns]), slack

    def __len__(self) -> int:
        return len(self.status)

    @property
    def y(self):
        if self._y is None:
            self._y = self._engine.duals()
        return self._y

    def _nlog(self, i: int) -> int:
        return int(self.ninit[i])

    def init_log(self, i: int) -> np.ndarray:
        """phase-1 (r, c) pairs of LP i (none on the plain path)"""
        return self._engine.log(i)[:self._nlog(i)]

    def log(self, i: int) -> np.ndarray:
        """phase-2 (r, c) pairs of LP i, oldest first (at most log_cap of them)"""
        return self._engine.log(i)[self._nlog(i):]

    def tableau(self, i: int) -> Tableau:
        """LP i's final tableau, downloaded alone from the live engine"""
        return Tableau.fromArray(self._engine.download(first=int(i), count=1)[0][:int(self.rows[i]) + 1])


class ProblemRaggedResult(ProblemResult):
    """What solve_problems_ragged returns: ProblemResult with sense, ns as
    per-LP lists and x, slack, y, basis as lists of per-LP arrays."""

    def _split(self, xall):
        xs, slacks = [], []
        for x, s, ns in zip(xall, self.sense, self.ns):
            rows, cols, _ = _slack_columns(s, ns)
            slack = np.zeros(len(s), dtype=np.float64)
            slack[rows] = x[cols]
            xs.append(np.ascontiguousarray(x[:ns]))
            slacks.append(slack)
        return xs, slacks


def _run(eng, all_le, placed, max_pivots):
    """steps 3 to 5 of solve_problems on an engine that holds the tableaux"""
    cap = -1 if max_pivots is None else int(max_pivots)
    if all_le and eng.derive_basis()[1] < 0:
        status, npiv, nstd = eng.solve(cap)
        stage = np.zeros(eng.count, dtype=np.int32)
        rows = np.array([eng.m] * eng.count if not hasattr(eng, "shapes") else [s[0] for s in eng.shapes],
                        dtype=np.int64)
        return "plain", status, stage, rows, np.zeros(eng.count, dtype=np.int64), npiv, nstd
    solve = eng.solve_lp_placed if placed else eng.solve_lp
    return ("twophase", *solve(cap))


def solve_problems(c, A, b, sense=None, *, max_pivots=None, tol=None, log_cap=0, device=0,
                   place="lds") -> ProblemResult:
    """min c.x subject to A x {<=, >=, ==} b, x >= 0 for B LPs of one shape: c
    ``[B, ns]``, A ``[B, m, ns]``, b ``[B, m]``, sense m entries shared by
    every LP ("<=", ">=", "==" or _lib.SENSE_*; None: all "<=").  The tableaux
    are assembled on the device; if every sense is "<=" and every LP is
    canonical (all b_i >= 0) Simplex.solve runs alone, else phase 1 runs first
    (lp_twophase_solve, or lp_phased_solve when place is not "lds"); x, the
    objective and, on first use, the duals are gathered on the device, and no
    tableau is downloaded.  Argument errors are ValueError before any device
    call."""
    P = pack_problems(c, A, b)
    B, m, ns = P.shape[0], P.shape[1] - 1, P.shape[2] - 1
    s = _lib.sense_codes(["<="] * m if sense is None else sense)
    if len(s) != m:
        raise ValueError(f"sense must hold {m} entries, one per row, not {len(s)}")
    placed = _lib.place_code(place) != _lib.PLACE_LDS
    eng = _lib.BatchEngine(B, m, problem_columns(s, ns), log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.set_senses(s)
    eng.upload_problems(P)
    path, status, stage, rows, ninit, npiv, nstd = _run(eng, bool((s == _lib.SENSE_LE).all()), placed, max_pivots)
    x, z = eng.solution()
    return ProblemResult(eng, path, s, ns, status, stage, rows, ninit, npiv, nstd, z, eng.get_basis(), x)


def solve_problems_ragged(problems, *, max_pivots=None, tol=None, log_cap=0, device=0,
                          place="lds") -> ProblemRaggedResult:
    """solve_problems for LPs of any shapes: problems is a sequence of
    (c, A, b, sense), c ``[ns_i]``, A ``[m_i, ns_i]``, b ``[m_i]`` and sense
    m_i entries or None (all "<=").  The plain path is taken when every sense
    of every LP is "<=" and every LP is canonical."""
    items = list(problems)
    if not items:
        raise ValueError("empty batch")
    blocks, senses = [], []
    for i, item in enumerate(items):
        if len(item) != 4:
            raise ValueError(f"LP {i} must be (c, A, b, sense)")
        ci, Ai, bi, si = item
        try:
            blocks.append(_pack_one(ci, Ai, bi))
        except ValueError as e:
            raise ValueError(f"LP {i}: {e}") from None
        m = blocks[-1].shape[0] - 1
        s = _lib.sense_codes(["<="] * m if si is None else si)
        if len(s) != m:
            raise ValueError(f"LP {i}: sense must hold {m} entries, one per row, not {len(s)}")
        senses.append(s)
    nss = [p.shape[1] - 1 for p in blocks]
    shapes = [(p.shape[0] - 1, problem_columns(s, ns)) for p, s, ns in zip(blocks, senses, nss)]
    placed = _lib.place_code(place) != _lib.PLACE_LDS
    eng = _lib.RaggedEngine(shapes, log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.set_senses(senses)
    eng.upload_problems(blocks)
    all_le = all(bool((s == _lib.SENSE_LE).all()) for s in senses)
    path, status, stage, rows, ninit, npiv, nstd = _run(eng, all_le, placed, max_pivots)
    x, z = eng.solution()
    return ProblemRaggedResult(eng, path, senses, nss, status, stage, rows, ninit, npiv, nstd, z, eng.get_basis(), x)
