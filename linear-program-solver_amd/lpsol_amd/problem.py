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

General form (lp_general_*): ``min`` or ``max`` of ``c0 + c.x``
with per-variable bounds ``lb <= x <= ub``.  Each variable has a *kind*
(``_lib.VAR_*``) derived from which of its bounds are finite; the device shifts,
splits and flips the LP into the standard form above and undoes it on x, the
objective, the duals and the reduced costs.  ``general_standard_form``,
``general_recover`` and ``general_duals`` are the host statements of that.
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


# ---------------------------------------------------------------------------
# general form: bounds, free variables, maximise
# ---------------------------------------------------------------------------
_SIGN = np.uint64(1 << 63)
_SHIFTED = (_lib.VAR_LOWER, _lib.VAR_BOXED, _lib.VAR_UPPER)


def _bounds(lb, ub, shape):
    """lb (None: 0) and ub (None: +inf) broadcast to `shape`, checked"""
    lo = np.zeros(shape) if lb is None else np.array(np.broadcast_to(np.asarray(lb, dtype=np.float64), shape))
    hi = np.full(shape, np.inf) if ub is None else np.array(np.broadcast_to(np.asarray(ub, dtype=np.float64), shape))
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("a bound is NaN")
    if (lo == np.inf).any():
        raise ValueError("a lower bound is +inf")
    if (hi == -np.inf).any():
        raise ValueError("an upper bound is -inf")
    return lo, hi


def general_kinds(lb, ub) -> np.ndarray:
    """The kind of each variable from which of its bounds are finite: lb and
    ub ``[ns]`` or ``[B, ns]`` -> int8 ``[ns]``.  VAR_PLAIN needs lb == 0 and
    ub == +inf (in every LP of a stack), VAR_LOWER a finite lb alone,
    VAR_BOXED both finite, VAR_UPPER a finite ub alone, VAR_FREE neither.  The
    LPs of a stack must agree on each variable's pattern (ValueError: use
    solve_problems_ragged); a NaN bound, lb = +inf or ub = -inf is a
    ValueError."""
    shape = np.broadcast_shapes(() if lb is None else np.shape(lb), () if ub is None else np.shape(ub))
    lo, hi = _bounds(lb, ub, shape)
    if lo.ndim not in (1, 2) or lo.shape[-1] < 1:
        raise ValueError("bounds must be [ns] or [B, ns] with ns >= 1")
    lo2, hi2 = np.atleast_2d(lo), np.atleast_2d(hi)
    flo, fhi = np.isfinite(lo2), np.isfinite(hi2)
    if (flo != flo[0]).any() or (fhi != fhi[0]).any():
        j = int(np.nonzero(((flo != flo[0]) | (fhi != fhi[0])).any(axis=0))[0][0])
        raise ValueError(f"the LPs of a uniform batch disagree on which bounds of variable {j} are finite: "
                         "use solve_problems_ragged, which takes a form per LP")
    kind = np.where(flo[0], np.where(fhi[0], _lib.VAR_BOXED, _lib.VAR_LOWER),
                    np.where(fhi[0], _lib.VAR_UPPER, _lib.VAR_FREE)).astype(np.int8)
    plain = (kind == _lib.VAR_LOWER) & (lo2 == 0.0).all(axis=0)
    kind[plain] = _lib.VAR_PLAIN
    return kind


def _general_counts(sense, kind):
    s, k = _lib.sense_codes(sense), _lib.kind_codes(kind)
    if len(s) < 1 or len(k) < 1:
        raise ValueError("an LP needs m >= 1 senses and ns >= 1 kinds")
    nf, nb = int(np.count_nonzero(k == _lib.VAR_FREE)), int(np.count_nonzero(k == _lib.VAR_BOXED))
    return s, k, nf, nb


def general_shape(sense, kind):
    """(m', n') of the standard form: m' = m + nb, n' = ns + nf + k + nb
    (lp_general_rows, lp_general_columns)"""
    s, k, nf, nb = _general_counts(sense, kind)
    return len(s) + nb, len(k) + nf + int(np.count_nonzero(s != _lib.SENSE_EQ)) + nb


def pack_general(P, lb, ub) -> np.ndarray:
    """problem blocks ``[B, m+1, ns+1]`` (``P[:, 0, 0] = -c0``) with lb, ub
    ``[B, ns]`` or ``[ns]`` -> general blocks ``[B, (m+1)(ns+1) + 2 ns]``: P,
    then lb, then ub; one block ``[m+1, ns+1]`` -> one flat block"""
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim == 2:
        return pack_general(P[None], lb, ub)[0]
    if P.ndim != 3 or P.shape[1] < 2 or P.shape[2] < 2:
        raise ValueError("problem blocks must be [B, m+1, ns+1] with m, ns >= 1")
    B, ns = P.shape[0], P.shape[2] - 1
    lo, hi = _bounds(lb, ub, (B, ns))
    return np.concatenate([P.reshape(B, -1), lo, hi], axis=1)


def _flip(a: np.ndarray) -> np.ndarray:
    """a copy with every sign bit flipped (NaN payloads survive)"""
    return (np.ascontiguousarray(a).view(np.uint64) ^ _SIGN).view(np.float64)


def general_standard_form(P, lb, ub, sense, kind, maximise=False) -> np.ndarray:
    """The host formula of k_general_shift and k_general_assemble: problem
    blocks ``[B, m+1, ns+1]`` (or one, ``[m+1, ns+1]``) with bounds, senses,
    kinds and a direction -> standard-form tableaux ``[B, m'+1, n'+1]``.
    Costs are flipped iff (maximise XOR UPPER), the rows of an UPPER variable
    and of a FREE one's negative part are flipped, column 0 is b_i (row 0: the
    stored _z cell, flipped iff maximise) less a_ij * s_j over the shifted j
    ascending, each product rounded first; a BOXED variable adds a row
    x' <= ub - lb.  One loop over j, so the order is the stated one."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim == 2:
        lo, hi = _bounds(lb, ub, (P.shape[1] - 1,))
        return general_standard_form(P[None], lo[None], hi[None], sense, kind, maximise)[0]
    s, k, nf, nb = _general_counts(sense, kind)
    B, m, ns = P.shape[0], P.shape[1] - 1, P.shape[2] - 1
    if len(s) != m or len(k) != ns:
        raise ValueError(f"the blocks have {m} rows and {ns} variables, not {len(s)} senses and {len(k)} kinds")
    lo, hi = _bounds(lb, ub, (B, ns))
    maximise = bool(maximise)
    ext = np.concatenate([s, np.full(nb, _lib.SENSE_LE, dtype=np.int8)])
    rows, cols, ones = _slack_columns(ext, ns + nf)
    T = np.zeros((B, m + nb + 1, 1 + ns + nf + len(rows)), dtype=np.float64)
    col0 = P[:, :, 0].copy()
    if maximise:
        col0[:, 0] = _flip(col0[:, 0])
    f = t = 0
    for j in range(ns):
        upper = k[j] == _lib.VAR_UPPER
        col = P[:, :, 1 + j].copy()
        if upper:
            col[:, 1:] = _flip(col[:, 1:])
        if maximise != upper:
            col[:, 0] = _flip(col[:, 0])
        T[:, :m + 1, 1 + j] = col
        if k[j] == _lib.VAR_FREE:
            neg = _flip(col)                            # the variable's own cells, each flipped once more
            T[:, :m + 1, 1 + ns + f] = neg
            f += 1
        if k[j] in _SHIFTED:
            a = P[:, :, 1 + j].copy()
            if maximise:
                a[:, 0] = _flip(a[:, 0])
            with np.errstate(invalid="ignore", over="ignore"):     # a NaN or an infinity is the caller's to keep
                prod = a * (hi if upper else lo)[:, j, None]
                col0 = col0 - prod
        if k[j] == _lib.VAR_BOXED:
            T[:, 1 + m + t, 0] = hi[:, j] - lo[:, j]
            T[:, 1 + m + t, 1 + j] = 1.0
            t += 1
    T[:, :m + 1, 0] = col0
    T[:, 1 + rows, 1 + cols] = ones
    return T


def general_recover(xstd, t00, lb, ub, kind, maximise=False):
    """The host formula of k_general_recover: xstd ``[B, n']`` (or ``[n']``)
    the standard form's variables, t00 its stored ``T[0][0]`` cells -> (x in
    the caller's variables, objective): the bits of x'_j for PLAIN, lb + x'_j
    for LOWER and BOXED, ub - x'_j for UPPER, x'_j - x'_neg for FREE; -t00
    under min, the bits of t00 under max."""
    k = _lib.kind_codes(kind)
    xs = np.asarray(xstd, dtype=np.float64)
    if xs.ndim == 1:
        lo, hi = _bounds(lb, ub, (len(k),))
        x, z = general_recover(xs[None], np.asarray(t00, dtype=np.float64).reshape(1), lo[None], hi[None], k, maximise)
        return x[0], z[0]
    ns = len(k)
    lo, hi = _bounds(lb, ub, (xs.shape[0], ns))
    x = np.ascontiguousarray(xs[:, :ns]).copy()
    f = 0
    for j in range(ns):
        if k[j] in (_lib.VAR_LOWER, _lib.VAR_BOXED):
            x[:, j] = lo[:, j] + xs[:, j]
        elif k[j] == _lib.VAR_UPPER:
            x[:, j] = hi[:, j] - xs[:, j]
        elif k[j] == _lib.VAR_FREE:
            x[:, j] = xs[:, j] - xs[:, ns + f]
            f += 1
    t00 = np.ascontiguousarray(t00, dtype=np.float64)
    return x, (t00.copy() if maximise else _flip(t00))


def general_duals(T, sense, kind, maximise=False):
    """The host formula of k_general_duals on one LP's stored standard-form
    tableau (only row 0 is read) -> (y ``[m]``, r ``[ns]``): y is
    problem_duals' value of the m original rows flipped iff maximise, the quiet
    NaN on an equality row; r_j is T[0, 1+j], less the cell under the slack of
    its bound row for BOXED, flipped iff (maximise XOR UPPER)."""
    s, k, nf, nb = _general_counts(sense, kind)
    m, ns = len(s), len(k)
    row0 = np.asarray(T, dtype=np.float64)[0]
    ext = np.concatenate([s, np.full(nb, _lib.SENSE_LE, dtype=np.int8)])
    rows, cols, ones = _slack_columns(ext, ns + nf)
    if 1 + ns + nf + len(rows) != len(row0):
        raise ValueError(f"the tableau has {len(row0) - 1} columns, the form gives {ns + nf + len(rows)}")
    y = np.full(m, QUIET_NAN, dtype=np.float64)
    own = rows < m
    c = row0[1 + cols[own]]
    yv = np.where(ones[own] > 0, _flip(c), c)
    y[rows[own]] = _flip(yv) if maximise else yv
    r = row0[1:ns + 1].copy()
    bcols = cols[~own]                          # the bound rows' slacks, in variable order
    boxed = np.nonzero(k == _lib.VAR_BOXED)[0]
    r[boxed] = r[boxed] - row0[1 + bcols]
    flip = (k == _lib.VAR_UPPER) != bool(maximise)
    r[flip] = _flip(r[flip])
    return y, r


def reprice_costs(T, basis, costs) -> np.ndarray:
    """The host formula of k_cost on one stored tableau: a copy of T whose row
    0 is the cost row ``costs`` (n + 1 values, costs[0] the stored ``_z``
    cell) less c_B times the rows of the basis:
    ``acc = costs[j]; for r: k = basis[r]; acc = acc - costs[1+k] * T[1+r][j]``,
    rows ascending, an entry outside [0, n) skipped, every product rounded
    before its subtraction (columns side by side: each is the same scalar
    float64 loop)."""
    T = np.array(T, dtype=np.float64)
    costs = np.asarray(costs, dtype=np.float64)
    n = T.shape[1] - 1
    if costs.shape != (n + 1,):
        raise ValueError(f"costs must hold {n + 1} values, not {costs.shape}")
    basis = np.asarray(basis).ravel()
    if len(basis) != T.shape[0] - 1:
        raise ValueError(f"basis must hold {T.shape[0] - 1} entries, not {len(basis)}")
    acc = costs.copy()
    with np.errstate(all="ignore"):
        for r, k in enumerate(basis):
            if k < 0 or k >= n:
                continue
            prod = costs[1 + int(k)] * T[1 + r]
            acc = acc - prod
    T[0] = acc
    return T


def extend_tableau(T, basis, rows, sense):
    """The host formula of lp_cut_extend on one stored tableau -> (D, basis'):
    T ``(m+1, n+1)`` with q stated rows ``(q, n+1)`` (beta, then one coefficient
    per tableau column) and q senses "<=" / ">=".  D ``(m+q+1, n+q+1)`` holds
    T's bits, +0.0 under the q new slack columns, the identity where the new
    rows meet them, and for new row k and column j
    ``acc = row_k[j]; for r: c = basis[r]; acc = acc - row_k[1+c] * T[1+r][j]``,
    rows ascending, an entry outside [0, n) skipped, every product rounded
    before its subtraction, the sign bit flipped for a ">=" row (columns side by
    side: each is the same scalar float64 loop).  basis' is basis followed by
    n .. n+q-1."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] < 2 or T.shape[1] < 2:
        raise ValueError("a tableau must be (m+1, n+1) with m, n >= 1")
    m, n = T.shape[0] - 1, T.shape[1] - 1
    rows = np.asarray(rows, dtype=np.float64)
    if rows.size == 0:
        rows = rows.reshape(0, n + 1)
    if rows.ndim != 2 or rows.shape[1] != n + 1:
        raise ValueError(f"rows must be (q, {n + 1}), not {rows.shape}")
    q = rows.shape[0]
    s = _lib.sense_codes([] if sense is None else sense)
    if len(s) != q:
        raise ValueError(f"sense must hold {q} entries, one per new row, not {len(s)}")
    if bool((s == _lib.SENSE_EQ).any()):
        raise ValueError('an "==" row owns no column: state it as a "<=" and a ">=" row')
    basis = np.asarray(basis).ravel()
    if len(basis) != m:
        raise ValueError(f"basis must hold {m} entries, not {len(basis)}")
    D = np.zeros((m + q + 1, n + q + 1), dtype=np.float64)
    D.view(np.uint64)[:m + 1, :n + 1] = T.view(np.uint64)
    acc = rows.copy()
    with np.errstate(all="ignore"):
        for r, c in enumerate(basis):
            if c < 0 or c >= n:
                continue
            prod = rows[:, 1 + int(c), None] * T[1 + r][None, :]
            acc = acc - prod
    acc[s == _lib.SENSE_GE] = _flip(acc[s == _lib.SENSE_GE])
    D[m + 1:, :n + 1] = acc
    D[m + 1 + np.arange(q), n + 1 + np.arange(q)] = 1.0
    return D, np.concatenate([basis.astype(np.int32), np.arange(n, n + q, dtype=np.int32)])


def general_cost_row(P_row0, lb, ub, kind, maximise=False, n=None) -> np.ndarray:
    """Row 0 of general_standard_form without the tableau: P_row0 ``[ns+1]``
    (or ``[B, ns+1]``), ``-c0`` then c, with the bounds, kinds and direction ->
    the cost row ``[1 + ns + nf]``: cell 0 the stored ``_z`` cell flipped iff
    maximise, less cs_j * s_j over the shifted j ascending; cell 1+j = c_j
    flipped iff (maximise XOR UPPER); a FREE variable's negative part that cell
    flipped once more.  The slack columns after them hold +0.0: with n given
    (the standard form's n') the row is padded to n + 1 cells."""
    row = np.ascontiguousarray(P_row0, dtype=np.float64)
    k = _lib.kind_codes(kind)
    if row.ndim == 1:
        lo, hi = _bounds(lb, ub, (len(k),))
        return general_cost_row(row[None], lo[None], hi[None], k, maximise, n)[0]
    B, ns = row.shape[0], row.shape[1] - 1
    if len(k) != ns:
        raise ValueError(f"the cost row has {ns} variables, not {len(k)} kinds")
    lo, hi = _bounds(lb, ub, (B, ns))
    maximise = bool(maximise)
    nf = int(np.count_nonzero(k == _lib.VAR_FREE))
    width = 1 + ns + nf if n is None else int(n) + 1
    if width < 1 + ns + nf:
        raise ValueError(f"n = {n} is below ns + nf = {ns + nf}")
    out = np.zeros((B, width), dtype=np.float64)
    cell0 = _flip(row[:, 0]) if maximise else row[:, 0].copy()
    f = 0
    for j in range(ns):
        upper = k[j] == _lib.VAR_UPPER
        c = row[:, 1 + j]
        out[:, 1 + j] = _flip(c) if maximise != upper else c
        if k[j] == _lib.VAR_FREE:
            out[:, 1 + ns + f] = _flip(out[:, 1 + j])
            f += 1
        if k[j] in _SHIFTED:
            a = _flip(c) if maximise else c
            with np.errstate(invalid="ignore", over="ignore"):
                prod = a * (hi if upper else lo)[:, j]
                cell0 = cell0 - prod
    out[:, 0] = cell0
    return out


_KIND_NEEDS = {_lib.VAR_PLAIN: "lb == 0 and ub == +inf", _lib.VAR_LOWER: "a finite lb and ub == +inf",
               _lib.VAR_BOXED: "both bounds finite", _lib.VAR_UPPER: "lb == -inf and a finite ub",
               _lib.VAR_FREE: "lb == -inf and ub == +inf"}


def _check_pattern(i, kind, lb, ub):
    """the bound-pattern rule of lp_reopt_set_general on LP i: ValueError naming the LP and the variable"""
    for j, (k, lo, hi) in enumerate(zip(kind, lb, ub)):
        flo, fhi = np.isfinite(lo), np.isfinite(hi)
        if np.isnan(lo) or np.isnan(hi):
            ok = False
        elif k == _lib.VAR_PLAIN:
            ok = lo == 0.0 and hi == np.inf
        elif k == _lib.VAR_LOWER:
            ok = flo and hi == np.inf
        elif k == _lib.VAR_BOXED:
            ok = flo and fhi
        elif k == _lib.VAR_UPPER:
            ok = lo == -np.inf and fhi
        else:
            ok = lo == -np.inf and hi == np.inf
        if not ok:
            raise ValueError(f"LP {i}, variable {j}: bounds [{lo}, {hi}] do not fit its kind {int(k)}, which needs "
                             f"{_KIND_NEEDS[int(k)]}: reoptimize() keeps the pattern of finite bounds (solve the "
                             "new form cold)")


class ProblemResult:
    """What solve_problems returns: per-LP arrays and the live engine.  x is
    ``[B, ns]`` (the structural variables), slack ``[B, m]`` the value of each
    row's slack or surplus variable (+0.0 on "==" rows), y ``[B, m]`` the dual
    values, fetched from the device on first use.  path is "plain" (every
    sense "<=" and every LP canonical: Simplex.solve alone) or "twophase".  On
    the plain path stage / rows / ninit are zeros / m / zeros.  reduced_costs
    ``[B, ns]`` is fetched on first use, as y is.  After a general-form call
    (kind is not None) x, objective, y, reduced_costs and slack are in the
    caller's terms -- slack the m original rows only -- while basis, rows and
    the logs speak of the standard form.

    resolve(b) re-solves the same LPs with other right-hand sides from the
    basis this result ended in (path "dual": npiv the dual pivots; stage, ninit
    and nstd zeros; basis fetched on first use).  The new result takes over the
    engine: this one keeps what it holds -- y is fetched for it first -- and
    raises RuntimeError on anything it would still have to fetch.

    reoptimize(b=, c=, lb=, ub=, c0=) is the wider warm call:
    new right-hand sides or bounds through the dual simplex (path "dual"), or
    new costs through the primal solve (path "primal"), on general-form
    results too; it takes over the engine as resolve does.  c, b, lb and ub
    of the call that made a result are kept on the host for it."""

    def __init__(self, engine, path, sense, ns, status, stage, rows, ninit, npiv, nstd, objective, basis, xall,
                 kind=None, maximize=None, x=None, z0=None, c=None, b=None, lb=None, ub=None):
        self._engine = engine
        self._stale = False
        self._host = dict(c=c, b=b, lb=lb, ub=ub)       # the call's data, for reoptimize()
        self._y = self._r = None
        self._basis = basis
        self._z0 = np.zeros(len(status)) if z0 is None else np.array(z0, dtype=np.float64)
        self.kind, self.maximize = kind, maximize
        self.path = path
        self.sense, self.ns = sense, ns
        self.status_code = status
        self.status = [_lib.STATUS_NAMES.get(int(s), str(int(s))) for s in status]
        self.stage, self.rows, self.ninit = stage, rows, ninit
        self.npiv, self.nstd = npiv, nstd
        self.objective = objective
        self.x, self.slack = self._split(xall)
        if x is not None:
            self.x = x

    @staticmethod
    def _nfree(kind) -> int:
        return 0 if kind is None else int(np.count_nonzero(np.asarray(kind) == _lib.VAR_FREE))

    def _split(self, xall):
        rows, cols, _ = _slack_columns(self.sense, self.ns + self._nfree(self.kind))
        slack = np.zeros((xall.shape[0], len(self.sense)), dtype=np.float64)
        slack[:, rows] = xall[:, cols]
        return np.ascontiguousarray(xall[:, :self.ns]), slack

    def __len__(self) -> int:
        return len(self.status)

    def _live(self):
        """the engine, while its tableaux are still this result's"""
        if self._stale:
            raise RuntimeError("resolve() has moved the engine on to other right-hand sides: this result keeps what it "
                               "had fetched, the rest is gone")
        return self._engine

    @property
    def basis(self):
        if self._basis is None:
            self._basis = self._live().get_basis()
        return self._basis

    @property
    def y(self):
        if self._y is None:
            eng = self._live()
            self._y = eng.duals() if self.kind is None else eng.general_duals(want_r=False)[0]
        return self._y

    def _plain_form(self):
        """the form of a problem-form call: every kind PLAIN, min"""
        self._engine.set_form(self.sense, np.zeros(self.ns, dtype=np.int8), False)

    @property
    def reduced_costs(self):
        if self._r is None:
            eng = self._live()
            if self.kind is None:
                self._plain_form()
            self._r = eng.general_duals(want_y=False)[1]
        return self._r

    def _nlog(self, i: int) -> int:
        return int(self.ninit[i])

    def init_log(self, i: int) -> np.ndarray:
        """phase-1 (r, c) pairs of LP i (none on the plain path)"""
        return self._live().log(i)[:self._nlog(i)]

    def log(self, i: int) -> np.ndarray:
        """phase-2 (r, c) pairs of LP i, oldest first (at most log_cap of them);
        after resolve(), its dual pivots"""
        return self._live().log(i)[self._nlog(i):]

    def tableau(self, i: int) -> Tableau:
        """LP i's final tableau, downloaded alone from the live engine"""
        return Tableau.fromArray(self._live().download(first=int(i), count=1)[0][:int(self.rows[i]) + 1])

    # -- warm re-solve ------------------------------------------------------
    def _senses(self):
        return [self.sense]

    def _rhs(self, b, z0):
        """-> (what set_rhs takes, the stored _z cells): b [B, m], z0 [B]"""
        b = np.asarray(b, dtype=np.float64)
        if b.shape != (len(self), len(self.sense)):
            raise ValueError(f"b must be ({len(self)}, {len(self.sense)}), not {b.shape}")
        return np.concatenate([z0[:, None], b], axis=1), z0

    def resolve(self, b, *, c0=None, max_pivots=None):
        """The same LPs with right-hand sides b, warm: the new column 0 is
        computed on the device from the stored tableaux (set_rhs), the dual
        simplex runs from the basis this result ended in (run(RULE_DUAL, cap)),
        and x and the objective are gathered (solution()).  Nothing is uploaded
        but b and nothing comes back but x and z.  c0: the objective's constant
        (None keeps the original call's).  max_pivots: the cap on dual pivots
        per LP; None is 10 * (m + n) of the largest LP, a guard -- the rule has
        no anti-cycling logic -- and an LP that reaches it reports "pivoted".
        -> a new result of this class on the same engine, path "dual".
        ValueError before any device call on a general-form result and on an LP
        with an "==" row."""
        if self.kind is not None:
            raise ValueError("resolve() is not available on a general-form result (lb, ub, maximize or c0 was given)")
        for i, s in enumerate(self._senses()):
            if bool((np.asarray(s) == _lib.SENSE_EQ).any()):
                raise ValueError(f"resolve() needs every row to own a column: LP {i} has an \"==\" row")
        n = len(self)
        z0 = self._z0 if c0 is None else -np.array(np.broadcast_to(np.asarray(c0, dtype=np.float64), (n,)))
        rhs, z0 = self._rhs(b, z0)
        if max_pivots is not None and int(max_pivots) < 0:
            raise ValueError("max_pivots must be >= 0")
        eng = self._live()
        shapes = eng.shapes if hasattr(eng, "shapes") else [(eng.m, eng.n)]
        cap = max(10 * (m + n_) for m, n_ in shapes) if max_pivots is None else int(max_pivots)
        self.y                          # this result's duals, while the tableaux are still its own
        eng.set_rhs(rhs)                # (a refusal changes nothing: this result stays live)
        self._stale = True
        status, done = eng.run(_lib.RULE_DUAL, cap)
        x, z = eng.solution()
        zeros = np.zeros(n, dtype=np.int64)
        return type(self)(eng, "dual", self.sense, self.ns, status, np.zeros(n, dtype=np.int32), np.array(self.rows),
                          zeros, done, zeros.copy(), z, None, x, z0=z0)

    # -- warm re-optimisation -------------------------------------------------
    def _forms(self):
        """(sense, ns, kind, maximize) per LP"""
        return [(self.sense, self.ns, self.kind, self.maximize)] * len(self)

    def _items(self, value, widths, name):
        """one value per LP as a list of 1-D arrays, the i-th of widths[i] entries; checked"""
        a = np.asarray(value, dtype=np.float64)
        if a.shape != (len(self), widths[0]):
            raise ValueError(f"{name} must be ({len(self)}, {widths[0]}), not {a.shape}")
        return list(a)

    @staticmethod
    def _stack(items):
        """per-LP arrays as the engine's data calls take them"""
        return np.stack(items)

    def _kept(self, name, widths):
        value = self._host[name]
        if value is None:
            raise ValueError(f"reoptimize() needs the {name} of the call that made this result, and it was not kept")
        return self._items(value, widths, name)

    def reoptimize(self, *, b=None, c=None, lb=None, ub=None, c0=None, max_pivots=None):
        """The same LPs with other data, warm, from the basis this result
        ended in.  One side per call: b, lb and ub are the dual side -- a
        change of the standard form's right-hand sides (set_rhs, or
        set_general on a general-form result), then run(RULE_DUAL, cap),
        path "dual"; c is the primal side -- row 0 re-priced from the basis
        (set_costs; on a general-form result after a set_general that stores
        the new c), then solve(max_pivots), path "primal", npiv and nstd those
        of that solve.  c0 (None keeps the stored constant) may go with either.
        Both sides, or neither, is a ValueError: chain two calls.  Shapes are
        those of the original call (per-LP lists on a ragged result); new
        bounds must keep each variable's kind, and an LP with an "==" row is
        refused on the dual side and on a general-form result -- all ValueError
        before any device call.  max_pivots: the cap per LP; None is
        10 * (m + n) of the largest LP on the dual side (see resolve) and no
        cap on the primal side.  An LP that was "infeasible" stays so under new
        costs: they do not change the feasible set, and it takes no pivot.
        -> a new result of this class on the same engine, as resolve()'s; on a
        general-form result x, objective, y and reduced_costs stay in the
        caller's terms."""
        dual = b is not None or lb is not None or ub is not None
        if dual == (c is not None):
            raise ValueError("reoptimize() takes one side per call: b, lb, ub (the dual side) or c (the primal "
                             "side); chain two calls for both")
        if max_pivots is not None and int(max_pivots) < 0:
            raise ValueError("max_pivots must be >= 0")
        n = len(self)
        forms = self._forms()
        general = self.kind is not None
        if not general and (lb is not None or ub is not None):
            raise ValueError("lb and ub need a general-form result (lb, ub, maximize or c0 given to the first call)")
        if dual or general:
            for i, f in enumerate(forms):
                if bool((np.asarray(f[0]) == _lib.SENSE_EQ).any()):
                    raise ValueError(f"reoptimize() needs every row to own a column: LP {i} has an \"==\" row")
        z0 = self._z0 if c0 is None else -np.array(np.broadcast_to(np.asarray(c0, dtype=np.float64), (n,)))
        ms, nss = [len(f[0]) for f in forms], [int(f[1]) for f in forms]
        new = {k: (None if v is None else self._items(v, ms if k == "b" else nss, k))
               for k, v in dict(c=c, b=b, lb=lb, ub=ub).items()}
        border = None
        if general:
            data = {k: (self._kept(k, ms if k == "b" else nss) if v is None else v) for k, v in new.items()}
            for i, f in enumerate(forms):
                _check_pattern(i, f[2], data["lb"][i], data["ub"][i])
            border = [np.concatenate([[z0[i]], data["c"][i], data["b"][i], data["lb"][i], data["ub"][i]])
                      for i in range(n)]
        elif dual:
            data = dict(self._host, b=new["b"])
        else:
            data = dict(self._host, c=new["c"])
        eng = self._live()
        shapes = eng.shapes if hasattr(eng, "shapes") else [(eng.m, eng.n)] * n
        self.y                          # this result's duals, while the tableaux are still its own
        if dual:
            cap = max(10 * (m + n_) for m, n_ in shapes) if max_pivots is None else int(max_pivots)
            if general:
                eng.set_general(self._stack(border))        # (a refusal changes nothing: this result stays live)
            else:
                eng.set_rhs(self._stack([np.concatenate([[z], v]) for z, v in zip(z0, new["b"])]))
            self._stale = True
            status, npiv = eng.run(_lib.RULE_DUAL, cap)
            nstd = np.zeros(n, dtype=np.int64)
        else:
            if general:
                rows = [general_cost_row(np.concatenate([[z0[i]], new["c"][i]]), data["lb"][i], data["ub"][i],
                                         forms[i][2], forms[i][3], shapes[i][1]) for i in range(n)]
            else:
                rows = [np.concatenate([[z0[i]], new["c"][i], np.zeros(shapes[i][1] - nss[i])]) for i in range(n)]
            # an infeasible LP's tableau is no primal start: it gets +0.0 costs for the solve, which takes
            # no pivot on it, and its own costs afterwards
            held = [i for i in range(n) if int(self.status_code[i]) == _lib.INFEASIBLE]
            staged = [np.zeros_like(r) if i in held else r for i, r in enumerate(rows)]
            if general:
                eng.set_general(self._stack(border))
            eng.set_costs(self._stack(staged))
            self._stale = True
            status, npiv, nstd = eng.solve(-1 if max_pivots is None else int(max_pivots))
            for i in held:
                eng.set_costs(self._stack([rows[i]]), first=i)
                status[i] = _lib.INFEASIBLE
        if general:
            x, z = eng.general_solution()
            xall, _ = eng.solution(want_z=False)
        else:
            (xall, z), x = eng.solution(), None
        keep = {k: (None if v is None else (v if not isinstance(v, list) else self._stack(v))) for k, v in data.items()}
        return type(self)(eng, "dual" if dual else "primal", self.sense, self.ns, status, np.zeros(n, dtype=np.int32),
                          np.array(self.rows), np.zeros(n, dtype=np.int64), npiv, nstd, z, None, xall,
                          kind=self.kind, maximize=self.maximize, x=x, z0=z0, **keep)


    # -- warm cuts -------------------------------------------------------------
    def _cuts(self, A, b, sense):
        """-> per LP (A_i [q, ns], b_i [q], senses [q]): A [B, q, ns], b [B, q], sense q entries every LP shares"""
        A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if A.ndim != 3 or A.shape[0] != len(self) or A.shape[2] != self.ns:
            raise ValueError(f"A must be ({len(self)}, q, {self.ns}), not {A.shape}")
        if b.shape != A.shape[:2]:
            raise ValueError(f"b must be {A.shape[:2]}, not {b.shape}")
        s = _lib.sense_codes(["<="] * A.shape[1] if sense is None else sense)
        if len(s) != A.shape[1]:
            raise ValueError(f"sense must hold {A.shape[1]} entries, one per new row, not {len(s)}")
        return [(A[i], b[i], s) for i in range(len(self))]

    def _joined(self, senses):
        """this result's senses with the new rows': what the new result holds as `sense`"""
        return np.concatenate([self.sense, senses[0]])

    def add_rows(self, A, b, sense=None, *, max_pivots=None, place=None):
        """The same LPs with q more constraints A x {<=, >=} b, warm (DESIGN.md
        4s): A ``[B, q, ns]``, b ``[B, q]``, sense q entries every LP shares
        (None: all "<=").  Each row is padded with +0.0 under the slack columns;
        a new engine gets the stored tableaux with the rows priced out against
        the basis this result ended in (extend), the dual simplex runs there
        (run(RULE_DUAL, cap)) and x and the objective are gathered.  max_pivots:
        the cap per LP; None is 10 * (m' + n') of the largest extended LP (see
        resolve).  place: the new engine's placement; None keeps this one's.
        -> a new result of this class on the new engine: path "dual", sense
        joined, rows = m + q, c kept and b with the new right-hand sides
        appended; y, resolve(), reoptimize(c=) and add_rows work on it.  This
        result stays live: nothing takes over its engine.  ValueError before
        any device call on a general-form result (the standard form keeps its
        bound rows after the m rows), an "==" row, wrong shapes, a result whose
        phase 1 dropped rows, and a negative max_pivots."""
        if self.kind is not None:
            raise ValueError("add_rows() is not available on a general-form result (lb, ub, maximize or c0 was given)")
        if max_pivots is not None and int(max_pivots) < 0:
            raise ValueError("max_pivots must be >= 0")
        cuts = self._cuts(A, b, sense)
        old = self._senses() * (len(self) if len(self._senses()) == 1 else 1)
        for i, ((_, _, s), s0) in enumerate(zip(cuts, old)):
            if bool((s == _lib.SENSE_EQ).any()):
                raise ValueError(f'add_rows() takes "<=" and ">=" rows: LP {i} is given an "==" row, which owns no '
                                 'column (state it as a "<=" and a ">=" row)')
            if int(self.rows[i]) < len(s0):
                raise ValueError(f"LP {i}: phase 1 left {int(self.rows[i])} of its {len(s0)} rows live; solve the "
                                 "extended LP cold")
        eng = self._live()
        widths = [n for _, n in eng._lp_shapes()]
        nss = [Ai.shape[1] for Ai, _, _ in cuts]
        rows = [np.concatenate([bi[:, None], Ai, np.zeros((len(bi), w - ns))], axis=1)
                for (Ai, bi, _), w, ns in zip(cuts, widths, nss)]
        senses = [s for _, _, s in cuts]
        new = eng.extend(rows, senses, place=place)
        cap = max(10 * (m + n) for m, n in new._lp_shapes()) if max_pivots is None else int(max_pivots)
        status, done = new.run(_lib.RULE_DUAL, cap)
        x, z = new.solution()
        n = len(self)
        zeros = np.zeros(n, dtype=np.int64)
        keep = dict(c=self._host["c"], b=self._host["b"])
        if keep["b"] is not None:
            keep["b"] = self._stack([np.concatenate([np.asarray(v, dtype=np.float64), bi])
                                     for v, (_, bi, _) in zip(keep["b"], cuts)])
        return type(self)(new, "dual", self._joined(senses), self.ns, status, np.zeros(n, dtype=np.int32),
                          np.array(self.rows) + np.array([len(s) for s in senses], dtype=np.int64), zeros, done,
                          zeros.copy(), z, None, x, z0=self._z0, **keep)


class ProblemRaggedResult(ProblemResult):
    """What solve_problems_ragged returns: ProblemResult with sense, ns as
    per-LP lists and x, slack, y, basis as lists of per-LP arrays."""

    def _cuts(self, A, b, sense):
        """A, b, sense: one entry per LP, (q_i, ns_i), q_i and q_i entries (sense None, or an entry None: all "<=")"""
        As, bs = list(A), list(b)
        ss = [None] * len(self) if sense is None else list(sense)
        if len(As) != len(self) or len(bs) != len(self) or len(ss) != len(self):
            raise ValueError("A, b and sense must hold one entry per LP")
        out = []
        for i, (Ai, bi, si, ns) in enumerate(zip(As, bs, ss, self.ns)):
            bi = np.asarray(bi, dtype=np.float64).ravel()
            Ai = np.asarray(Ai, dtype=np.float64)
            if Ai.size == 0:
                Ai = Ai.reshape(0, ns)
            if Ai.ndim != 2 or Ai.shape != (len(bi), ns):
                raise ValueError(f"A of LP {i} must be ({len(bi)}, {ns}), not {Ai.shape}")
            s = _lib.sense_codes(["<="] * len(bi) if si is None else si)
            if len(s) != len(bi):
                raise ValueError(f"sense of LP {i} must hold {len(bi)} entries, not {len(s)}")
            out.append((Ai, bi, s))
        return out

    def _joined(self, senses):
        return [np.concatenate([a, b]) for a, b in zip(self.sense, senses)]

    def _split(self, xall):
        xs, slacks = [], []
        kinds = [None] * len(xall) if self.kind is None else self.kind
        for x, s, ns, k in zip(xall, self.sense, self.ns, kinds):
            rows, cols, _ = _slack_columns(s, ns + self._nfree(k))
            slack = np.zeros(len(s), dtype=np.float64)
            slack[rows] = x[cols]
            xs.append(np.ascontiguousarray(x[:ns]))
            slacks.append(slack)
        return xs, slacks

    def _plain_form(self):
        self._engine.set_form(self.sense, [np.zeros(ns, dtype=np.int8) for ns in self.ns], None)

    def _senses(self):
        return self.sense

    def _rhs(self, b, z0):
        """b: one array of m_i entries per LP"""
        items = [np.asarray(v, dtype=np.float64).ravel() for v in b]
        if len(items) != len(self) or any(len(v) != len(s) for v, s in zip(items, self.sense)):
            raise ValueError("b must hold one array of m_i entries per LP")
        return [np.concatenate([[z], v]) for z, v in zip(z0, items)], z0

    def _forms(self):
        n = len(self)
        kinds = [None] * n if self.kind is None else self.kind
        mxs = [None] * n if self.maximize is None else self.maximize
        return list(zip(self.sense, self.ns, kinds, mxs))

    def _items(self, value, widths, name):
        items = [np.asarray(v, dtype=np.float64).ravel() for v in value]
        if len(items) != len(self):
            raise ValueError(f"{name} must hold one array per LP")
        for i, (v, w) in enumerate(zip(items, widths)):
            if len(v) != w:
                raise ValueError(f"{name} of LP {i} must hold {w} entries, not {len(v)}")
        return items

    @staticmethod
    def _stack(items):
        return list(items)


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


def _dual_method(method, general, senses):
    """method="dual" of solve_problems / solve_problems_ragged, checked -> bool"""
    if method not in ("primal", "dual"):
        raise ValueError('method must be "primal" or "dual"')
    if method == "primal":
        return False
    if general:
        raise ValueError('method="dual" takes problem-form LPs only: no lb, ub, maximize or c0')
    if not all(bool((s == _lib.SENSE_LE).all()) for s in senses):
        raise ValueError('method="dual" needs every sense "<=" (write a ">=" row as -A x <= -b)')
    return True


def _run_dual(eng, slack_basis, max_pivots):
    """the dual simplex from the slack basis on an engine that holds the
    assembled tableaux -> (status, done)"""
    shapes = eng.shapes if hasattr(eng, "shapes") else [(eng.m, eng.n)]
    cap = max(10 * (m + n) for m, n in shapes) if max_pivots is None else int(max_pivots)
    eng.set_basis(slack_basis)
    return eng.run(_lib.RULE_DUAL, cap)


def solve_problems(c, A, b, sense=None, *, max_pivots=None, tol=None, log_cap=0, device=0,
                   place="lds", lb=None, ub=None, maximize=False, c0=None, method="primal") -> ProblemResult:
    """min c.x subject to A x {<=, >=, ==} b, x >= 0 for B LPs of one shape: c
    ``[B, ns]``, A ``[B, m, ns]``, b ``[B, m]``, sense m entries shared by
    every LP ("<=", ">=", "==" or _lib.SENSE_*; None: all "<=").  The tableaux
    are assembled on the device; if every sense is "<=" and every LP is
    canonical (all b_i >= 0) Simplex.solve runs alone, else phase 1 runs first
    (lp_twophase_solve, or lp_phased_solve when place is not "lds"); x, the
    objective and, on first use, the duals are gathered on the device, and no
    tableau is downloaded.  Argument errors are ValueError before any device
    call.

    With lb, ub (``[ns]`` or ``[B, ns]``; -inf / +inf where absent), maximize
    or c0 (``[B]`` or a scalar, the objective's constant) given, the LP is
    min or max of c0 + c.x under lb <= x <= ub: the kinds come from
    general_kinds, the standard form is built and undone on the device
    (lp_general_*), and the result is in the caller's terms.  With none of them
    given the call is the one above.

    method="dual" is the cold start of the dual simplex, for LPs with every
    sense "<=", any sign of b and every c_j >= 0 (a covering LP written as
    -A x <= -b): the tableaux are assembled as above, the basis is the slack
    columns, and run(RULE_DUAL, cap) pivots to the optimum -- no phase 1, no
    artificial columns.  cap is max_pivots, or 10 * (m + n) when None; path is
    "dual".  An LP with a negative cost reports "bad_arg".  Any other sense or
    a general-form keyword with it is a ValueError."""
    general = lb is not None or ub is not None or bool(maximize) or c0 is not None
    z0 = None
    if c0 is not None:
        z0 = -np.broadcast_to(np.asarray(c0, dtype=np.float64), (np.shape(A)[0],) if np.ndim(A) == 3 else (1,))
    P = pack_problems(c, A, b, z0)
    B, m, ns = P.shape[0], P.shape[1] - 1, P.shape[2] - 1
    s = _lib.sense_codes(["<="] * m if sense is None else sense)
    if len(s) != m:
        raise ValueError(f"sense must hold {m} entries, one per row, not {len(s)}")
    placed = _lib.place_code(place) != _lib.PLACE_LDS
    dual = _dual_method(method, general, [s])
    if general:
        lo, hi = _bounds(lb, ub, (B, ns))
        kind = general_kinds(lo, hi)
        mp, np_ = general_shape(s, kind)
        eng = _lib.BatchEngine(B, mp, np_, log_cap=log_cap, device=device, place=place)
        if tol:
            eng.set_tol(**tol)
        eng.set_form(s, kind, bool(maximize))
        eng.upload_general(pack_general(P, lo, hi))
        path, status, stage, rows, ninit, npiv, nstd = _run(eng, bool((s == _lib.SENSE_LE).all()), placed, max_pivots)
        x, z = eng.general_solution()
        xall, _ = eng.solution(want_z=False)
        return ProblemResult(eng, path, s, ns, status, stage, rows, ninit, npiv, nstd, z, eng.get_basis(), xall,
                             kind=kind, maximize=bool(maximize), x=x, z0=P[:, 0, 0], c=P[:, 0, 1:].copy(),
                             b=P[:, 1:, 0].copy(), lb=lo, ub=hi)
    eng = _lib.BatchEngine(B, m, problem_columns(s, ns), log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.set_senses(s)
    eng.upload_problems(P)
    if dual:
        status, done = _run_dual(eng, np.tile(np.arange(ns, ns + m, dtype=np.int32), (B, 1)), max_pivots)
        x, z = eng.solution()
        zeros = np.zeros(B, dtype=np.int64)
        return ProblemResult(eng, "dual", s, ns, status, np.zeros(B, dtype=np.int32), np.full(B, m, dtype=np.int64),
                             zeros, done, zeros.copy(), z, None, x, c=P[:, 0, 1:].copy(), b=P[:, 1:, 0].copy())
    path, status, stage, rows, ninit, npiv, nstd = _run(eng, bool((s == _lib.SENSE_LE).all()), placed, max_pivots)
    x, z = eng.solution()
    return ProblemResult(eng, path, s, ns, status, stage, rows, ninit, npiv, nstd, z, eng.get_basis(), x,
                         c=P[:, 0, 1:].copy(), b=P[:, 1:, 0].copy())


def _per_lp(value, count, name):
    """None, or one entry per LP"""
    if value is None:
        return [None] * count
    value = list(value)
    if len(value) != count:
        raise ValueError(f"{name} must hold one entry per LP")
    return value


def solve_problems_ragged(problems, *, max_pivots=None, tol=None, log_cap=0, device=0,
                          place="lds", lb=None, ub=None, maximize=False, c0=None,
                          method="primal") -> ProblemRaggedResult:
    """solve_problems for LPs of any shapes: problems is a sequence of
    (c, A, b, sense), c ``[ns_i]``, A ``[m_i, ns_i]``, b ``[m_i]`` and sense
    m_i entries or None (all "<=").  The plain path is taken when every sense
    of every LP is "<=" and every LP is canonical.

    General form: an item may be (c, A, b, sense, lb, ub, maximize), or lb, ub
    and c0 may be given as one entry per LP and maximize as one flag or one
    per LP; each LP then has its own kinds and direction.  With none of them
    given the call is the one above.

    method="dual": as solve_problems', every LP from its slack basis; the cap
    when max_pivots is None is 10 * (m + n) of the largest LP."""
    items = list(problems)
    if not items:
        raise ValueError("empty batch")
    general = (lb is not None or ub is not None or c0 is not None or np.any(maximize)
               or any(len(item) == 7 for item in items))
    if general:
        _dual_method(method, True, [])
        return _solve_general_ragged(items, lb, ub, maximize, c0, max_pivots, tol, log_cap, device, place)
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
    dual = _dual_method(method, False, senses)
    eng = _lib.RaggedEngine(shapes, log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.set_senses(senses)
    eng.upload_problems(blocks)
    if dual:
        status, done = _run_dual(eng, [np.arange(ns, ns + m, dtype=np.int32) for (m, _), ns in zip(shapes, nss)],
                                 max_pivots)
        x, z = eng.solution()
        zeros = np.zeros(len(items), dtype=np.int64)
        return ProblemRaggedResult(eng, "dual", senses, nss, status, np.zeros(len(items), dtype=np.int32),
                                   np.array([m for m, _ in shapes], dtype=np.int64), zeros, done, zeros.copy(), z,
                                   None, x, c=[p[0, 1:].copy() for p in blocks], b=[p[1:, 0].copy() for p in blocks])
    all_le = all(bool((s == _lib.SENSE_LE).all()) for s in senses)
    path, status, stage, rows, ninit, npiv, nstd = _run(eng, all_le, placed, max_pivots)
    x, z = eng.solution()
    return ProblemRaggedResult(eng, path, senses, nss, status, stage, rows, ninit, npiv, nstd, z, eng.get_basis(), x,
                               c=[p[0, 1:].copy() for p in blocks], b=[p[1:, 0].copy() for p in blocks])


def _solve_general_ragged(items, lb, ub, maximize, c0, max_pivots, tol, log_cap, device, place):
    """the general path of solve_problems_ragged"""
    n = len(items)
    lbs, ubs, c0s = _per_lp(lb, n, "lb"), _per_lp(ub, n, "ub"), _per_lp(c0, n, "c0")
    mxs = [bool(maximize)] * n if np.ndim(maximize) == 0 else [bool(v) for v in _per_lp(maximize, n, "maximize")]
    blocks, senses, kinds, packed, los, his = [], [], [], [], [], []
    for i, item in enumerate(items):
        if len(item) not in (4, 7):
            raise ValueError(f"LP {i} must be (c, A, b, sense) or (c, A, b, sense, lb, ub, maximize)")
        ci, Ai, bi, si = item[:4]
        if len(item) == 7:
            lbs[i], ubs[i], mxs[i] = item[4], item[5], bool(item[6])
        try:
            P = _pack_one(ci, Ai, bi)
            if c0s[i] is not None:
                P[0, 0] = -float(c0s[i])
            m, ns = P.shape[0] - 1, P.shape[1] - 1
            s = _lib.sense_codes(["<="] * m if si is None else si)
            if len(s) != m:
                raise ValueError(f"sense must hold {m} entries, one per row, not {len(s)}")
            lo, hi = _bounds(lbs[i], ubs[i], (ns,))
            kinds.append(general_kinds(lo, hi))
        except ValueError as e:
            raise ValueError(f"LP {i}: {e}") from None
        blocks.append(P)
        senses.append(s)
        packed.append(pack_general(P, lo, hi))
        los.append(lo)
        his.append(hi)
    nss = [p.shape[1] - 1 for p in blocks]
    shapes = [general_shape(s, k) for s, k in zip(senses, kinds)]
    placed = _lib.place_code(place) != _lib.PLACE_LDS
    eng = _lib.RaggedEngine(shapes, log_cap=log_cap, device=device, place=place)
    if tol:
        eng.set_tol(**tol)
    eng.set_form(senses, kinds, mxs)
    eng.upload_general(packed)
    all_le = all(bool((s == _lib.SENSE_LE).all()) for s in senses)
    path, status, stage, rows, ninit, npiv, nstd = _run(eng, all_le, placed, max_pivots)
    x, z = eng.general_solution()
    xall, _ = eng.solution(want_z=False)
    return ProblemRaggedResult(eng, path, senses, nss, status, stage, rows, ninit, npiv, nstd, z, eng.get_basis(),
                               xall, kind=kinds, maximize=mxs, x=x, z0=[p[0, 0] for p in blocks],
                               c=[p[0, 1:].copy() for p in blocks], b=[p[1:, 0].copy() for p in blocks], lb=los, ub=his)
