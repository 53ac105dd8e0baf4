"""ctypes binding of liblpgpu.so (C-ABI: include/lpgpu.h).

This is the only module that touches the shared library.  There is no CPU
fallback: if the library is missing or no GPU is visible, every device
operation raises ``EngineUnavailable`` loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# LPGPU_LIB selects another build of the same library (A/B timing of variants)
LIB_PATH = os.environ.get("LPGPU_LIB") or os.path.join(HERE, "_lib", "liblpgpu.so")

# lp_status
PIVOTED, OPTIMAL, UNBOUNDED = 0, 1, 2
ZERO_PIVOT, BAD_ARG, DEVICE_ERROR, CAP_REACHED, BAD_PIVOT = -1, -2, -3, -4, -5
OBJ_INCREASED = -6
INFEASIBLE, PHASE1_FAILED = -7, -8
# LP_STAGE_* (lp_twophase_solve)
STAGE_PHASE2, STAGE_ARTIFICIAL, STAGE_DRIVE_OUT = 0, 1, 2
STATUS_NAMES = {PIVOTED: "pivoted", OPTIMAL: "optimal", UNBOUNDED: "unbounded",
                ZERO_PIVOT: "zero_pivot", BAD_ARG: "bad_arg", DEVICE_ERROR: "device_error",
                CAP_REACHED: "cap_reached", BAD_PIVOT: "bad_pivot",
                OBJ_INCREASED: "objective_increased", INFEASIBLE: "infeasible",
                PHASE1_FAILED: "phase1_failed"}
# lp_exchange_path
PATH_KERNELS, PATH_PERSISTENT, PATH_PEER, PATH_COLLECTIVE = 0, 1, 2, 3
PATH_NAMES = {PATH_KERNELS: "per-pivot kernels", PATH_PERSISTENT: "persistent selection",
              PATH_PEER: "persistent selection, device-side peer exchange",
              PATH_COLLECTIVE: "per-pivot kernels, one collective per pivot"}
# lp_rule
RULE_STANDARD, RULE_MIN_INDEX = 0, 1
RULE_MAX_INCREASE = 2       # findPivotMaxIncrease: BatchEngine.run / RaggedEngine.run only
RULE_DUAL = 3               # one dual simplex step per LP: BatchEngine.run / RaggedEngine.run only
# LP_PLACE_* (lp_placed_create): where a batch keeps an LP's tableau during a launch
PLACE_LDS, PLACE_AUTO, PLACE_DEVICE = 0, 1, 2
PLACES = {"lds": PLACE_LDS, "auto": PLACE_AUTO, "device": PLACE_DEVICE}
PLACE_NAMES = {PLACE_LDS: "lds", PLACE_DEVICE: "device"}
# LP_SENSE_* (lp_problem_set_senses): one per constraint row of an LP in problem form
SENSE_LE, SENSE_GE, SENSE_EQ = 0, 1, 2
SENSES = {"<=": SENSE_LE, ">=": SENSE_GE, "==": SENSE_EQ}
# LP_VAR_* (lp_general_set_form): one per variable of an LP in general form
VAR_PLAIN, VAR_LOWER, VAR_BOXED, VAR_UPPER, VAR_FREE = 0, 1, 2, 3, 4


class EngineUnavailable(RuntimeError):
    """liblpgpu.so could not be loaded or no GPU is visible."""


class DeviceError(RuntimeError):
    """A HIP/RCCL call failed inside the engine."""


class Tol(C.Structure):
    _fields_ = [("cost", C.c_double), ("cost_tie", C.c_double), ("pivot", C.c_double),
                ("zero", C.c_double), ("ratio_tie", C.c_double), ("stall", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


_H = C.c_void_p
_I64 = C.c_int64
_P64 = C.POINTER(C.c_int64)
_PD = C.POINTER(C.c_double)
_P32 = C.POINTER(C.c_int32)
_P8 = C.POINTER(C.c_int8)

_PROTOS = {
    "lp_default_tol": (None, [C.POINTER(Tol)]),
    "lp_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "lp_create": (C.c_int, [_I64, _I64, C.c_int, C.POINTER(_H)]),
    "lp_comm_unique_id": (C.c_int, [C.c_void_p]),
    "lp_create_sharded": (C.c_int, [_I64, _I64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.POINTER(_H)]),
    "lp_create_group": (C.c_int, [_I64, _I64, C.c_int, C.c_int, C.POINTER(_H)]),
    "lp_shard_rows": (C.c_int, [_H, _P64, _P64]),
    "lp_destroy": (C.c_int, [_H]),
    "lp_set_tol": (C.c_int, [_H, C.POINTER(Tol)]),
    "lp_get_tol": (C.c_int, [_H, C.POINTER(Tol)]),
    "lp_upload_rows": (C.c_int, [_H, _I64, _I64, _PD, _I64]),
    "lp_download_rows": (C.c_int, [_H, _I64, _I64, _PD, _I64]),
    "lp_pivot": (C.c_int, [_H, _I64, _I64]),
    "lp_find_pivot": (C.c_int, [_H, C.c_int, C.c_int, _P64, _P64]),
    "lp_pivot_checked": (C.c_int, [_H, _I64, _I64]),
    "lp_solve": (C.c_int, [_H, _I64, _P64, _P64]),
    "lp_run": (C.c_int, [_H, C.c_int, _I64, _P64]),
    "lp_pivot_log": (C.c_int, [_H, _P64, _I64, _P64]),
    "lp_objective": (C.c_int, [_H, _PD]),
    "lp_set_block": (C.c_int, [_H, C.c_int]),
    "lp_get_block": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "lp_profile": (C.c_int, [_H, C.c_int]),
    "lp_update_time": (C.c_int, [_H, _PD, _P64]),
    "lp_select_time": (C.c_int, [_H, _PD, _P64]),
    "lp_find_pivot_max_increase": (C.c_int, [_H, C.c_int, _P64, _P64]),
    "lp_find_pivot_all": (C.c_int, [_H, _P64, _I64, _P64]),
    "lp_form_checks": (C.c_int, [_H, C.POINTER(C.c_int32), _P64]),
    "lp_peer_handle": (C.c_int, [_H, C.c_char_p]),
    "lp_peer_open": (C.c_int, [_H, C.c_char_p]),
    "lp_peer_enable": (C.c_int, [_H, C.c_int]),
    "lp_set_host_allgather": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "lp_exchange_path": (C.c_int, [_H, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lp_xwait": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lp_last_error": (C.c_char_p, [_H]),
    "lp_batch_create": (C.c_int, [_I64, _I64, _I64, _I64, C.c_int, C.POINTER(_H)]),
    "lp_batch_destroy": (C.c_int, [_H]),
    "lp_batch_set_tol": (C.c_int, [_H, C.POINTER(Tol)]),
    "lp_batch_set_chunk": (C.c_int, [_H, _I64]),
    "lp_batch_upload": (C.c_int, [_H, _I64, _I64, _PD, _I64]),
    "lp_batch_download": (C.c_int, [_H, _I64, _I64, _PD, _I64]),
    "lp_batch_set_basis": (C.c_int, [_H, _P32]),
    "lp_batch_get_basis": (C.c_int, [_H, _P32]),
    "lp_batch_solve": (C.c_int, [_H, _I64, _P32, _P64, _P64]),
    "lp_batch_run": (C.c_int, [_H, C.c_int, _I64, _P32, _P64]),
    "lp_batch_objective": (C.c_int, [_H, _PD]),
    "lp_batch_log": (C.c_int, [_H, _I64, _P64, _I64, _P64]),
    "lp_batch_last_error": (C.c_char_p, [_H]),
    "lp_twophase_lds_bytes": (_I64, [_I64, _I64]),
    "lp_twophase_solve": (C.c_int, [_H, _I64, _P32, _P32, _P64, _P64, _P64, _P64]),
    "lp_ragged_create": (C.c_int, [_I64, _P64, _P64, _I64, C.c_int, C.POINTER(_H)]),
    "lp_ragged_shape": (C.c_int, [_H, _I64, _P64, _P64]),
    "lp_ragged_upload": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_ragged_download": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_ragged_set_basis": (C.c_int, [_H, _P32]),
    "lp_ragged_get_basis": (C.c_int, [_H, _P32]),
    "lp_ragged_plan": (C.c_int, [_H, C.c_int, _P64, _I64, _P64]),
    "lp_placed_create": (C.c_int, [_I64, _I64, _I64, _I64, C.c_int, C.c_int, C.POINTER(_H)]),
    "lp_placed_create_ragged": (C.c_int, [_I64, _P64, _P64, _I64, C.c_int, C.c_int, C.POINTER(_H)]),
    "lp_placed_placement": (C.c_int, [_H, _I64, C.POINTER(C.c_int)]),
    "lp_placed_lds_bytes": (_I64, [_I64, _I64]),
    "lp_phased_solve": (C.c_int, [_H, _I64, _P32, _P32, _P64, _P64, _P64, _P64]),
    "lp_phased_lds_bytes": (_I64, [_I64, _I64]),
    "lp_phased_placement": (C.c_int, [_H, _I64, C.POINTER(C.c_int)]),
    "lp_phased_plan": (C.c_int, [_H, _P64, _I64, _P64]),
    "lp_teamed_create": (C.c_int, [_I64, _I64, _I64, _I64, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    "lp_teamed_create_ragged": (C.c_int, [_I64, _P64, _P64, _I64, C.c_int, C.c_int, _P32, C.POINTER(_H)]),
    "lp_teamed_size": (C.c_int, [_H, _I64, C.POINTER(C.c_int)]),
    "lp_teamed_plan": (C.c_int, [_H, _P64, _I64, _P64]),
    "lp_teamed_set_window": (C.c_int, [_H, _I64]),
    "lp_solution_canonical": (C.c_int, [_H, _I64, _I64, _P32, _P64]),
    "lp_solution_gather": (C.c_int, [_H, _I64, _I64, _PD, _PD]),
    "lp_problem_columns": (_I64, [_P8, _I64, _I64]),
    "lp_problem_set_senses": (C.c_int, [_H, _P8]),
    "lp_problem_vars": (C.c_int, [_H, _I64, _P64]),
    "lp_problem_upload": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_problem_duals": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_resolve_set_rhs": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_general_rows": (_I64, [_P8, _P8, _I64, _I64]),
    "lp_general_columns": (_I64, [_P8, _P8, _I64, _I64]),
    "lp_general_set_form": (C.c_int, [_H, _P64, _P64, _P8, _P8, _P8]),
    "lp_general_vars": (C.c_int, [_H, _I64, _P64, _P64]),
    "lp_general_upload": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_general_solution": (C.c_int, [_H, _I64, _I64, _PD, _PD]),
    "lp_general_duals": (C.c_int, [_H, _I64, _I64, _PD, _PD]),
    "lp_reopt_set_costs": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_reopt_set_general": (C.c_int, [_H, _I64, _I64, _PD]),
    "lp_cut_extend": (C.c_int, [_H, _H, _I64, _I64, _PD, _P8]),
}

EXPORTS = tuple(_PROTOS)

_lib = None


def load(path: str = LIB_PATH):
    """Load liblpgpu.so (no GPU needed to load it)."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise EngineUnavailable(
            f"{path} is missing: build it with `make -C linear-program-solver_amd/csrc` "
            "or __graft_entry__.build() (there is no CPU fallback)")
    lib = C.CDLL(path)
    for name, (res, argt) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = argt
    if path == LIB_PATH:
        _lib = lib
    return lib


def default_tol() -> Tol:
    t = Tol()
    load().lp_default_tol(C.byref(t))
    return t


def device_count() -> int:
    n = C.c_int(0)
    load().lp_device_count(C.byref(n))
    return n.value


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_PD)


class Engine:
    """One device tableau (or one shard of a row-sharded one).

    Thin, typed wrapper of an ``lp_handle``: every method is one C-ABI call.
    ``rows()``/``put_rows()`` use GLOBAL row numbers (row 0 = objective)."""

    def __init__(self, m: int, n: int, device: int = 0, *, _handle=None):
        self.lib = load()
        self.m, self.n = int(m), int(n)
        self.device = device
        if _handle is not None:
            self.h = _handle
        else:
            if device_count() <= device:
                raise EngineUnavailable(
                    f"no GPU {device} visible (lp_device_count = {device_count()}); "
                    "the engine has no CPU fallback")
            h = _H()
            self._check(self.lib.lp_create(self.m, self.n, device, C.byref(h)), None)
            self.h = h
        b, c = C.c_int64(), C.c_int64()
        self.lib.lp_shard_rows(self.h, C.byref(b), C.byref(c))
        self.row_begin, self.row_count = b.value, c.value

    # -- plumbing ---------------------------------------------------------
    def _check(self, st: int, h) -> int:
        if st in (BAD_ARG,):
            raise ValueError(self._err(h))
        if st == DEVICE_ERROR:
            raise DeviceError(self._err(h))
        return st

    def _err(self, h) -> str:
        msg = self.lib.lp_last_error(h)
        return msg.decode() if msg else ""

    def close(self):
        if getattr(self, "h", None):
            self.lib.lp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- tolerances ---------------------------------------------------------
    def set_tol(self, **kw):
        t = self.get_tol()
        for k, v in kw.items():
            if not hasattr(t, k):
                raise KeyError(k)
            setattr(t, k, float(v))
        self.lib.lp_set_tol(self.h, C.byref(t))

    def get_tol(self) -> Tol:
        t = Tol()
        self.lib.lp_get_tol(self.h, C.byref(t))
        return t

    # -- data ---------------------------------------------------------------
    def put_rows(self, row0: int, rows: np.ndarray):
        a = np.ascontiguousarray(rows, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.n + 1:
            raise ValueError(f"rows must be (k, {self.n + 1}) float64")
        self._check(self.lib.lp_upload_rows(self.h, row0, a.shape[0], _ptr(a), a.shape[1]), self.h)

    def rows(self, row0: int, nrows: int) -> np.ndarray:
        out = np.empty((nrows, self.n + 1), dtype=np.float64)
        if nrows:
            self._check(self.lib.lp_download_rows(self.h, row0, nrows, _ptr(out), self.n + 1),
                        self.h)
        return out

    def upload(self, T: np.ndarray):
        """Whole tableau (single device) or row 0 + this shard's rows taken
        from a full-size array."""
        T = np.asarray(T, dtype=np.float64)
        if T.shape != (self.m + 1, self.n + 1):
            raise ValueError(f"tableau must be {(self.m + 1, self.n + 1)}")
        self.put_rows(0, T[:1])
        b = self.row_begin
        self.put_rows(1 + b, T[1 + b:1 + b + self.row_count])

    def download(self) -> np.ndarray:
        """Whole tableau (single device only)."""
        if self.row_count != self.m:
            raise ValueError("download() needs an unsharded engine; use rows()")
        return self.rows(0, self.m + 1)

    def objective(self) -> float:
        z = C.c_double()
        self._check(self.lib.lp_objective(self.h, C.byref(z)), self.h)
        return z.value

    # -- pivots -------------------------------------------------------------
    def pivot(self, r: int, c: int) -> int:
        return self._check(self.lib.lp_pivot(self.h, r, c), self.h)

    def pivot_checked(self, r: int, c: int) -> int:
        return self._check(self.lib.lp_pivot_checked(self.h, r, c), self.h)

    def find(self, rule: int, do_pivot: bool):
        """-> (r, c) | 'optimal' | 'unbounded'"""
        r, c = C.c_int64(), C.c_int64()
        st = self._check(self.lib.lp_find_pivot(self.h, rule, int(bool(do_pivot)),
                                                C.byref(r), C.byref(c)), self.h)
        if st == OPTIMAL:
            return "optimal"
        if st == UNBOUNDED:
            return "unbounded"
        if st != PIVOTED:
            raise DeviceError(f"unexpected status {STATUS_NAMES.get(st, st)}")
        return r.value, c.value

    def find_max_increase(self, do_pivot: bool):
        """findPivotMaxIncrease -> (r, c) | 'optimal' | 'unbounded'"""
        r, c = C.c_int64(), C.c_int64()
        st = self._check(self.lib.lp_find_pivot_max_increase(self.h, int(bool(do_pivot)),
                                                             C.byref(r), C.byref(c)), self.h)
        if st == OPTIMAL:
            return "optimal"
        if st == UNBOUNDED:
            return "unbounded"
        if st != PIVOTED:
            raise DeviceError(f"unexpected status {STATUS_NAMES.get(st, st)}")
        return r.value, c.value

    def find_all(self) -> list[tuple[int, int]]:
        """findPivotAll -> [(r, c), ...] column-major"""
        cnt = C.c_int64()
        self._check(self.lib.lp_find_pivot_all(self.h, None, 0, C.byref(cnt)), self.h)
        if cnt.value == 0:
            return []
        out = np.zeros(2 * cnt.value, dtype=np.int64)
        self._check(self.lib.lp_find_pivot_all(self.h, out.ctypes.data_as(_P64), cnt.value,
                                               C.byref(cnt)), self.h)
        return [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(cnt.value)]

    def form_checks(self):
        """-> dict(canonical, optimal, unbounded, infeasible, degenerate, bcols)"""
        flags = (C.c_int32 * 5)()
        bcols = np.full(self.m, -2, dtype=np.int64)
        self._check(self.lib.lp_form_checks(self.h, flags, bcols.ctypes.data_as(_P64)), self.h)
        keys = ("canonical", "optimal", "unbounded", "infeasible", "degenerate")
        out = {k: bool(flags[i]) for i, k in enumerate(keys)}
        out["bcols"] = None if np.all(bcols == -2) and self.m else [int(x) for x in bcols]
        return out

    def solve(self, max_pivots: int = -1):
        """-> (status, npiv, nstd)"""
        a, b = C.c_int64(), C.c_int64()
        st = self._check(self.lib.lp_solve(self.h, max_pivots, C.byref(a), C.byref(b)), self.h)
        return st, a.value, b.value

    def run(self, rule: int, k: int):
        """-> (status, pivots done)"""
        d = C.c_int64()
        st = self._check(self.lib.lp_run(self.h, rule, k, C.byref(d)), self.h)
        return st, d.value

    def log(self) -> np.ndarray:
        cnt = C.c_int64()
        self.lib.lp_pivot_log(self.h, None, 0, C.byref(cnt))
        out = np.zeros((cnt.value, 2), dtype=np.int64)
        if cnt.value:
            self._check(self.lib.lp_pivot_log(self.h, out.ctypes.data_as(_P64), cnt.value,
                                              C.byref(cnt)), self.h)
        return out

    def exchange_path(self):
        """-> (lp_exchange_path of the last solve/run, timed-out groups redone)"""
        p, f = C.c_int(), C.c_int()
        self.lib.lp_exchange_path(self.h, C.byref(p), C.byref(f))
        return p.value, f.value

    def xwait(self):
        """-> (cross-rank hop seconds, pivots) of the row-sharded persistent
        selection, cumulative (lp_xwait: block 0, 100 MHz device clock)"""
        t, n = C.c_int64(), C.c_int64()
        self.lib.lp_xwait(self.h, C.byref(t), C.byref(n))
        return t.value * 1e-8, n.value

    def set_block(self, pivots_per_sweep: int):
        """pivots deferred into one sweep of the tableau (1..64; 0 = auto)"""
        self._check(self.lib.lp_set_block(self.h, int(pivots_per_sweep)), self.h)

    def geometry(self) -> dict:
        """diagnostics (lpdiag_geometry): the persistent selection's launch
        geometry for this handle and what its last launch found on the device"""
        out = (C.c_longlong * 9)()
        self._check(self.lib.lpdiag_geometry(self.h, out), self.h)
        keys = ("blocks", "ipl", "rpl", "nr", "one_xcd_grid", "two_level_variant", "sel", "flags", "xcd_shards")
        d = dict(zip(keys, list(out)))
        d["kernel"] = "none" if d["blocks"] == 0 else "k_sel" if d["sel"] else "k_group"
        d["on_one_xcd"] = bool(d["flags"] & 1)
        d["two_level_engaged"] = bool(d["flags"] & 2)
        d["xcd_shards_engaged"] = bool(d["flags"] & 16)
        return d

    def sweep_buffers(self) -> int:
        """diagnostics (lpdiag_sweep_buffers): 2 when the sweeps run out of
        place (a second tableau buffer), 1 in place"""
        nb = C.c_int(0)
        self._check(self.lib.lpdiag_sweep_buffers(self.h, C.byref(nb)), self.h)
        return nb.value

    def sweep_clocks(self, cap: int = 1024) -> np.ndarray:
        """diagnostics (lpdiag_sweep_clocks): per 64-pivot sweep launch, its
        block 0's (launch number, shader cycles, 100 MHz ticks, start tick),
        the latest `cap` launches oldest first -- cycles / (ticks / 1e8) is
        the shader clock during that launch"""
        buf = (C.c_ulonglong * (4 * cap))()
        n = C.c_int(0)
        self._check(self.lib.lpdiag_sweep_clocks(self.h, buf, C.c_int(cap), C.byref(n)), self.h)
        return np.array(buf[:4 * n.value], dtype=np.uint64).reshape(-1, 4).astype(np.int64)

    def sweep_block_clocks(self, cap: int = 8192) -> np.ndarray:
        """diagnostics (lpdiag_sweep_block_clocks): every block's pass in the
        latest 64-pivot sweep launch -- (block, start tick, pass-end tick,
        shader cycles), 100 MHz ticks"""
        buf = (C.c_ulonglong * (4 * cap))()
        n = C.c_int(0)
        self._check(self.lib.lpdiag_sweep_block_clocks(self.h, buf, C.c_int(cap), C.byref(n)), self.h)
        return np.array(buf[:4 * n.value], dtype=np.uint64).reshape(-1, 4).astype(np.int64)

    def set_xcd_shards(self, on: bool):
        """diagnostics / A/B (lpdiag_set_xcd_shards): a tall single-device
        tableau runs k_sel as one row shard per XCD (default) or k_group"""
        self._check(self.lib.lpdiag_set_xcd_shards(self.h, 1 if on else 0), self.h)

    def get_block(self) -> int:
        """pivots per sweep in use (the auto choice resolved)"""
        b = C.c_int()
        self.lib.lp_get_block(self.h, C.byref(b))
        return b.value

    # -- timing -------------------------------------------------------------
    def profile(self, enable: bool, every: int = 1):
        """time the launches (every `every`-th of each kernel) with HIP events"""
        self.lib.lp_profile(self.h, max(1, int(every)) if enable else 0)

    def update_time(self):
        """-> (total ms, launches) of the rank-1 update kernel since profile()."""
        ms, n = C.c_double(), C.c_int64()
        self.lib.lp_update_time(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    # ---- device-side exchange between the ranks of a sharded job
    PEER_HANDLE_BYTES = 64

    def peer_handle(self) -> bytes:
        """This rank's exchange-buffer IPC handle (all-gather it in rank order)."""
        buf = C.create_string_buffer(self.PEER_HANDLE_BYTES)
        self._check(self.lib.lp_peer_handle(self.h, buf), self.h)
        return buf.raw

    def peer_open(self, handles: bytes):
        """Open every rank's buffer and check the exchange (collective)."""
        self._check(self.lib.lp_peer_open(self.h, handles), self.h)

    def peer_enable(self, enable: bool):
        self._check(self.lib.lp_peer_enable(self.h, 1 if enable else 0), self.h)

    def set_host_allgather(self, fn):
        """Give a multi-process shard the host's all-gather: fn(bytes) -> list
        of every rank's bytes in rank order (e.g. torch.distributed over gloo,
        see gloo_allgather).  The column scans combine through it; a handle
        without an RCCL communicator also runs its per-pivot exchanges
        through it."""
        cb = allgather_callback(fn)
        self._check(self.lib.lp_set_host_allgather(self.h, C.cast(cb, C.c_void_p), None), self.h)
        self._allgather_cb = cb     # the library holds the pointer: keep it alive

    def select_time(self):
        """-> (total ms, launches) of the pivot-selection kernel since profile()."""
        ms, n = C.c_double(), C.c_int64()
        self.lib.lp_select_time(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value


_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)


def allgather_callback(fn):
    """The C callback (lp_allgather_fn) around fn(bytes) -> [bytes per rank]."""
    def tramp(ctx, send, recv, nbytes):
        try:
            parts = fn(C.string_at(send, nbytes))
            blob = b"".join(parts)
            if len(blob) != nbytes * len(parts):
                return 1
            C.memmove(recv, blob, len(blob))
            return 0
        except Exception:       # noqa: BLE001 - no exception may cross the C ABI
            return 1
    return _ALLGATHER_FN(tramp)


def gloo_allgather(group=None):
    """A host all-gather over torch.distributed (CPU tensors: gloo) for
    Engine.set_host_allgather."""
    import torch
    import torch.distributed as dist

    def fn(data: bytes) -> list[bytes]:
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = [torch.empty_like(t) for _ in range(dist.get_world_size(group))]
        dist.all_gather(out, t, group=group)
        return [o.numpy().tobytes() for o in out]
    return fn


def create_group(m: int, n: int, nshards: int, device: int = 0) -> list[Engine]:
    """In-process emulation of an nshards-rank row-sharded job on one GPU."""
    lib = load()
    if device_count() <= device:
        raise EngineUnavailable("no GPU visible; the engine has no CPU fallback")
    hs = (_H * nshards)()
    st = lib.lp_create_group(m, n, device, nshards, hs)
    if st != PIVOTED:
        raise (ValueError if st == BAD_ARG else DeviceError)(lib.lp_last_error(None).decode())
    engines = [Engine(m, n, device, _handle=_H(hs[k])) for k in range(nshards)]
    # destroy in reverse order: shard 0 owns the shared stream
    for e in engines[1:]:
        e._keep = engines[0]
    return engines


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id (call on rank 0, broadcast to all ranks)."""
    buf = C.create_string_buffer(128)
    st = load().lp_comm_unique_id(buf)
    if st != PIVOTED:
        raise DeviceError(load().lp_last_error(None).decode())
    return buf.raw


def create_sharded(m: int, n: int, rank: int, nranks: int, uid: bytes,
                   device: int = 0) -> Engine:
    """One rank's shard of an nranks-process row-sharded tableau (RCCL)."""
    lib = load()
    if device_count() <= device:
        raise EngineUnavailable("no GPU visible; the engine has no CPU fallback")
    if uid is not None and len(uid) != 128:
        raise ValueError("uid must be the 128-byte RCCL unique id (or None: no RCCL)")
    h = _H()
    st = lib.lp_create_sharded(m, n, device, rank, nranks, uid, C.byref(h))
    if st != PIVOTED:
        raise (ValueError if st == BAD_ARG else DeviceError)(lib.lp_last_error(None).decode())
    return Engine(m, n, device, _handle=h)


BATCH_LDS_MAX = 160 * 1024


def batch_lds_bytes(m: int, n: int) -> int:
    """LDS one workgroup of the batch kernel needs for an m x n LP
    (lp_batch_create's formula): the tableau at an odd row pitch, the
    normalised pivot row, the multipliers and the reduction scratch."""
    pitch = (n + 1) | 1
    return ((m + 1) * pitch + pitch + (m + 1) + 16) * 8


def batch_max_m(n: int) -> int:
    """largest m the batch path takes at n columns (0: none)"""
    pitch = (n + 1) | 1
    return max(0, (BATCH_LDS_MAX // 8 - 16 - pitch) // (pitch + 1) - 1)


def batch_device_lds_bytes(m: int, n: int) -> int:
    """LDS one workgroup needs for a device-placed m x n LP
    (lp_placed_lds_bytes): the normalised pivot row, the multipliers and
    the reduction scratch; the tableau stays in device memory."""
    return ((n + 1) + (m + 1) + 16) * 8


def place_code(place) -> int:
    """"lds" | "auto" | "device" -> LP_PLACE_*"""
    if place not in PLACES:
        raise ValueError(f'place must be "lds", "auto" or "device", not {place!r}')
    return PLACES[place]


def placed_on_device(place: int, m: int, n: int) -> bool:
    """the placement rule (batch_plan.h: plan_place) for a shape that is valid"""
    return place == PLACE_DEVICE or (place == PLACE_AUTO and batch_lds_bytes(m, n) > BATCH_LDS_MAX)


def placed_too_large(place: int, m: int, n: int) -> bool:
    """the LP fits neither placement `place` allows"""
    if placed_on_device(place, m, n):
        return batch_device_lds_bytes(m, n) > BATCH_LDS_MAX
    return batch_lds_bytes(m, n) > BATCH_LDS_MAX


def place_hint(place: int, shapes) -> str:
    """what to add to a "too large" refusal under place="lds" when place="auto" would take every LP"""
    if place != PLACE_LDS or any(m <= 0 or n <= 0 for m, n in shapes):
        return ""
    if not any(placed_too_large(PLACE_LDS, m, n) for m, n in shapes):
        return ""
    if any(placed_too_large(PLACE_AUTO, m, n) for m, n in shapes):
        return ""
    return '; place="auto" solves such an LP from device memory'


def sense_codes(seq) -> np.ndarray:
    """ints 0..2 or the strings "<=", ">=", "==" -> int8 LP_SENSE_* codes"""
    out = []
    for s in seq:
        if isinstance(s, str):
            if s not in SENSES:
                raise ValueError(f'a sense must be "<=", ">=" or "==" (or 0, 1, 2), not {s!r}')
            out.append(SENSES[s])
        elif isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) <= 2:
            raise ValueError(f'a sense must be "<=", ">=" or "==" (or 0, 1, 2), not {s!r}')
        else:
            out.append(int(s))
    return np.array(out, dtype=np.int8)


def kind_codes(seq) -> np.ndarray:
    """ints 0..4 -> int8 LP_VAR_* codes"""
    out = []
    for k in seq:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= 4:
            raise ValueError(f"a kind must be VAR_PLAIN (0) to VAR_FREE (4), not {k!r}")
        out.append(int(k))
    return np.array(out, dtype=np.int8)


def team_code(team) -> int:
    """1 | G | "auto" -> the team request of lp_teamed_create (0: auto)"""
    if isinstance(team, str):
        if team != "auto":
            raise ValueError(f'team must be a positive int or "auto", not {team!r}')
        return 0
    if isinstance(team, bool) or not isinstance(team, (int, np.integer)) or team < 1:
        raise ValueError(f'team must be a positive int or "auto", not {team!r}')
    return int(team)


def _team_plan(engine) -> list:
    """lp_teamed_plan as one dict per teamed LP: lp, team, ranges [(e0, e1), ...] in rank order"""
    cnt = C.c_int64()
    engine._check(engine.lib.lp_teamed_plan(engine.h, None, 0, C.byref(cnt)), engine.h)
    rows = np.zeros((cnt.value, 5), dtype=np.int64)
    engine._check(engine.lib.lp_teamed_plan(engine.h, rows.ctypes.data_as(_P64), cnt.value, C.byref(cnt)), engine.h)
    out = []
    for lp, rank, g, e0, e1 in rows.tolist():
        if rank == 0:
            out.append(dict(lp=lp, team=g, ranges=[]))
        out[-1]["ranges"].append((e0, e1))
    return out


def twophase_lds_bytes(m: int, n: int) -> int:
    """LDS one workgroup of the two-phase kernel needs for an m x n LP
    (lp_twophase_lds_bytes): batch_lds_bytes at the pitch of the widest
    artificial problem, n + 1 + m columns, plus the basis (m int32)."""
    pitch = (n + 1 + m) | 1
    return ((m + 1) * pitch + pitch + (m + 1) + 16 + (m + 1) // 2) * 8


def twophase_max_m(n: int) -> int:
    """largest m lp_twophase_solve takes at n columns (0: none)"""
    m = 0
    while twophase_lds_bytes(m + 1, n) <= BATCH_LDS_MAX:
        m += 1
    return m


def twophase_waves(m: int, n: int) -> int:
    """waves per LP of the two-phase kernel: one up to 2048 widened elements"""
    return 1 if (m + 1) * (n + 1 + m) <= 2048 else 4


def phased_lds_bytes(m: int, n: int) -> int:
    """LDS one workgroup needs for a device-placed two-phase m x n LP
    (lp_phased_lds_bytes): the normalised pivot row at the widest live width
    n + 1 + m, the multipliers, the reduction scratch and the basis (m int32);
    the working tableau stays in device memory."""
    return ((n + 1 + m) + (m + 1) + 16 + (m + 1) // 2) * 8


def phased_on_device(place: int, m: int, n: int) -> bool:
    """the placement rule of the two-phase call (batch_plan.h:
    plan_place_phased) for a shape that is valid"""
    return place == PLACE_DEVICE or (place == PLACE_AUTO and twophase_lds_bytes(m, n) > BATCH_LDS_MAX)


def phased_too_large(place: int, m: int, n: int) -> bool:
    """the LP fits neither placement `place` allows the two-phase call"""
    if phased_on_device(place, m, n):
        return phased_lds_bytes(m, n) > BATCH_LDS_MAX
    return twophase_lds_bytes(m, n) > BATCH_LDS_MAX


class BatchEngine:
    """`count` device tableaux of one shape solved one workgroup per LP
    (an ``lp_batch``).  Thin, typed wrapper: every method is one C-ABI call.
    place: "lds" keeps each LP's tableau in a CU's LDS and refuses a shape
    that does not fit; "auto" keeps such a shape in device memory instead;
    "device" does so for every shape (lp_placed_create).
    team: workgroups per device-placed LP for solve() and run(): 1, a forced
    G, or "auto", which gives a small batch of large LPs several each
    (lp_teamed_create); the results are the same bits.
    No GPU, no engine: there is no host fallback."""

    def __init__(self, count: int, m: int, n: int, log_cap: int = 0, device: int = 0, place: str = "lds",
                 team=1):
        self.lib = load()
        self.count, self.m, self.n = int(count), int(m), int(n)
        self.log_cap, self.device = int(log_cap), device
        self.place = place_code(place)
        self.team = team_code(team)
        self.h = None
        self._tol = default_tol()
        h = _H()

        def create():
            if self.team != 1:
                return self.lib.lp_teamed_create(self.count, self.m, self.n, self.log_cap, device, self.place,
                                                 self.team, C.byref(h))
            return self.lib.lp_placed_create(self.count, self.m, self.n, self.log_cap, device, self.place,
                                                   C.byref(h))
        bad = (self.count <= 0 or self.m <= 0 or self.n <= 0 or self.log_cap < 0
               or placed_too_large(self.place, self.m, self.n))
        if bad:     # refused by the library before any device call: ValueError with or without a GPU
            self._check(create(), None, place_hint(self.place, [(self.m, self.n)]))
        st = create() if self.team > 1 else None        # a forced team the library refuses, likewise
        if st == BAD_ARG:
            self._check(st, None)
        if device_count() <= device:
            raise EngineUnavailable(
                f"no GPU {device} visible (lp_device_count = {device_count()}); "
                "the batch engine has no CPU fallback")
        self._check(create() if st is None else st, None)
        self.h = h

    # -- plumbing ---------------------------------------------------------
    def _check(self, st: int, h, hint: str = "") -> int:
        if st == BAD_ARG:
            raise ValueError(self._err(h) + hint)
        if st < 0:
            raise DeviceError(self._err(h) or f"status {STATUS_NAMES.get(st, st)}")
        return st

    def _err(self, h) -> str:
        msg = self.lib.lp_batch_last_error(h)
        return msg.decode() if msg else ""

    def close(self):
        if getattr(self, "h", None):
            self.lib.lp_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- settings -----------------------------------------------------------
    def set_tol(self, **kw):
        t = self._tol
        for k, v in kw.items():
            if not hasattr(t, k):
                raise KeyError(k)
            setattr(t, k, float(v))
        self._check(self.lib.lp_batch_set_tol(self.h, C.byref(t)), self.h)

    def placement(self, index: int) -> str:
        """"lds" or "device": where LP `index` is kept during a launch"""
        p = C.c_int()
        if self.lib.lp_placed_placement(self.h, int(index), C.byref(p)) != PIVOTED:
            raise ValueError("LP index out of bounds")
        return PLACE_NAMES[p.value]

    def team_of(self, index: int) -> int:
        """the workgroups that solve() / run() put on LP `index` (1: not teamed)"""
        g = C.c_int()
        if self.lib.lp_teamed_size(self.h, int(index), C.byref(g)) != PIVOTED:
            raise ValueError("LP index out of bounds")
        return g.value

    def team_plan(self) -> list:
        """the teamed LPs, ascending: dicts of lp, team and ranges, the
        (first, one past last) elements each workgroup of the team updates"""
        return _team_plan(self)

    def set_window(self, launches_per_readback: int):
        """launches of the teamed kernel, one pivot each, per read-back of
        the LPs' state (results do not depend on it)"""
        self._check(self.lib.lp_teamed_set_window(self.h, int(launches_per_readback)), self.h)

    def set_chunk(self, pivots_per_launch: int):
        """most pivots one launch runs per LP (results do not depend on it)"""
        self._check(self.lib.lp_batch_set_chunk(self.h, int(pivots_per_launch)), self.h)

    # -- data ---------------------------------------------------------------
    def upload(self, T: np.ndarray, first: int = 0):
        """tableaux [k, m+1, n+1] into LPs [first, first+k); resets their state"""
        a = np.ascontiguousarray(T, dtype=np.float64)
        if a.ndim != 3 or a.shape[1:] != (self.m + 1, self.n + 1):
            raise ValueError(f"tableaux must be (k, {self.m + 1}, {self.n + 1}) float64")
        self._check(self.lib.lp_batch_upload(self.h, first, a.shape[0], _ptr(a), self.n + 1), self.h)

    def download(self, first: int = 0, count: int | None = None) -> np.ndarray:
        k = self.count - first if count is None else count
        out = np.empty((max(k, 0), self.m + 1, self.n + 1), dtype=np.float64)
        self._check(self.lib.lp_batch_download(self.h, first, k, _ptr(out), self.n + 1), self.h)
        return out

    def set_basis(self, basis):
        """attach a [count, m] basis the pivots maintain (None detaches it)"""
        if basis is None:
            self._check(self.lib.lp_batch_set_basis(self.h, None), self.h)
            return
        a = np.ascontiguousarray(basis, dtype=np.int32)
        if a.shape != (self.count, self.m):
            raise ValueError(f"basis must be ({self.count}, {self.m})")
        self._check(self.lib.lp_batch_set_basis(self.h, a.ctypes.data_as(_P32)), self.h)

    def get_basis(self) -> np.ndarray:
        out = np.empty((self.count, self.m), dtype=np.int32)
        self._check(self.lib.lp_batch_get_basis(self.h, out.ctypes.data_as(_P32)), self.h)
        return out

    def objective(self) -> np.ndarray:
        z = np.empty(self.count, dtype=np.float64)
        self._check(self.lib.lp_batch_objective(self.h, _ptr(z)), self.h)
        return z

    # -- solutions on the device (lp_solution_canonical / lp_solution_gather) -----
    def _window(self, first: int, count):
        first = int(first)
        return first, (self.count - first if count is None else int(count))

    def _xsize(self, first: int, k: int) -> int:
        """doubles of the packed x of LPs [first, first+k)"""
        return max(k, 0) * self.n

    def derive_basis(self, first: int = 0, count: int | None = None):
        """Tableau.isCanonical's basic column per row of LPs [first,
        first+count), derived on the device from the tableaux as stored and
        attached as the basis (lp_solution_canonical) -> (flags int32 [count],
        first_bad): bit 0 of a flag, some b_r < 0; bit 1, a row without a
        basic column (its entry is -1); first_bad the first LP with a flag,
        or -1"""
        first, k = self._window(first, count)
        flags = np.zeros(max(k, 0), dtype=np.int32)
        bad = C.c_int64(-1)
        self._check(self.lib.lp_solution_canonical(self.h, first, k, flags.ctypes.data_as(_P32), C.byref(bad)), self.h)
        return flags, int(bad.value)

    def _solution(self, first, count, want_x, want_z):
        first, k = self._window(first, count)
        ok = 0 <= first <= self.count and 0 <= k <= self.count - first
        x = np.empty(self._xsize(first, k) if ok else 0, dtype=np.float64) if want_x else None
        z = np.empty(max(k, 0), dtype=np.float64) if want_z else None
        self._check(self.lib.lp_solution_gather(self.h, first, k, None if x is None else _ptr(x),
                                               None if z is None else _ptr(z)), self.h)
        return first, k, x, z

    def solution(self, first: int = 0, count: int | None = None, *, want_x: bool = True, want_z: bool = True):
        """Simplex.getBFS and getObjValue of LPs [first, first+count), gathered
        on the device from the stored tableaux and the attached basis
        (lp_solution_gather) -> (x [count, n], z [count]); None for one not
        wanted"""
        _, k, x, z = self._solution(first, count, want_x, want_z)
        return (None if x is None else x.reshape(k, self.n)), z

    # -- problem form (lp_problem_*) ------------------------------------------
    def set_senses(self, sense):
        """one sense per constraint row, shared by every LP: LP_SENSE_* codes
        or "<=", ">=", "==" (None detaches them)"""
        if sense is None:
            self._check(self.lib.lp_problem_set_senses(self.h, None), self.h)
            self._sense = None
            return
        a = np.ascontiguousarray(sense_codes(sense))
        if a.shape != (self.m,):
            raise ValueError(f"sense must hold {self.m} entries, one per row")
        self._check(self.lib.lp_problem_set_senses(self.h, a.ctypes.data_as(_P8)), self.h)
        self._sense = a             # kept for extend(), which joins the new rows' senses to them

    def nvars(self, index: int) -> int:
        """the structural variables of LP `index`: n less its slack columns"""
        ns = C.c_int64()
        if self.lib.lp_problem_vars(self.h, int(index), C.byref(ns)) != PIVOTED:
            raise ValueError("no senses attached (set_senses), or LP index out of bounds")
        return ns.value

    def upload_problems(self, P: np.ndarray, first: int = 0):
        """problem blocks [k, m+1, ns+1] into LPs [first, first+k): the
        tableaux are assembled on the device; resets those LPs' state"""
        a = np.ascontiguousarray(P, dtype=np.float64)
        ns = self.nvars(0)
        if a.ndim != 3 or a.shape[1:] != (self.m + 1, ns + 1):
            raise ValueError(f"problem blocks must be (k, {self.m + 1}, {ns + 1}) float64")
        self._check(self.lib.lp_problem_upload(self.h, int(first), a.shape[0], _ptr(a)), self.h)

    def _ysize(self, first: int, k: int) -> int:
        """doubles of the packed duals of LPs [first, first+k)"""
        return max(k, 0) * self.m

    def _duals(self, first, count):
        first, k = self._window(first, count)
        ok = 0 <= first <= self.count and 0 <= k <= self.count - first
        y = np.empty(self._ysize(first, k) if ok else 0, dtype=np.float64)
        self._check(self.lib.lp_problem_duals(self.h, first, k, _ptr(y)), self.h)
        return first, k, y

    def duals(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """the dual values of LPs [first, first+count) read on the device from
        row 0 of the stored tableaux (lp_problem_duals) -> [count, m]; NaN on
        an equality row"""
        _, k, y = self._duals(first, count)
        return y.reshape(k, self.m)

    # -- warm re-solves (lp_resolve_set_rhs) ----------------------------------
    def set_rhs(self, rhs, first: int = 0):
        """new right-hand sides [k, m+1] on the stored tableaux of LPs [first,
        first+k): rhs[:, 0] the stored _z cell, rhs[:, 1:] = b.  Column 0
        becomes what the pivots so far would have left of it; nothing else
        changes (lp_resolve_set_rhs).  run(RULE_DUAL, k) goes on from there"""
        a = np.ascontiguousarray(rhs, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.m + 1:
            raise ValueError(f"rhs must be (k, {self.m + 1}) float64")
        self._check(self.lib.lp_resolve_set_rhs(self.h, int(first), a.shape[0], _ptr(a)), self.h)

    # -- warm re-optimisation (lp_reopt_*) -------------------------------------
    def set_costs(self, costs, first: int = 0):
        """new cost rows [k, n+1] on the stored tableaux of LPs [first,
        first+k): costs[:, 0] the stored _z cell, costs[:, 1+j] the cost of
        tableau column j (+0.0 for a slack column).  Row 0 becomes the cost
        row less c_B times the rows of the attached basis; nothing else
        changes (lp_reopt_set_costs).  solve() goes on from there"""
        a = np.ascontiguousarray(costs, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.n + 1:
            raise ValueError(f"costs must be (k, {self.n + 1}) float64")
        self._check(self.lib.lp_reopt_set_costs(self.h, int(first), a.shape[0], _ptr(a)), self.h)

    def set_general(self, border, first: int = 0):
        """new borders [k, 3 ns + m + 1] of the general blocks of LPs [first,
        first+k): row 0 of P (-c0, then c), b, lb, ub.  The stored blocks, the
        shifted columns and column 0 of the stored tableaux follow
        (lp_reopt_set_general); a changed c needs set_costs before any run"""
        a = np.ascontiguousarray(border, dtype=np.float64)
        m, ns = self.general_vars(0)
        if a.ndim != 2 or a.shape[1] != 3 * ns + m + 1:
            raise ValueError(f"borders must be (k, {3 * ns + m + 1}) float64")
        self._check(self.lib.lp_reopt_set_general(self.h, int(first), a.shape[0], _ptr(a)), self.h)

    # -- warm cuts (lp_cut_extend) ---------------------------------------------
    def _lp_shapes(self) -> list:
        """(m_i, n_i) per LP, on either kind of engine"""
        return self.shapes if hasattr(self, "shapes") else [(self.m, self.n)] * self.count

    def _cut_items(self, rows, sense, first):
        """rows: k per-LP arrays (q_i, n_i + 1) -- a [k, q, n+1] array is such a
        sequence; sense: k per-LP sequences of q_i entries, or one flat
        sequence every LP shares -> (rows, int8 senses), checked"""
        items = [np.asarray(r, dtype=np.float64) for r in rows]
        k = len(items)
        if first < 0 or first + k > self.count:
            raise ValueError("LP range out of bounds")
        sense = [] if sense is None else list(sense)
        if not sense:
            senses = [np.zeros(0, dtype=np.int8)] * k
        elif isinstance(sense[0], (str, int, np.integer)):
            senses = [sense_codes(sense)] * k
        else:
            senses = [sense_codes(s) for s in sense]
        if len(senses) != k:
            raise ValueError("sense must hold one sequence per LP of rows, or one that every LP shares")
        shapes = self._lp_shapes()
        for j in range(k):
            n = shapes[first + j][1]
            if items[j].size == 0:
                items[j] = items[j].reshape(0, n + 1)
            if items[j].ndim != 2 or items[j].shape[1] != n + 1:
                raise ValueError(f"rows of LP {first + j} must be (q, {n + 1}) float64, not {items[j].shape}")
            if len(senses[j]) != items[j].shape[0]:
                raise ValueError(f"LP {first + j} has {items[j].shape[0]} rows and {len(senses[j])} senses")
        return items, senses

    def extend_into(self, dst, rows, sense, first: int = 0):
        """the stored tableaux of LPs [first, first+k) with q_i more rows each,
        written into engine `dst`, whose LP i is (m_i + q_i) x (n_i + q_i): the
        old tableau's bits, +0.0 under the new slack columns, and each stated
        row (beta, then one coefficient per tableau column) priced out against
        the rows of the attached basis; dst's basis is this one's followed by
        the new slacks (lp_cut_extend).  dst.run(RULE_DUAL, k) goes on from
        there.  This engine is not changed.  rows and sense as _cut_items takes
        them; "==" is refused"""
        first = int(first)
        items, senses = self._cut_items(rows, sense, first)
        mine, theirs = self._lp_shapes(), dst._lp_shapes()
        for j, a in enumerate(items):
            i = first + j
            q = theirs[i][0] - mine[i][0] if i < len(theirs) else -1
            if q >= 0 and a.shape[0] != q:
                raise ValueError(f"LP {i} of the destination has {q} more rows than the source's, not {a.shape[0]}")
        flat = np.ascontiguousarray(np.concatenate([a.ravel() for a in items]) if items else np.empty(0),
                                    dtype=np.float64)
        sflat = np.ascontiguousarray(np.concatenate(senses) if senses else np.empty(0), dtype=np.int8)
        self._check(self.lib.lp_cut_extend(self.h, dst.h, first, len(items), _ptr(flat) if flat.size else None,
                                           sflat.ctypes.data_as(_P8) if sflat.size else None), dst.h)

    def extend(self, rows, sense, *, log_cap=None, place=None, team=None):
        """a new engine that holds every LP of this one with the stated rows
        added (extend_into on a destination made here): uniform when this
        engine is and every LP gets the same number of rows -- and, where
        senses are attached, the same senses -- ragged otherwise.  It gets this
        engine's tolerances and, where this one has senses, the joined senses.
        log_cap, place, team: None keeps this engine's setting; a shape the
        placement refuses is the create call's ValueError"""
        items, senses = self._cut_items(rows, sense, 0)
        if len(items) != self.count:
            raise ValueError(f"rows must hold one array per LP, {self.count} of them")
        shapes = [(m + a.shape[0], n + a.shape[0]) for (m, n), a in zip(self._lp_shapes(), items)]
        mine = getattr(self, "_sense", None)
        same = all(np.array_equal(s, senses[0]) for s in senses)
        uniform = not hasattr(self, "shapes") and len(set(shapes)) == 1 and (mine is None or same)
        names = {v: k for k, v in PLACES.items()}
        place = names[self.place] if place is None else place
        log_cap = self.log_cap if log_cap is None else log_cap
        if team is None:
            one = (lambda t: "auto" if t == 0 else t)
            team = [one(t) for t in self.team] if isinstance(self.team, list) else one(self.team)
        if uniform:
            dst = BatchEngine(self.count, *shapes[0], log_cap=log_cap, device=self.device, place=place, team=team)
        else:
            dst = RaggedEngine(shapes, log_cap=log_cap, device=self.device, place=place, team=team)
        dst.set_tol(**self._tol.as_dict())
        if mine is not None:
            if uniform:
                dst.set_senses(np.concatenate([mine, senses[0]]))
            else:
                each = mine if isinstance(mine, list) else [mine] * self.count
                dst.set_senses([np.concatenate([a, b]) for a, b in zip(each, senses)])
        self.extend_into(dst, items, senses)
        return dst

    # -- general form (lp_general_*) ------------------------------------------
    def set_form(self, sense, kind=None, maximise=False):
        """the form every LP shares: m senses, ns kinds (VAR_*) and the
        direction; the batch's (m, n) must be lp_general_rows / _columns of
        them (None detaches the form)"""
        if sense is None:
            self._check(self.lib.lp_general_set_form(self.h, None, None, None, None, None), self.h)
            return
        if kind is None:
            raise ValueError("kind must hold one VAR_* code per variable")
        s = np.ascontiguousarray(sense_codes(sense))
        k = np.ascontiguousarray(kind_codes(kind))
        dims = np.array([len(s), len(k)], dtype=np.int64)
        mx = np.array([1 if maximise else 0], dtype=np.int8)
        self._check(self.lib.lp_general_set_form(self.h, dims[:1].ctypes.data_as(_P64), dims[1:].ctypes.data_as(_P64),
                                                 s.ctypes.data_as(_P8), k.ctypes.data_as(_P8),
                                                 mx.ctypes.data_as(_P8)), self.h)

    def general_vars(self, index: int):
        """(m, ns) of LP `index` as the caller states it"""
        m, ns = C.c_int64(), C.c_int64()
        if self.lib.lp_general_vars(self.h, int(index), C.byref(m), C.byref(ns)) != PIVOTED:
            raise ValueError("no form attached (set_form), or LP index out of bounds")
        return m.value, ns.value

    def upload_general(self, G: np.ndarray, first: int = 0):
        """general blocks [k, (m+1)(ns+1) + 2 ns] (problem.pack_general) into
        LPs [first, first+k): shifted, assembled into standard-form tableaux
        on the device; resets those LPs' state"""
        a = np.ascontiguousarray(G, dtype=np.float64)
        m, ns = self.general_vars(0)
        if a.ndim != 2 or a.shape[1] != (m + 1) * (ns + 1) + 2 * ns:
            raise ValueError(f"general blocks must be (k, {(m + 1) * (ns + 1) + 2 * ns}) float64")
        self._check(self.lib.lp_general_upload(self.h, int(first), a.shape[0], _ptr(a)), self.h)

    def _general_sizes(self, first: int, k: int):
        """doubles of the packed caller rows and variables of LPs [first, first+k)"""
        m, ns = self.general_vars(0)
        return max(k, 0) * m, max(k, 0) * ns

    def _general(self, call, first, count, want_a, want_b, per_lp_b):
        first, k = self._window(first, count)
        ok = 0 <= first <= self.count and 0 <= k <= self.count - first
        ny, nv = self._general_sizes(first, k) if ok else (0, 0)
        a = np.empty(ny if per_lp_b else nv, dtype=np.float64) if want_a else None
        b = np.empty(nv if per_lp_b else max(k, 0), dtype=np.float64) if want_b else None
        self._check(call(self.h, first, k, None if a is None else _ptr(a), None if b is None else _ptr(b)), self.h)
        return first, k, a, b

    def general_solution(self, first: int = 0, count: int | None = None, *, want_x: bool = True,
                         want_z: bool = True):
        """x and the objective of LPs [first, first+count) in the caller's
        variables (lp_general_solution) -> (x [count, ns], z [count])"""
        _, k, x, z = self._general(self.lib.lp_general_solution, first, count, want_x, want_z, False)
        return (None if x is None else x.reshape(k, self.general_vars(0)[1])), z

    def general_duals(self, first: int = 0, count: int | None = None, *, want_y: bool = True, want_r: bool = True):
        """the duals of the m caller rows and the reduced costs of the ns
        caller variables (lp_general_duals) -> (y [count, m], r [count, ns])"""
        _, k, y, r = self._general(self.lib.lp_general_duals, first, count, want_y, want_r, True)
        m, ns = self.general_vars(0)
        return (None if y is None else y.reshape(k, m)), (None if r is None else r.reshape(k, ns))

    # -- pivots -------------------------------------------------------------
    def solve(self, max_pivots: int = -1):
        """Simplex.solve per LP -> (status[count], npiv[count], nstd[count])"""
        st = np.empty(self.count, dtype=np.int32)
        a = np.empty(self.count, dtype=np.int64)
        b = np.empty(self.count, dtype=np.int64)
        self._check(self.lib.lp_batch_solve(self.h, max_pivots, st.ctypes.data_as(_P32),
                                            a.ctypes.data_as(_P64), b.ctypes.data_as(_P64)), self.h)
        return st, a, b

    def solve_lp(self, max_pivots: int = -1):
        """Simplex(t) + solve() per LP, phase 1 included (lp_twophase_solve)
        -> (status, stage, rows, ninit, npiv, nstd), each [count]"""
        st = np.empty(self.count, dtype=np.int32)
        sg = np.empty(self.count, dtype=np.int32)
        o = [np.empty(self.count, dtype=np.int64) for _ in range(4)]
        self._check(self.lib.lp_twophase_solve(self.h, max_pivots, st.ctypes.data_as(_P32),
                                               sg.ctypes.data_as(_P32),
                                               *[a.ctypes.data_as(_P64) for a in o]), self.h)
        return (st, sg, *o)

    def solve_lp_placed(self, max_pivots: int = -1):
        """solve_lp with each LP placed under the engine's `place`
        (lp_phased_solve): an LP whose widened tableau does not fit a CU's
        LDS runs both phases from device memory -> solve_lp's six arrays"""
        st = np.empty(self.count, dtype=np.int32)
        sg = np.empty(self.count, dtype=np.int32)
        o = [np.empty(self.count, dtype=np.int64) for _ in range(4)]
        self._check(self.lib.lp_phased_solve(self.h, max_pivots, st.ctypes.data_as(_P32),
                                             sg.ctypes.data_as(_P32),
                                             *[a.ctypes.data_as(_P64) for a in o]), self.h)
        return (st, sg, *o)

    def phased_placement(self, index: int) -> str:
        """"lds" or "device": where solve_lp_placed runs LP `index`"""
        p = C.c_int()
        if self.lib.lp_phased_placement(self.h, int(index), C.byref(p)) != PIVOTED:
            raise ValueError("LP index out of bounds, or the LP is too large for the two-phase batch path")
        return PLACE_NAMES[p.value]

    def plan_phased(self) -> list:
        """the launch bins of the next solve_lp_placed(), in launch order, as
        RaggedEngine.plan gives them; the device-placed LPs are one bin, first"""
        cnt = C.c_int64()
        self._check(self.lib.lp_phased_plan(self.h, None, 0, C.byref(cnt)), self.h)
        out = np.zeros((cnt.value, 4), dtype=np.int64)
        self._check(self.lib.lp_phased_plan(self.h, out.ctypes.data_as(_P64), cnt.value, C.byref(cnt)), self.h)
        return [dict(waves=int(r[0]), lds_bytes=int(r[1]), lps=int(r[2]), lps_per_cu=int(r[3])) for r in out]

    def run(self, rule: int, k: int):
        """k pivots of one rule per LP -> (status[count], done[count]).  rule:
        RULE_STANDARD, RULE_MIN_INDEX, RULE_MAX_INCREASE or RULE_DUAL; the last
        two are refused (ValueError) on a batch in which some LP has a team
        above 1"""
        st = np.empty(self.count, dtype=np.int32)
        d = np.empty(self.count, dtype=np.int64)
        self._check(self.lib.lp_batch_run(self.h, rule, k, st.ctypes.data_as(_P32),
                                          d.ctypes.data_as(_P64)), self.h)
        return st, d

    def log(self, index: int) -> np.ndarray:
        """the kept (r, c) pairs of LP `index` from the last solve / run"""
        cnt = C.c_int64()
        self._check(self.lib.lp_batch_log(self.h, index, None, 0, C.byref(cnt)), self.h)
        k = min(cnt.value, self.log_cap)
        out = np.zeros((k, 2), dtype=np.int64)
        if k:
            self._check(self.lib.lp_batch_log(self.h, index, out.ctypes.data_as(_P64), k,
                                              C.byref(cnt)), self.h)
        return out


class RaggedEngine(BatchEngine):
    """An ``lp_batch`` of LPs of different shapes (lp_ragged_create): LP i is
    shapes[i] = (m_i, n_i).  The solves, the settings, objective() and log()
    are BatchEngine's own -- the same C calls on the same handle; the data
    calls take and return lists of per-LP arrays (lp_ragged_*: the packed
    layout).  team: as BatchEngine's, or one request per LP.
    No GPU, no engine: there is no host fallback."""

    def __init__(self, shapes, log_cap: int = 0, device: int = 0, place: str = "lds", team=1):
        self.lib = load()
        self.shapes = [(int(m), int(n)) for m, n in shapes]
        self.count = len(self.shapes)
        self.log_cap, self.device = int(log_cap), device
        self.place = place_code(place)
        if isinstance(team, (list, tuple, np.ndarray)):
            if len(team) != self.count:
                raise ValueError("team must hold one request per LP")
            teams = np.array([team_code(t) for t in team], dtype=np.int32)
        else:
            teams = np.full(self.count, team_code(team), dtype=np.int32)
        self.team = teams.tolist()
        self.h = None
        self._tol = default_tol()
        ms = np.array([s[0] for s in self.shapes], dtype=np.int64)
        ns = np.array([s[1] for s in self.shapes], dtype=np.int64)
        h = _H()

        def create():
            if bool((teams != 1).any()):
                return self.lib.lp_teamed_create_ragged(self.count, ms.ctypes.data_as(_P64), ns.ctypes.data_as(_P64),
                                                        self.log_cap, device, self.place,
                                                        teams.ctypes.data_as(_P32), C.byref(h))
            return self.lib.lp_placed_create_ragged(self.count, ms.ctypes.data_as(_P64), ns.ctypes.data_as(_P64),
                                                    self.log_cap, device, self.place, C.byref(h))
        bad = (self.count <= 0 or self.log_cap < 0 or bool((ms <= 0).any()) or bool((ns <= 0).any())
               or any(placed_too_large(self.place, m, n) for m, n in self.shapes))
        if bad:     # refused by the library before any device call: ValueError with or without a GPU
            self._check(create(), None, place_hint(self.place, self.shapes))
        st = create() if bool((teams > 1).any()) else None      # a forced team the library refuses, likewise
        if st == BAD_ARG:
            self._check(st, None)
        if device_count() <= device:
            raise EngineUnavailable(
                f"no GPU {device} visible (lp_device_count = {device_count()}); "
                "the batch engine has no CPU fallback")
        self._check(create() if st is None else st, None)
        self.h = h
        self._sizes = [(m + 1) * (n + 1) for m, n in self.shapes]
        self._toff = np.concatenate([[0], np.cumsum(self._sizes)]).astype(np.int64)
        self._boff = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
        self._coff = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)

    # -- data ---------------------------------------------------------------
    def upload(self, tableaux, first: int = 0):
        """tableaux: k arrays, the i-th (m+1, n+1) of LP first + i; resets
        those LPs' state"""
        items = [np.asarray(t, dtype=np.float64) for t in tableaux]
        if first < 0 or first + len(items) > self.count:
            raise ValueError("LP range out of bounds")
        for k, a in enumerate(items):
            m, n = self.shapes[first + k]
            if a.shape != (m + 1, n + 1):
                raise ValueError(f"tableau of LP {first + k} must be ({m + 1}, {n + 1}), not {a.shape}")
        flat = (np.concatenate([a.ravel() for a in items]) if items else np.empty(0))
        flat = np.ascontiguousarray(flat, dtype=np.float64)
        self._check(self.lib.lp_ragged_upload(self.h, first, len(items), _ptr(flat)), self.h)

    def download(self, first: int = 0, count: int | None = None) -> list:
        k = self.count - first if count is None else count
        if first < 0 or k < 0 or first + k > self.count:
            raise ValueError("LP range out of bounds")
        flat = np.empty(int(self._toff[first + k] - self._toff[first]), dtype=np.float64)
        self._check(self.lib.lp_ragged_download(self.h, first, k, _ptr(flat)), self.h)
        at = self._toff[first:first + k + 1] - self._toff[first]
        return [flat[at[i]:at[i + 1]].reshape(self.shapes[first + i][0] + 1, self.shapes[first + i][1] + 1)
                for i in range(k)]

    def set_basis(self, basis):
        """attach per-LP bases (a list, the i-th of m_i entries) the pivots
        maintain (None detaches them)"""
        if basis is None:
            self._check(self.lib.lp_ragged_set_basis(self.h, None), self.h)
            return
        items = [np.asarray(b, dtype=np.int32).ravel() for b in basis]
        if len(items) != self.count or any(len(b) != s[0] for b, s in zip(items, self.shapes)):
            raise ValueError("basis must hold one array of m_i entries per LP")
        flat = np.ascontiguousarray(np.concatenate(items), dtype=np.int32)
        self._check(self.lib.lp_ragged_set_basis(self.h, flat.ctypes.data_as(_P32)), self.h)

    def get_basis(self) -> list:
        flat = np.empty(int(self._boff[-1]), dtype=np.int32)
        self._check(self.lib.lp_ragged_get_basis(self.h, flat.ctypes.data_as(_P32)), self.h)
        return [flat[self._boff[i]:self._boff[i + 1]] for i in range(self.count)]

    def _xsize(self, first: int, k: int) -> int:
        return int(self._coff[first + k] - self._coff[first])

    def solution(self, first: int = 0, count: int | None = None, *, want_x: bool = True, want_z: bool = True):
        """BatchEngine.solution with x as a list of per-LP arrays (n_i each)"""
        first, k, x, z = self._solution(first, count, want_x, want_z)
        if x is None:
            return None, z
        at = self._coff[first:first + k + 1] - self._coff[first]
        return [x[at[i]:at[i + 1]] for i in range(k)], z

    # -- problem form (lp_problem_*) ------------------------------------------
    def set_senses(self, sense):
        """per-LP senses: a list, the i-th of m_i entries (None detaches them)"""
        if sense is None:
            self._check(self.lib.lp_problem_set_senses(self.h, None), self.h)
            self._sense = None
            return
        items = [sense_codes(s) for s in sense]
        if len(items) != self.count or any(len(s) != sh[0] for s, sh in zip(items, self.shapes)):
            raise ValueError("sense must hold one sequence of m_i entries per LP")
        flat = np.ascontiguousarray(np.concatenate(items), dtype=np.int8)
        self._check(self.lib.lp_problem_set_senses(self.h, flat.ctypes.data_as(_P8)), self.h)
        self._sense = items

    def upload_problems(self, problems, first: int = 0):
        """problems: k arrays, the i-th the (m+1, ns+1) block of LP first + i"""
        items = [np.asarray(p, dtype=np.float64) for p in problems]
        if first < 0 or first + len(items) > self.count:
            raise ValueError("LP range out of bounds")
        for k, a in enumerate(items):
            m, ns = self.shapes[first + k][0], self.nvars(first + k)
            if a.shape != (m + 1, ns + 1):
                raise ValueError(f"problem block of LP {first + k} must be ({m + 1}, {ns + 1}), not {a.shape}")
        flat = (np.concatenate([a.ravel() for a in items]) if items else np.empty(0))
        flat = np.ascontiguousarray(flat, dtype=np.float64)
        self._check(self.lib.lp_problem_upload(self.h, int(first), len(items), _ptr(flat)), self.h)

    def _ysize(self, first: int, k: int) -> int:
        return int(self._boff[first + k] - self._boff[first])

    def duals(self, first: int = 0, count: int | None = None) -> list:
        """BatchEngine.duals as a list of per-LP arrays (m_i each)"""
        first, k, y = self._duals(first, count)
        at = self._boff[first:first + k + 1] - self._boff[first]
        return [y[at[i]:at[i + 1]] for i in range(k)]

    # -- warm re-solves (lp_resolve_set_rhs) ----------------------------------
    def set_rhs(self, rhs, first: int = 0):
        """BatchEngine.set_rhs with rhs a list, the i-th the m_i + 1 new
        values of LP first + i"""
        items = [np.asarray(r, dtype=np.float64).ravel() for r in rhs]
        if first < 0 or first + len(items) > self.count:
            raise ValueError("LP range out of bounds")
        for k, a in enumerate(items):
            m = self.shapes[first + k][0]
            if len(a) != m + 1:
                raise ValueError(f"rhs of LP {first + k} must hold {m + 1} values, not {len(a)}")
        flat = np.ascontiguousarray(np.concatenate(items) if items else np.empty(0), dtype=np.float64)
        self._check(self.lib.lp_resolve_set_rhs(self.h, int(first), len(items), _ptr(flat)), self.h)

    # -- warm re-optimisation (lp_reopt_*) -------------------------------------
    def _packed(self, items, first, size, what):
        """k per-LP arrays, the i-th of size(first + i) doubles -> one flat array"""
        items = [np.asarray(a, dtype=np.float64).ravel() for a in items]
        if first < 0 or first + len(items) > self.count:
            raise ValueError("LP range out of bounds")
        for k, a in enumerate(items):
            if len(a) != size(first + k):
                raise ValueError(f"{what} of LP {first + k} must hold {size(first + k)} values, not {len(a)}")
        return len(items), np.ascontiguousarray(np.concatenate(items) if items else np.empty(0), dtype=np.float64)

    def set_costs(self, costs, first: int = 0):
        """BatchEngine.set_costs with costs a list, the i-th the n_i + 1 new
        values of LP first + i"""
        k, flat = self._packed(costs, first, lambda i: self.shapes[i][1] + 1, "costs")
        self._check(self.lib.lp_reopt_set_costs(self.h, int(first), k, _ptr(flat)), self.h)

    def set_general(self, border, first: int = 0):
        """BatchEngine.set_general with border a list, the i-th the
        3 ns_i + m_i + 1 doubles of LP first + i"""
        def size(i):
            m, ns = self.general_vars(i)
            return 3 * ns + m + 1
        k, flat = self._packed(border, first, size, "border")
        self._check(self.lib.lp_reopt_set_general(self.h, int(first), k, _ptr(flat)), self.h)

    # -- general form (lp_general_*) ------------------------------------------
    def set_form(self, sense, kind=None, maximise=None):
        """per-LP forms: lists of m_i senses, of ns_i kinds and of directions
        (None detaches the form)"""
        if sense is None:
            self._check(self.lib.lp_general_set_form(self.h, None, None, None, None, None), self.h)
            return
        if kind is None:
            raise ValueError("kind must hold one sequence of VAR_* codes per LP")
        ss = [sense_codes(s) for s in sense]
        ks = [kind_codes(k) for k in kind]
        mx = [False] * self.count if maximise is None else list(maximise)
        if not (len(ss) == len(ks) == len(mx) == self.count):
            raise ValueError("sense, kind and maximise must hold one entry per LP")
        ms = np.array([len(s) for s in ss], dtype=np.int64)
        nss = np.array([len(k) for k in ks], dtype=np.int64)
        s = np.ascontiguousarray(np.concatenate(ss), dtype=np.int8)
        k = np.ascontiguousarray(np.concatenate(ks), dtype=np.int8)
        d = np.array([1 if v else 0 for v in mx], dtype=np.int8)
        self._check(self.lib.lp_general_set_form(self.h, ms.ctypes.data_as(_P64), nss.ctypes.data_as(_P64),
                                                 s.ctypes.data_as(_P8), k.ctypes.data_as(_P8),
                                                 d.ctypes.data_as(_P8)), self.h)
        self._gm = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
        self._gv = np.concatenate([[0], np.cumsum(nss)]).astype(np.int64)

    def upload_general(self, blocks, first: int = 0):
        """blocks: k flat arrays, the i-th the general block of LP first + i"""
        items = [np.asarray(g, dtype=np.float64).ravel() for g in blocks]
        if first < 0 or first + len(items) > self.count:
            raise ValueError("LP range out of bounds")
        for k, a in enumerate(items):
            m, ns = self.general_vars(first + k)
            if a.size != (m + 1) * (ns + 1) + 2 * ns:
                raise ValueError(f"general block of LP {first + k} must hold {(m + 1) * (ns + 1) + 2 * ns} doubles, "
                                 f"not {a.size}")
        flat = np.ascontiguousarray(np.concatenate(items) if items else np.empty(0), dtype=np.float64)
        self._check(self.lib.lp_general_upload(self.h, int(first), len(items), _ptr(flat)), self.h)

    def _general_sizes(self, first: int, k: int):
        self.general_vars(0)        # ValueError without a form
        return int(self._gm[first + k] - self._gm[first]), int(self._gv[first + k] - self._gv[first])

    def _cut(self, flat, off, first, k):
        at = off[first:first + k + 1] - off[first]
        return [flat[at[i]:at[i + 1]] for i in range(k)]

    def general_solution(self, first: int = 0, count: int | None = None, *, want_x: bool = True,
                         want_z: bool = True):
        """BatchEngine.general_solution with x as a list of per-LP arrays (ns_i each)"""
        first, k, x, z = self._general(self.lib.lp_general_solution, first, count, want_x, want_z, False)
        return (None if x is None else self._cut(x, self._gv, first, k)), z

    def general_duals(self, first: int = 0, count: int | None = None, *, want_y: bool = True, want_r: bool = True):
        """BatchEngine.general_duals as lists of per-LP arrays (m_i and ns_i each)"""
        first, k, y, r = self._general(self.lib.lp_general_duals, first, count, want_y, want_r, True)
        return (None if y is None else self._cut(y, self._gm, first, k),
                None if r is None else self._cut(r, self._gv, first, k))

    def plan(self, twophase: bool = False) -> list:
        """the launch bins of the next solve() / run() (or solve_lp()), in
        launch order: dicts of waves, lds_bytes, lps, lps_per_cu"""
        return ragged_plan(self, twophase)


def ragged_plan(engine, twophase: bool = False) -> list:
    """lp_ragged_plan of a BatchEngine or RaggedEngine"""
    cnt = C.c_int64()
    engine._check(engine.lib.lp_ragged_plan(engine.h, int(bool(twophase)), None, 0, C.byref(cnt)), engine.h)
    out = np.zeros((cnt.value, 4), dtype=np.int64)
    engine._check(engine.lib.lp_ragged_plan(engine.h, int(bool(twophase)), out.ctypes.data_as(_P64), cnt.value,
                                            C.byref(cnt)), engine.h)
    return [dict(waves=int(r[0]), lds_bytes=int(r[1]), lps=int(r[2]), lps_per_cu=int(r[3])) for r in out]
