"""Batched solve: the parts of the C-ABI and the front-end that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import lpsol_amd
from lpsol_amd import Tableau, _lib, solve_batch
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis

BATCH_SYMBOLS = {
    "lp_batch_create", "lp_batch_destroy", "lp_batch_set_tol", "lp_batch_set_chunk",
    "lp_batch_upload", "lp_batch_download", "lp_batch_set_basis", "lp_batch_get_basis",
    "lp_batch_solve", "lp_batch_run", "lp_batch_objective", "lp_batch_log",
    "lp_batch_last_error",
}


def test_batch_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "lpgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lp_batch_\w+)\s*\(", text))
    assert declared == BATCH_SYMBOLS
    assert BATCH_SYMBOLS <= set(_lib.EXPORTS)
    for name in BATCH_SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    assert {"solve_batch", "BatchResult", "BatchEngine"} <= set(lpsol_amd.__all__)


@pytest.mark.parametrize("count,m,n,log_cap", [(0, 8, 18, 0), (4, 0, 18, 0), (4, 8, -1, 0),
                                                (4, 8, 18, -1)])
def test_batch_create_rejects_bad_arguments_without_a_device(count, m, n, log_cap):
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    # device 1 << 20 does not exist anywhere: the refusal comes before any device call
    assert lib.lp_batch_create(count, m, n, log_cap, 1 << 20, ctypes.byref(h)) == _lib.BAD_ARG
    assert not h.value
    assert b"count > 0" in lib.lp_batch_last_error(None)


def test_batch_create_rejects_a_shape_beyond_one_cu():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.lp_batch_create(4, 200, 400, 0, 1 << 20, ctypes.byref(h)) == _lib.BAD_ARG
    assert b"too large" in lib.lp_batch_last_error(None)
    # the boundary is the documented LDS formula
    n = 128
    mmax = _lib.batch_max_m(n)
    assert _lib.batch_lds_bytes(mmax, n) <= _lib.BATCH_LDS_MAX < _lib.batch_lds_bytes(mmax + 1, n)
    assert lib.lp_batch_create(1, mmax + 1, n, 0, 1 << 20, ctypes.byref(h)) == _lib.BAD_ARG
    assert lib.lp_batch_create(1, mmax, n, 0, 1 << 20, ctypes.byref(h)) == _lib.DEVICE_ERROR
    with pytest.raises(ValueError, match="too large"):
        _lib.BatchEngine(4, 200, 400)


def test_null_batch_is_refused():
    lib = _lib.load()
    assert lib.lp_batch_destroy(None) == _lib.BAD_ARG
    assert lib.lp_batch_set_chunk(None, 4) == _lib.BAD_ARG
    assert lib.lp_batch_solve(None, -1, None, None, None) == _lib.BAD_ARG
    assert lib.lp_batch_run(None, 0, 1, None, None) == _lib.BAD_ARG
    assert lib.lp_batch_log(None, 0, None, 0, None) == _lib.BAD_ARG


def test_canonical_basis_matches_isCanonical():
    stack = np.stack([gen.tableau("mixed", 8, 10, s) for s in (1, 2, 3)])
    # a repeated unit column: the first one wins the row, as in Tableau.isCanonical
    stack[1, :, 3] = stack[1, :, 11 + 2]
    got = canonical_basis(stack)
    for i in range(3):
        bc = [0] * 8
        assert Tableau.fromArray(stack[i]).isCanonical(bc)
        assert got[i].tolist() == bc
    assert got[1, 2] == 2


def test_mixed_stack_is_the_generator_for_every_seed():
    seeds = [1, 2, 77, 12289, 1 << 40]
    for m, ns in ((8, 10), (40, 40), (1, 1)):
        stack = gen.mixed_stack(m, ns, seeds)
        for k, s in enumerate(seeds):
            assert np.array_equal(stack[k], gen.tableau("mixed", m, ns, s)), (m, ns, s)


def test_solve_batch_rejects_ragged_and_non_canonical_input():
    a = gen.tableau("mixed", 8, 10, 1)
    b = gen.tableau("mixed", 16, 16, 11)
    with pytest.raises(ValueError, match="same shape"):
        solve_batch([a, b])
    with pytest.raises(ValueError, match="same shape"):
        solve_batch([Tableau.fromArray(a), Tableau.fromArray(b)])
    stack = np.stack([gen.tableau("mixed", 8, 10, s) for s in (1, 2, 3)])
    stack[2, 4, 0] = -1.0                       # b_3 < 0
    with pytest.raises(ValueError, match="LP 2 "):
        solve_batch(stack)
    stack = np.stack([gen.tableau("mixed", 8, 10, s) for s in (1, 2, 3)])
    stack[1, 5, 11 + 4] = 2.0                   # row 4 loses its unit column
    with pytest.raises(ValueError, match="LP 1 "):
        solve_batch(stack)
    with pytest.raises(ValueError, match="rule and steps"):
        solve_batch(stack[:1], rule=_lib.RULE_MIN_INDEX)


def test_solve_batch_has_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    stack = np.stack([gen.tableau("mixed", 8, 10, s) for s in (1, 2)])
    with pytest.raises(_lib.EngineUnavailable):
        solve_batch(stack)
    with pytest.raises(_lib.EngineUnavailable):
        _lib.BatchEngine(2, 8, 18)
