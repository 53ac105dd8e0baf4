"""Ragged batches (lp_ragged_*, solve_ragged, solve_lp_ragged): the parts of
the C-ABI and the front-end that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import lpsol_amd
from lpsol_amd import Tableau, _lib, solve_batch, solve_lp_batch, solve_lp_ragged, solve_ragged
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis, ragged_canonical_basis

RAGGED_SYMBOLS = {
    "lp_ragged_create", "lp_ragged_shape", "lp_ragged_upload", "lp_ragged_download",
    "lp_ragged_set_basis", "lp_ragged_get_basis", "lp_ragged_plan",
}
BATCH_SYMBOLS = {
    "lp_batch_create", "lp_batch_destroy", "lp_batch_set_tol", "lp_batch_set_chunk",
    "lp_batch_upload", "lp_batch_download", "lp_batch_set_basis", "lp_batch_get_basis",
    "lp_batch_solve", "lp_batch_run", "lp_batch_objective", "lp_batch_log",
    "lp_batch_last_error",
}
TWOPHASE_SYMBOLS = {"lp_twophase_lds_bytes", "lp_twophase_solve"}
NO_DEVICE = 1 << 20         # exists nowhere: a refusal with it comes before any device call


def declared(prefix):
    text = open(os.path.join(ROOT, "include", "lpgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", text))


def test_ragged_symbols_declared_exported_and_bound():
    lib = _lib.load()
    assert declared("lp_ragged_") == RAGGED_SYMBOLS
    assert RAGGED_SYMBOLS <= set(_lib.EXPORTS)
    for name in RAGGED_SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    # the existing families are what they were
    assert declared("lp_batch_") == BATCH_SYMBOLS
    assert declared("lp_twophase_") == TWOPHASE_SYMBOLS
    assert {"solve_ragged", "solve_lp_ragged", "RaggedResult", "LPRaggedResult"} <= set(lpsol_amd.__all__)
    assert hasattr(_lib, "RaggedEngine")


def create(ms, ns, log_cap=0, count=None, null=None):
    lib = _lib.load()
    m = np.array(ms, dtype=np.int64)
    n = np.array(ns, dtype=np.int64)
    h = ctypes.c_void_p(1)
    pm = None if null == "m" else m.ctypes.data_as(_lib._P64)
    pn = None if null == "n" else n.ctypes.data_as(_lib._P64)
    st = lib.lp_ragged_create(len(ms) if count is None else count, pm, pn, log_cap, NO_DEVICE, ctypes.byref(h))
    return st, h.value, lib.lp_batch_last_error(None).decode()


@pytest.mark.parametrize("kw", [dict(count=0), dict(count=-3), dict(null="m"), dict(null="n"),
                                dict(log_cap=-1)])
def test_create_rejects_bad_arguments_without_a_device(kw):
    st, h, msg = create([8, 16], [18, 32], **kw)
    assert st == _lib.BAD_ARG and not h
    assert "count > 0" in msg


@pytest.mark.parametrize("ms,ns,index", [([8, 0, 4], [18, 3, 5], 1), ([8, 4, 4], [18, 3, -1], 2),
                                          ([-1, 0], [1, 1], 0)])
def test_create_names_the_lp_with_a_bad_shape(ms, ns, index):
    st, h, msg = create(ms, ns)
    assert st == _lib.BAD_ARG and not h
    assert f"LP {index}:" in msg


def test_create_rejects_an_lp_beyond_one_cu_and_names_it():
    n = 128
    mmax = _lib.batch_max_m(n)
    assert _lib.batch_lds_bytes(mmax, n) <= _lib.BATCH_LDS_MAX < _lib.batch_lds_bytes(mmax + 1, n)
    st, h, msg = create([1, mmax, mmax + 1, 200], [1, n, n, 400])
    assert st == _lib.BAD_ARG and not h
    assert "too large" in msg and "LP 2 " in msg
    st, h, msg = create([1 << 21], [4])
    assert st == _lib.BAD_ARG and "too large" in msg and "LP 0 " in msg
    # the largest shape passes the argument checks and reaches the device
    st, h, msg = create([1, mmax], [1, n])
    assert st == _lib.DEVICE_ERROR and not h
    with pytest.raises(ValueError, match="too large"):
        _lib.RaggedEngine([(1, 1), (mmax + 1, n)])
    with pytest.raises(ValueError, match="LP 1:"):
        _lib.RaggedEngine([(1, 1), (0, n)])
    with pytest.raises(ValueError):
        _lib.RaggedEngine([])


def test_valid_arguments_reach_the_device():
    st, h, msg = create([8, 16, 40], [18, 32, 80], log_cap=16)
    assert st == _lib.DEVICE_ERROR and not h and msg
    lib = _lib.load()
    assert lib.lp_ragged_create(1, None, None, 0, NO_DEVICE, None) == _lib.BAD_ARG       # out is NULL


def test_null_batch_is_refused():
    lib = _lib.load()
    assert lib.lp_ragged_shape(None, 0, None, None) == _lib.BAD_ARG
    assert lib.lp_ragged_upload(None, 0, 0, None) == _lib.BAD_ARG
    assert lib.lp_ragged_download(None, 0, 0, None) == _lib.BAD_ARG
    assert lib.lp_ragged_set_basis(None, None) == _lib.BAD_ARG
    assert lib.lp_ragged_get_basis(None, None) == _lib.BAD_ARG
    assert lib.lp_ragged_plan(None, 0, None, 0, None) == _lib.BAD_ARG


def test_ragged_canonical_basis_per_shape_group():
    lps = [gen.tableau("mixed", 8, 10, 1), gen.tableau("mixed", 16, 16, 11), gen.tableau("mixed", 8, 10, 2),
           gen.tableau("mixed", 1, 1, 1), gen.tableau("mixed", 16, 16, 12)]
    got = ragged_canonical_basis(lps)
    for a, b in zip(lps, got):
        assert b.dtype == np.int32 and b.tolist() == canonical_basis(a[None])[0].tolist()
    # the first non-canonical LP by its position in the caller's sequence, not in its group
    lps[4] = lps[4].copy()
    lps[4][3, 0] = -1.0
    lps[2] = lps[2].copy()
    lps[2][5, 11 + 4] = 2.0
    with pytest.raises(ValueError, match="LP 2 "):
        ragged_canonical_basis(lps)
    with pytest.raises(ValueError, match="LP 2 "):
        solve_ragged(lps)
    lps[2] = gen.tableau("mixed", 8, 10, 2)
    with pytest.raises(ValueError, match="LP 4 "):
        solve_ragged(lps)


def test_front_end_argument_checks():
    a = gen.tableau("mixed", 8, 10, 1)
    b = gen.tableau("mixed", 16, 16, 11)
    with pytest.raises(ValueError, match="empty"):
        solve_ragged([])
    with pytest.raises(ValueError, match="LP 1 "):
        solve_ragged([a, b[0]])
    with pytest.raises(ValueError, match="LP 1 "):
        solve_lp_ragged([a, np.zeros((1, 4))])
    with pytest.raises(ValueError, match="rule and steps"):
        solve_ragged([a, b], rule=_lib.RULE_MIN_INDEX)
    with pytest.raises(ValueError, match="basis"):
        solve_ragged([a, b], basis=[np.zeros(8, dtype=np.int32)])
    with pytest.raises(ValueError, match="too large"):
        solve_lp_ragged([a, np.zeros((202, 402))])


def test_uniform_calls_still_refuse_ragged_input():
    a = gen.tableau("mixed", 8, 10, 1)
    b = gen.tableau("mixed", 16, 16, 11)
    with pytest.raises(ValueError, match="same shape"):
        solve_batch([a, b])
    with pytest.raises(ValueError, match="same shape"):
        solve_lp_batch([Tableau.fromArray(a), Tableau.fromArray(b)])


def test_ragged_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    a = gen.tableau("mixed", 8, 10, 1)
    b = gen.tableau("mixed", 16, 16, 11)
    with pytest.raises(_lib.EngineUnavailable):
        solve_ragged([a, b])
    with pytest.raises(_lib.EngineUnavailable):
        solve_lp_ragged([Tableau.fromArray(a), b])
    with pytest.raises(_lib.EngineUnavailable):
        _lib.RaggedEngine([(8, 18), (16, 32)])
