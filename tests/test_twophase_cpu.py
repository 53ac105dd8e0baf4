"""Batched two-phase solve (lp_twophase_*): the parts of the C-ABI and the
front-end that need no GPU."""
import os
import re

import pytest

from conftest import ROOT

import lpsol_amd
from lpsol_amd import Tableau, _lib, solve_batch, solve_lp_batch
from lpsol_amd import generators as gen

TWOPHASE_SYMBOLS = {"lp_twophase_solve", "lp_twophase_lds_bytes"}


def _header():
    text = open(os.path.join(ROOT, "include", "lpgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_twophase_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = _header()
    assert set(re.findall(r"\b(lp_twophase_\w+)\s*\(", text)) == TWOPHASE_SYMBOLS
    assert TWOPHASE_SYMBOLS <= set(_lib.EXPORTS)
    for name in TWOPHASE_SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    assert len(_lib._PROTOS["lp_twophase_solve"][1]) == 8
    assert {"solve_lp_batch", "LPBatchResult"} <= set(lpsol_amd.__all__)
    assert hasattr(_lib.BatchEngine, "solve_lp")


def test_status_codes_and_stages_match_the_header():
    text = _header()
    assert re.search(r"\bLP_INFEASIBLE\s*=\s*-7\b", text)
    assert re.search(r"\bLP_PHASE1_FAILED\s*=\s*-8\b", text)
    assert (_lib.INFEASIBLE, _lib.PHASE1_FAILED) == (-7, -8)
    assert _lib.STATUS_NAMES[_lib.INFEASIBLE] == "infeasible"
    assert _lib.STATUS_NAMES[_lib.PHASE1_FAILED] == "phase1_failed"
    assert len(set(_lib.STATUS_NAMES.values())) == len(_lib.STATUS_NAMES)
    for name, val in (("PHASE2", 0), ("ARTIFICIAL", 1), ("DRIVE_OUT", 2)):
        assert re.search(r"#define\s+LP_STAGE_" + name + r"\s+" + str(val) + r"\b", text)
        assert getattr(_lib, "STAGE_" + name) == val


def test_lds_formula_is_the_python_mirror():
    lib = _lib.load()
    for m, n in ((1, 1), (7, 13), (8, 10), (24, 24), (32, 73), (34, 66), (40, 40), (88, 128),
                 (200, 400)):
        assert lib.lp_twophase_lds_bytes(m, n) == _lib.twophase_lds_bytes(m, n), (m, n)
        # never less than the plain batch kernel asks for the same LP
        assert _lib.twophase_lds_bytes(m, n) > _lib.batch_lds_bytes(m, n)
    # the formula spelled out: rows and P at the widened odd pitch, F, scratch, basis
    m, n = 7, 13
    pitch = (n + 1 + m) | 1
    assert _lib.twophase_lds_bytes(m, n) == 8 * ((m + 1) * pitch + pitch + (m + 1) + 16 + (m + 1) // 2)
    assert lib.lp_twophase_lds_bytes(0, 4) == _lib.BAD_ARG
    assert lib.lp_twophase_lds_bytes(4, -1) == _lib.BAD_ARG
    assert lib.lp_twophase_lds_bytes(1 << 40, 4) > _lib.BATCH_LDS_MAX


def test_max_m_sits_on_the_160_kib_boundary():
    n = 128
    mmax = _lib.twophase_max_m(n)
    assert mmax > 0
    assert _lib.twophase_lds_bytes(mmax, n) <= _lib.BATCH_LDS_MAX < _lib.twophase_lds_bytes(mmax + 1, n)
    # the widened shape is refused where the plain one still fits
    assert _lib.batch_lds_bytes(mmax + 1, n) <= _lib.BATCH_LDS_MAX
    assert mmax < _lib.batch_max_m(n)
    assert _lib.twophase_max_m(1 << 20) == 0


def test_wave_threshold():
    assert _lib.twophase_waves(6, 12) == 1 and _lib.twophase_waves(6, 8) == 1
    assert _lib.twophase_waves(31, 72) == 4 and _lib.twophase_waves(33, 65) == 4
    # exactly 2048 widened elements is still one wave: (m+1)(n+1+m) = 32 * 64
    assert _lib.twophase_waves(31, 32) == 1 and _lib.twophase_waves(31, 33) == 4


def test_null_batch_is_refused():
    lib = _lib.load()
    assert lib.lp_twophase_solve(None, -1, None, None, None, None, None, None) == _lib.BAD_ARG


def test_solve_lp_batch_rejects_ragged_input_as_solve_batch_does():
    a = gen.phase1_lp("ge", 4, 5, 1)
    b = gen.phase1_lp("ge", 6, 8, 1)
    for fn in (solve_batch, solve_lp_batch):
        with pytest.raises(ValueError, match="same shape"):
            fn([a, b])
        with pytest.raises(ValueError, match="same shape"):
            fn([Tableau.fromArray(a), Tableau.fromArray(b)])
        with pytest.raises(ValueError, match="empty batch"):
            fn([])


def test_solve_batch_still_refuses_phase1_and_names_the_new_function():
    with pytest.raises(ValueError, match="LP 0 .*solve_lp_batch"):
        solve_batch([gen.phase1_lp("ge", 4, 5, 1)])


def test_solve_lp_batch_has_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    with pytest.raises(_lib.EngineUnavailable):
        solve_lp_batch([gen.phase1_lp("ge", 4, 5, 1)])
