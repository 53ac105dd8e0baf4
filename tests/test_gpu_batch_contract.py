"""k_batch (csrc/batch.hip) against oracle/lp_f64.c where test_gpu_batch.py does
not go: non-finite cells, negative b and zero pivots; every lp_tol field; rows
at the ends of the exponent range and in the denormals; and the parts of the
lp_batch_* API no other test calls.

Every comparison takes status, npiv, nstd, the whole log, the objective and
the tableau: exact bytes where the input is finite, same_values (NaN in the
same cells, every other cell's bytes) where it is not.  The inputs and the
conditions that make them worth running are in tests/_contract_cases.py and
tests/test_contract_cpu.py.  Every solve of an input with non-finite cells or
a zero pivot carries a cap."""
import ctypes as C

import numpy as np
import pytest

import _contract_cases as cc
from lpsol_amd import _lib
from lpsol_amd import generators as gen

pytestmark = pytest.mark.gpu

CAP = 4096


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def records(eng, st, npiv, nstd):
    T, z = eng.download(), eng.objective()
    return [dict(status=int(st[i]), npiv=int(npiv[i]), nstd=int(nstd[i]), log=eng.log(i).tolist(),
                 T=T[i], z=z[i]) for i in range(eng.count)]


def batch_solve(stack, *, cap, tol=None, chunk=None, log_cap=CAP):
    stack = np.ascontiguousarray(stack, dtype=np.float64)
    eng = _lib.BatchEngine(stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1, log_cap=log_cap)
    if tol:
        eng.set_tol(**tol)
    if chunk is not None:
        eng.set_chunk(chunk)
    eng.upload(stack)
    out = records(eng, *eng.solve(cap))
    eng.close()
    return out


def batch_run(stack, rule, k, *, tol=None, chunk=None, log_cap=64):
    stack = np.ascontiguousarray(stack, dtype=np.float64)
    eng = _lib.BatchEngine(stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1, log_cap=log_cap)
    if tol:
        eng.set_tol(**tol)
    if chunk is not None:
        eng.set_chunk(chunk)
    eng.upload(stack)
    st, done = eng.run(rule, k)
    out = records(eng, st, done, np.zeros_like(done))
    eng.close()
    return out


def check(got, want, *, finite, what=""):
    """one LP's GPU record against the oracle's (or another GPU record)"""
    same = cc.same_bits if finite else cc.same_values
    assert got["status"] == want["status"], what
    assert (got["npiv"], got["nstd"]) == (want["npiv"], want["nstd"]), what
    assert got["log"] == want["log"], what
    assert same(got["T"], want["T"]), what
    assert same(np.atleast_1d(np.float64(got["z"])), np.atleast_1d(np.float64(want["z"]))), what
    if finite:
        assert np.isfinite(want["T"]).all(), what


def check_stack(got, stack, *, cap, tol=None, finite):
    with np.errstate(all="ignore"):
        want = [cc.oracle_solve(T, cap, tol) for T in stack]
    for i, (g, w) in enumerate(zip(got, want)):
        check(g, w, finite=finite, what=f"LP {i}")
    return want


# ---------------------------------------------------------------------------
# 1. the hand-built cases, embedded at both kernels' shapes
# ---------------------------------------------------------------------------

def _groups():
    """the cases that share an lp_tol and a cap go into one batch"""
    out = {}
    for c in cc.CASES:
        key = (tuple(sorted((c["tol"] or {}).items())), c["cap"])
        out.setdefault(key, []).append(c["name"])
    return list(out.values())


@pytest.mark.parametrize("chunk", [1, None], ids=["chunk1", "chunk_default"])
@pytest.mark.parametrize("m,n,row_at", cc.EMBEDDINGS)
def test_special_cases(m, n, row_at, chunk):
    """NaN in b, a and c, a -inf cost (the NaN band), negative b, a zero pivot
    counted and not applied, a at the pivot tolerance, overflowing ratios: the
    oracle's result, and the table's literal status and log"""
    seen = 0
    for names in _groups():
        cases, stack = cc.case_stack(m, n, row_at, names)
        tol, cap = cases[0]["tol"], cases[0]["cap"]
        got = batch_solve(stack, cap=cap, tol=tol, chunk=chunk, log_cap=8)
        check_stack(got, stack, cap=cap, tol=tol, finite=False)
        for c, g, T in zip(cases, got, stack):
            assert g["status"] == c["status"], c["name"]
            assert g["log"] == cc.mapped_log(c, row_at), c["name"]
            assert g["nstd"] == c["nstd"], c["name"]
            assert cc.same_values(g["T"], T) == c["untouched"], c["name"]
        seen += len(cases)
    assert seen == len(cc.CASES)


# ---------------------------------------------------------------------------
# 2. dirty stacks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,ns,k", cc.DIRTY_SHAPES)
def test_dirty_stacks(m, ns, k):
    stack = cc.dirty_stack(m, ns, k, range(1, 65))
    got = batch_solve(stack, cap=cc.DIRTY_CAP, log_cap=cc.DIRTY_CAP)
    want = check_stack(got, stack, cap=cc.DIRTY_CAP, finite=False)
    assert max(w["npiv"] for w in want) < cc.DIRTY_CAP


# ---------------------------------------------------------------------------
# 3. each tolerance field alone, then all six together
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain_results():
    return {}


@pytest.mark.parametrize("name,tol", cc.TOL_SETS, ids=cc.TOL_IDS)
@pytest.mark.parametrize("m,ns", [(8, 10), (31, 33)], ids=["one_wave", "four_waves"])
def test_each_tolerance_field(m, ns, name, tol, plain_results):
    stack = gen.mixed_stack(m, ns, range(1, 9))
    got = batch_solve(stack, cap=CAP, tol=tol, log_cap=512)
    check_stack(got, stack, cap=CAP, tol=tol, finite=True)
    if (m, ns) not in plain_results:
        plain_results[m, ns] = batch_solve(stack, cap=CAP, log_cap=512)
    assert any(cc.result_differs(a, b) for a, b in zip(got, plain_results[m, ns]))
    if name == "zero" and (m, ns) == (31, 33):
        assert [g["status"] for g in got] == [cc.OBJ_INCREASED] * 8


@pytest.mark.parametrize("padded", [False, True], ids=["one_wave", "four_waves"])
def test_stall_field(padded):
    km = cc.km8_padded() if padded else gen.klee_minty(8)
    m, n = km.shape[0] - 1, km.shape[1] - 1
    stack = np.stack([km, km])
    tol = dict(stall=cc.STALL)
    got = batch_solve(stack, cap=CAP, tol=tol, log_cap=256)
    check_stack(got, stack, cap=CAP, tol=tol, finite=True)
    assert got[0]["nstd"] == m + n < got[0]["npiv"]
    assert (got[0]["npiv"], got[0]["nstd"]) == ((253, 238) if padded else (89, 24))
    plain = batch_solve(stack[:1], cap=CAP, log_cap=256)
    assert (plain[0]["npiv"], plain[0]["nstd"]) == (255, 255)


# ---------------------------------------------------------------------------
# 4. exponent range
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("down", [False, True], ids=["wide", "denormal"])
@pytest.mark.parametrize("m,ns", cc.SCALED_SHAPES)
def test_scaled_rows(m, ns, down):
    """every constraint row times its own power of two (2^-480..2^480, or
    2^-1040..2^-40 into the denormals): the divisions, the LDS update and the
    ratio test at extreme exponents, bit for bit"""
    stack = cc.scaled_stack(m, ns, range(1, 5), down)
    got = batch_solve(stack, cap=CAP, tol=cc.SCALE_TOL, log_cap=512)
    want = check_stack(got, stack, cap=CAP, tol=cc.SCALE_TOL, finite=True)
    plain = [cc.oracle_solve(gen.tableau("mixed", m, ns, s), CAP, cc.SCALE_TOL) for s in range(1, 5)]
    assert [g["log"] for g in got] == [p["log"] for p in plain]
    assert all(w["status"] == cc.OPTIMAL and w["npiv"] >= 2 for w in want)


# ---------------------------------------------------------------------------
# 5. parts of the API no other test reaches
# ---------------------------------------------------------------------------

def test_run_with_the_standard_rule():
    stack = gen.mixed_stack(8, 10, range(1, 9))
    full = max(cc.oracle_solve(T, CAP)["npiv"] for T in stack)
    for k in (0, 1, 7, full + 5):
        got = batch_run(stack, _lib.RULE_STANDARD, k)
        for i, T in enumerate(stack):
            check(got[i], cc.oracle_run(T, cc.RULE_STANDARD, k), finite=True, what=f"k {k} LP {i}")
        if k == 0:
            assert all(g["status"] == cc.PIVOTED and g["npiv"] == 0 for g in got)
            assert all(cc.same_bits(g["T"], T) for g, T in zip(got, stack))
        if k == 1:
            assert all(g["status"] == cc.PIVOTED and g["npiv"] == 1 for g in got)
        if k == 7:      # some LPs are optimal sooner, some still running
            assert {g["status"] for g in got} == {cc.PIVOTED, cc.OPTIMAL}
        if k > full:
            assert all(g["status"] == cc.OPTIMAL and g["npiv"] < k for g in got)


def same_records(a, b):
    for x, y in zip(a, b):
        check(x, y, finite=True)


def test_chunked_run_and_chunked_capped_solves():
    stack = gen.mixed_stack(8, 10, range(1, 5))
    for rule in (_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX):
        want = batch_run(stack, rule, 7)
        for i, T in enumerate(stack):
            check(want[i], cc.oracle_run(T, rule, 7), finite=True)
        for chunk in (1, 2, 3):
            same_records(batch_run(stack, rule, 7, chunk=chunk), want)
    p = max(cc.oracle_solve(T, CAP)["npiv"] for T in stack)
    assert p == 9
    for cap in range(p + 2):
        whole = batch_solve(stack, cap=cap, log_cap=16)
        check_stack(whole, stack, cap=cap, finite=True)
        for chunk in (1, 2, 3):
            same_records(batch_solve(stack, cap=cap, chunk=chunk, log_cap=16), whole)
    assert {w["status"] for w in whole} == {cc.OPTIMAL}


def test_log_shorter_than_the_pivot_count():
    stack = gen.mixed_stack(8, 10, range(1, 5))
    want = [cc.oracle_solve(T, CAP) for T in stack]
    assert want[0]["npiv"] == 6
    eng = _lib.BatchEngine(4, 8, 18, log_cap=3)
    eng.upload(stack)
    st, npiv, nstd = eng.solve(CAP)
    assert npiv.tolist() == [w["npiv"] for w in want]
    for i, w in enumerate(want):
        assert eng.log(i).tolist() == w["log"][:3], i          # the neighbours' logs are intact
        cnt = C.c_int64()
        eng._check(eng.lib.lp_batch_log(eng.h, i, None, 0, C.byref(cnt)), eng.h)
        assert cnt.value == w["npiv"]
    out = eng.download()
    assert all(cc.same_bits(out[i], w["T"]) for i, w in enumerate(want))
    eng.close()


def test_raw_log_with_a_cap_below_log_cap():
    T = gen.tableau("mixed", 8, 10, 1)
    want = cc.oracle_solve(T, CAP)
    eng = _lib.BatchEngine(1, 8, 18, log_cap=16)
    eng.upload(T[None])
    eng.solve(CAP)
    buf = np.full((4, 2), -7, dtype=np.int64)
    cnt = C.c_int64()
    eng._check(eng.lib.lp_batch_log(eng.h, 0, buf.ctypes.data_as(_lib._P64), 2, C.byref(cnt)), eng.h)
    assert cnt.value == 6
    assert buf[:2].tolist() == want["log"][:2] and (buf[2:] == -7).all()
    eng.close()


def test_second_solve_continues_a_capped_one():
    """a new lp_batch_solve starts from the current tableau: z0 is taken anew,
    the counters and the log start over"""
    stack = gen.mixed_stack(8, 10, range(1, 5))
    eng = _lib.BatchEngine(4, 8, 18, log_cap=16)
    eng.upload(stack)
    first = records(eng, *eng.solve(2))
    second = records(eng, *eng.solve(-1))
    eng.close()
    for i, T in enumerate(stack):
        a = cc.oracle_solve(T, 2)
        check(first[i], a, finite=True)
        assert a["status"] == cc.CAP_REACHED and a["npiv"] == 2
        b = cc.oracle_solve(a["T"], CAP)
        check(second[i], b, finite=True)
        assert b["status"] == cc.OPTIMAL
    assert [r["npiv"] for r in second] == [4, 0, 7, 3]      # LP 1 was optimal after its two


def test_host_leading_dimension_above_n_plus_1():
    stack = gen.mixed_stack(8, 10, range(1, 4))
    B, rows, w = stack.shape
    ldh, sentinel = w + 3, -777.25
    host = np.full((B, rows, ldh), sentinel)
    host[:, :, :w] = stack
    eng = _lib.BatchEngine(B, 8, 18, log_cap=16)
    eng._check(eng.lib.lp_batch_upload(eng.h, 0, B, host.ctypes.data_as(_lib._PD), ldh), eng.h)
    assert cc.same_bits(eng.download(), stack)              # the padding did not reach the device
    eng.solve(CAP)
    back = np.full((B, rows, ldh), sentinel)
    eng._check(eng.lib.lp_batch_download(eng.h, 0, B, back.ctypes.data_as(_lib._PD), ldh), eng.h)
    assert (back[:, :, w:] == sentinel).all()               # ... and is not written on the way back
    for i in range(B):
        assert cc.same_bits(back[i, :, :w], cc.oracle_solve(stack[i], CAP)["T"])
    # one LP of the window, at an offset
    one = np.full((1, rows, ldh), sentinel)
    eng._check(eng.lib.lp_batch_download(eng.h, 2, 1, one.ctypes.data_as(_lib._PD), ldh), eng.h)
    assert cc.same_bits(one, back[2:3])
    with pytest.raises(ValueError):
        eng._check(eng.lib.lp_batch_upload(eng.h, 0, B, host.ctypes.data_as(_lib._PD), w - 1), eng.h)
    eng.close()


def test_get_basis_after_detaching_raises():
    stack = gen.mixed_stack(8, 10, range(1, 3))
    eng = _lib.BatchEngine(2, 8, 18)
    eng.upload(stack)
    eng.set_basis(np.zeros((2, 8), dtype=np.int32))
    assert eng.get_basis().shape == (2, 8)
    eng.set_basis(None)
    with pytest.raises(ValueError, match="no basis attached"):
        eng.get_basis()
    eng.solve(CAP)                                          # and the solve runs without one
    assert cc.same_bits(eng.download()[0], cc.oracle_solve(stack[0], CAP)["T"])
    eng.close()
