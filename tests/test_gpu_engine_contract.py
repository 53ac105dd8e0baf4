"""The single-LP engine (lp_create / lp_create_group) against oracle/lp_f64.c
where the other tests do not go: every lp_tol field on every selection path
(k_ratio / k_pick per pivot, the persistent selection on one XCD, an in-process
group of row shards, the XCD shards), on the column scans and on
lp_pivot_checked; rows at the ends of the exponent range and in the denormals;
and the header's claim that a batched solve equals a single-LP one.

Finite inputs only: the engine's contract covers finite tableaux whose
eligible ratios stay finite (include/lpgpu.h).  Every comparison is of exact
bytes, and every test asserts the path it means to run.  The inputs and why
each field bites on them: tests/_contract_cases.py, tests/test_contract_cpu.py."""
import numpy as np
import pytest

import _contract_cases as cc
from lpsol_amd import _lib, solve_batch
from lpsol_amd import generators as gen
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu

CAP = 4096


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def make(T, nshards=1, block=None, tol=None):
    """-> the handles of one tableau: [engine] or the members of a shard group"""
    m, n = T.shape[0] - 1, T.shape[1] - 1
    grp = [_lib.Engine(m, n)] if nshards == 1 else _lib.create_group(m, n, nshards)
    for g in grp:
        g.upload(T)
    if block is not None:
        grp[0].set_block(block)
    if tol:
        grp[0].set_tol(**tol)           # lp_set_tol reaches every member
    return grp


def close(grp):
    for g in reversed(grp):
        g.close()


def tableau_of(grp, shape):
    D = np.empty(shape)
    D[:1] = grp[0].rows(0, 1)
    for g in grp:
        b, c = g.row_begin, g.row_count
        D[1 + b:1 + b + c] = g.rows(1 + b, c)
        assert cc.same_bits(g.rows(0, 1), D[:1])            # row 0 is replicated
    return D


def drive(grp, call, rule, k, shape):
    e = grp[0]
    if call == "solve":
        st, npiv, nstd = e.solve(k)
    else:
        (st, npiv), nstd = e.run(rule, k), 0
    T = tableau_of(grp, shape)
    return dict(status=st, npiv=npiv, nstd=nstd, log=e.log().tolist(), T=T, z=e.objective())


def check(got, want, what=""):
    assert np.isfinite(want["T"]).all(), what
    assert got["status"] == want["status"], what
    assert (got["npiv"], got["nstd"]) == (want["npiv"], want["nstd"]), what
    assert got["log"] == want["log"], what
    assert cc.same_bits(got["T"], want["T"]), what
    assert cc.same_bits(np.float64(got["z"]), np.float64(want["z"])), what


def assert_path(grp, path):
    e = grp[0]
    p, fallbacks = e.exchange_path()
    assert fallbacks == 0
    if path == "kernels":
        assert p == _lib.PATH_KERNELS
    elif path.startswith("persistent"):
        geo = e.geometry()
        assert p == _lib.PATH_PERSISTENT
        assert geo["kernel"] == "k_sel" and geo["on_one_xcd"] and geo["xcd_shards"] != 8, geo
    elif path == "group3":
        assert p == _lib.PATH_PEER and len(grp) == 3
    elif path == "xcd_shards":
        geo = e.geometry()
        assert p == _lib.PATH_PERSISTENT
        assert geo["kernel"] == "k_sel" and geo["xcd_shards"] == 8 and geo["xcd_shards_engaged"], geo


def setup_of(path, monkeypatch):
    """-> (nshards, pivots per sweep) and the environment of the path"""
    monkeypatch.setenv("LPGPU_SELECT", "kernels" if path == "kernels" else "persistent")
    if path == "group3":
        return 3, None
    return 1, {"persistent_run_8": 8, "persistent_run_64": 64}.get(path)


# ---------------------------------------------------------------------------
# 1. tolerance fields
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,tol", cc.TOL_SETS, ids=cc.TOL_IDS)
@pytest.mark.parametrize("path", cc.ENGINE_PATHS)
def test_each_tolerance_field_on_each_path(path, name, tol, monkeypatch):
    call, rule, k, inputs = cc.engine_plan(path, name)
    nshards, block = setup_of(path, monkeypatch)
    differs = False
    for T in inputs:
        grp = make(T, nshards, block, tol)
        got = drive(grp, call, rule, k, T.shape)
        check(got, cc.oracle_call(call, rule, k, T, tol), f"{path} {name}")
        differs = differs or cc.result_differs(got, cc.oracle_call(call, rule, k, T))
        if got["npiv"]:
            assert_path(grp, path)
        close(grp)
    assert differs


@pytest.mark.parametrize("select", ["persistent", "kernels"])
def test_stall_field_through_lp_solve(select, monkeypatch):
    monkeypatch.setenv("LPGPU_SELECT", select)
    T = gen.klee_minty(8)
    tol = dict(stall=cc.STALL)
    grp = make(T, tol=tol)
    got = drive(grp, "solve", 0, CAP, T.shape)
    check(got, cc.oracle_solve(T, CAP, tol))
    assert (got["npiv"], got["nstd"]) == (89, 24) and got["nstd"] == 8 + 16
    assert grp[0].exchange_path()[1] == 0
    close(grp)


def _norm(x):
    return list(x) if isinstance(x, tuple) else x


@pytest.mark.parametrize("field", cc.SCAN_FIELDS + ["all_six"])
@pytest.mark.parametrize("nshards", [1, 3])
def test_each_tolerance_field_on_the_scans(nshards, field):
    """findPivotAll and findPivotMaxIncrease (k_colstat / k_colband and the
    host combine read cost, pivot, zero and ratio_tie) along a 10-pivot walk"""
    tol = dict(cc.TOL_SETS)[field]
    T = cc.scan_input()
    want, want_T = cc.scan_walk(T, tol)
    grp = make(T, nshards, tol=tol)
    got = []
    for _ in range(10):
        fa = [list(p) for p in grp[0].find_all()]
        w = grp[0].find_max_increase(True)
        got.append([fa, _norm(w)])
        if isinstance(w, str):
            break
    assert got == want
    assert got != cc.scan_walk(T, None)[0]
    assert cc.same_bits(tableau_of(grp, T.shape), want_T)
    close(grp)


@pytest.mark.parametrize("field", cc.CHECKED_FIELDS + ["all_six"])
@pytest.mark.parametrize("nshards", [1, 3])
def test_each_tolerance_field_on_pivot_checked(nshards, field):
    """Simplex.pivot's min-ratio check reads pivot, zero and ratio_tie: one
    pivot the band refuses (nothing changes), one it takes although the
    default lp_tol would not"""
    tol = dict(cc.TOL_SETS)[field]
    T = cc.scan_input()
    acc, ref = cc.checked_pair(T, tol)
    grp = make(T, nshards, tol=tol)
    assert grp[0].pivot_checked(*ref) == _lib.BAD_PIVOT
    assert cc.same_bits(tableau_of(grp, T.shape), T)
    assert grp[0].pivot_checked(*acc) == _lib.PIVOTED
    o = F64Tableau(T, tol)
    assert o.pivot(*acc) == _lib.PIVOTED
    assert cc.same_bits(tableau_of(grp, T.shape), o.T)
    close(grp)
    # the same two pivots under the default lp_tol: the accepted one is refused
    grp = make(T, nshards)
    assert grp[0].pivot_checked(*acc) == _lib.BAD_PIVOT
    close(grp)


# ---------------------------------------------------------------------------
# 2. exponent range
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("down", [False, True], ids=["wide", "denormal"])
@pytest.mark.parametrize("path", ["kernels", "persistent_solve", "group3"])
def test_scaled_rows(path, down, monkeypatch):
    """every constraint row of mixed 130x70 times its own power of two: the
    pivot-row division, the deferred FMA sweep and the ratio summaries at
    extreme exponents and on denormals; log and every row exact"""
    nshards, block = setup_of(path, monkeypatch)
    for s in (1, 2):
        plain = gen.tableau("mixed", 130, 70, s)
        T = cc.scaled(plain, s, down)
        grp = make(T, nshards, block, cc.SCALE_TOL)
        got = drive(grp, "solve", 0, CAP, T.shape)
        want = cc.oracle_solve(T, CAP, cc.SCALE_TOL)
        check(got, want, f"{path} seed {s}")
        assert want["log"] == cc.oracle_solve(plain, CAP, cc.SCALE_TOL)["log"] and want["npiv"] > 100
        assert_path(grp, path)
        close(grp)


# ---------------------------------------------------------------------------
# 3. a batched solve equals a single-LP solve of each LP
# ---------------------------------------------------------------------------

def _batch_inputs():
    return {
        "mixed_8x10": (gen.mixed_stack(8, 10, range(1, 9)), None),
        "mixed_8x10_all_six": (gen.mixed_stack(8, 10, range(1, 9)), cc.ALL_SIX),
        "mixed_31x33": (gen.mixed_stack(31, 33, range(1, 9)), None),
        "mixed_31x33_all_six": (gen.mixed_stack(31, 33, range(1, 9)), cc.ALL_SIX),
        "scaled_31x33_wide": (cc.scaled_stack(31, 33, range(1, 5), False), cc.SCALE_TOL),
        "scaled_31x33_denormal": (cc.scaled_stack(31, 33, range(1, 5), True), cc.SCALE_TOL),
        "km8_stall": (gen.klee_minty(8)[None], dict(stall=cc.STALL)),
    }


@pytest.mark.parametrize("which", list(_batch_inputs()))
def test_batch_equals_single_lp(which):
    """include/lpgpu.h: on finite tableaux whose eligible ratios stay finite,
    each LP of a batch gets the result of an lp_solve of its own"""
    stack, tol = _batch_inputs()[which]
    basis0 = np.full((stack.shape[0], stack.shape[1] - 1), -1, dtype=np.int32)
    res = solve_batch(stack, basis=basis0, tol=tol, max_pivots=CAP, log_cap=512)
    for i, T in enumerate(stack):
        want = cc.oracle_solve(T, CAP, tol)
        grp = make(T, tol=tol)
        single = drive(grp, "solve", 0, CAP, T.shape)
        assert grp[0].exchange_path()[1] == 0
        close(grp)
        batch = dict(status=int(res.status_code[i]), npiv=int(res.npiv[i]), nstd=int(res.nstd[i]),
                     log=res.log(i).tolist(), T=res.tableaux[i], z=res.objective[i])
        check(single, want, f"single LP {i}")
        check(batch, want, f"batch LP {i}")
        check(batch, single, f"batch against single, LP {i}")
        assert want["status"] == cc.OPTIMAL and want["npiv"] >= 1
