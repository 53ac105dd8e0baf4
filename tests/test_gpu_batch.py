"""Batched solve on the GPU (csrc/batch.hip, lp_batch_*, lpsol_amd.solve_batch).

Every comparison is exact: status, pivot counts, the log and the basis are
equal to the oracle's (oracle/lp_f64.c through oracle.f64.F64Tableau) or the
golden fixture's, and the tableaux are bit-identical."""
import numpy as np
import pytest

from conftest import fixture_input

from lpsol_amd import _lib, solve_batch
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis
from oracle.f64 import F64Tableau

pytestmark = pytest.mark.gpu

CAP = 4096      # pivot cap given to both sides where the test is not about caps


def oracle_solve(T, cap=CAP, tol=None):
    o = F64Tableau(T, tol)
    st, log, nstd = o.solve(cap=cap, logcap=max(cap, 1))
    return st, log, nstd, o.T


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def engine_solve(stack, *, cap=CAP, chunk=None, log_cap=CAP, basis=None, tol=None):
    """one lp_batch_solve through the thin engine -> dict of per-LP results"""
    stack = np.ascontiguousarray(stack, dtype=np.float64)
    B, m, n = stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1
    eng = _lib.BatchEngine(B, m, n, log_cap=log_cap)
    if tol:
        eng.set_tol(**tol)
    if chunk is not None:
        eng.set_chunk(chunk)
    eng.upload(stack)
    if basis is not None:
        eng.set_basis(basis)
    st, npiv, nstd = eng.solve(cap)
    out = dict(status=st, npiv=npiv, nstd=nstd, T=eng.download(), z=eng.objective(),
               log=[eng.log(i) for i in range(B)],
               basis=eng.get_basis() if basis is not None else None)
    eng.close()
    return out


def assert_matches_oracle(res, stack, *, cap=CAP, tol=None, basis0=None):
    for i in range(stack.shape[0]):
        st, log, nstd, T = oracle_solve(stack[i], cap, tol)
        assert res["status"][i] == st, i
        assert res["npiv"][i] == len(log) and res["nstd"][i] == nstd, i
        assert res["log"][i].tolist() == log.tolist(), i
        assert np.array_equal(res["T"][i], T), i
        assert res["z"][i] == -T[0, 0], i
        if basis0 is not None:
            b = basis0[i].copy()
            for r, c in log:
                b[r] = c
            assert res["basis"][i].tolist() == b.tolist(), i


# ---------------------------------------------------------------------------
# 1. golden solves, one batch per shape
# ---------------------------------------------------------------------------

GROUPS = {
    "cfg1": lambda name: name.startswith("cfg1_"),
    "km_d8": lambda name: name in ("km_std_d8", "km_deg_d8"),
    "16x16": lambda name: name.startswith("mixed_16x16"),
    "24x32": lambda name: name.startswith("mixed_24x32"),
    "32x24": lambda name: name.startswith("mixed_32x24"),
    "40x40": lambda name: name.startswith("mixed_40x40"),
    "32x32": lambda name: name.startswith("pos_32x32"),
    "64x64": lambda name: name.startswith("pos_64x64"),
    "beale": lambda name: name == "beale",
}
GROUP_SIZES = {"cfg1": 12, "km_d8": 2, "16x16": 3, "24x32": 3, "32x24": 3, "40x40": 3,
               "32x32": 2, "64x64": 2, "beale": 1}


@pytest.mark.parametrize("group", list(GROUPS))
def test_golden_solves_grouped_by_shape(small_golden, group):
    fxs = [fx for fx in small_golden["solve"] if GROUPS[group](fx["name"])]
    assert len(fxs) == GROUP_SIZES[group]
    stack = np.stack([fixture_input(fx) for fx in fxs])
    res = solve_batch(stack, log_cap=max(len(fx["seq"]) for fx in fxs) + 1)
    for i, fx in enumerate(fxs):
        st, log, nstd, T = oracle_solve(stack[i])
        assert res.status[i] == "optimal" and st == _lib.OPTIMAL, fx["name"]
        assert res.log(i).tolist() == fx["seq"], fx["name"]
        assert res.npiv[i] == len(fx["seq"]) and res.nstd[i] == fx["nstd"], fx["name"]
        assert res.basis[i].tolist() == fx["bfs"], fx["name"]
        assert np.array_equal(res.tableaux[i], T), fx["name"]
        assert res.objective[i] == -T[0, 0], fx["name"]
        assert res.tableau(i).getZ() == -T[0, 0]


# ---------------------------------------------------------------------------
# 2. Klee-Minty d = 10: the long solve and the stall switch, with neighbours
# ---------------------------------------------------------------------------

def km10_batch(small_golden, name):
    fx = next(f for f in small_golden["solve"] if f["name"] == name)
    stack = np.stack([fixture_input(fx)] + [gen.tableau("mixed", 10, 10, s) for s in (1, 2, 3)])
    return fx, stack


@pytest.mark.parametrize("name,npiv,nstd", [("km_std_d10", 1023, 1023), ("km_deg_d10", 52, 30)])
def test_klee_minty_d10(small_golden, name, npiv, nstd):
    fx, stack = km10_batch(small_golden, name)
    assert len(fx["seq"]) == npiv and fx["nstd"] == nstd
    res = solve_batch(stack, log_cap=1024)
    assert res.log(0).tolist() == fx["seq"]
    assert (res.npiv[0], res.nstd[0]) == (npiv, nstd)
    assert res.basis[0].tolist() == fx["bfs"]
    for i in range(stack.shape[0]):
        st, log, ns, T = oracle_solve(stack[i])
        assert res.status_code[i] == st == _lib.OPTIMAL
        assert res.log(i).tolist() == log.tolist() and res.nstd[i] == ns
        assert np.array_equal(res.tableaux[i], T)


# ---------------------------------------------------------------------------
# 3. chunk resume: stuck, z0 and rule survive the launch boundary
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", [8, 10])
def test_chunked_launches_give_identical_results(d):
    stack = np.stack([gen.klee_minty(d), gen.klee_minty(d, degenerate=True)]
                     + [gen.tableau("mixed", d, d, s) for s in (1, 2)])
    basis0 = canonical_basis(stack)
    results = [engine_solve(stack, chunk=c, basis=basis0) for c in (1, 5, 4096)]
    assert_matches_oracle(results[2], stack, basis0=basis0)
    assert results[2]["npiv"][0] == 2 ** d - 1
    assert results[2]["nstd"][1] < results[2]["npiv"][1]        # the stall switch happened
    for r in results[:2]:
        for key in ("status", "npiv", "nstd", "T", "z", "basis"):
            assert np.array_equal(r[key], results[2][key]), key
        assert all(np.array_equal(a, b) for a, b in zip(r["log"], results[2]["log"]))


# ---------------------------------------------------------------------------
# 4. caps
# ---------------------------------------------------------------------------

def test_caps_match_the_oracle():
    T = gen.tableau("mixed", 8, 10, 1)
    p = len(oracle_solve(T)[1])
    assert p == 6
    for cap in (0, 1, p - 1, p, p + 1):
        res = engine_solve(T[None], cap=cap, log_cap=16)
        st = oracle_solve(T, cap)[0]
        assert st == (_lib.OPTIMAL if cap > p else _lib.CAP_REACHED)
        assert_matches_oracle(res, T[None], cap=cap)
        r = solve_batch(T[None], max_pivots=cap)
        assert r.status[0] == ("optimal" if cap > p else "cap_reached")
        assert np.array_equal(r.tableaux[0], res["T"][0])


def test_tolerances_reach_the_kernel():
    """wide tie bands change the pivot sequences; both sides get the same lp_tol"""
    stack = gen.mixed_stack(8, 10, range(1, 9))
    tol = dict(cost_tie=0.5, ratio_tie=0.25)
    res = engine_solve(stack, tol=tol, log_cap=64)
    assert_matches_oracle(res, stack, tol=tol)
    plain = engine_solve(stack, log_cap=64)
    assert any(a.tolist() != b.tolist() for a, b in zip(res["log"], plain["log"]))


# ---------------------------------------------------------------------------
# 5. mixed fates in one batch
# ---------------------------------------------------------------------------

def test_mixed_fates_in_one_batch():
    stack = np.stack([gen.tableau("mixed", 8, 10, s) for s in (1, 2, 3, 4, 5)])
    stack[2, 0, 4] = -100.0                             # the entering column ...
    stack[2, 1:, 4] = -np.abs(stack[2, 1:, 4])          # ... has no positive entry: unbounded
    stack[3, 0, 1:] = np.abs(stack[3, 0, 1:])           # no negative cost: already optimal
    res = solve_batch(stack, log_cap=16)
    assert res.status == ["optimal", "optimal", "unbounded", "optimal", "optimal"]
    assert res.npiv[2] == 0 and res.npiv[3] == 0
    assert np.array_equal(res.tableaux[3], stack[3]) and np.array_equal(res.tableaux[2], stack[2])
    assert res.log(3).shape == (0, 2)
    for i in range(5):
        st, log, nstd, T = oracle_solve(stack[i])
        assert res.status_code[i] == st
        assert res.log(i).tolist() == log.tolist() and res.nstd[i] == nstd
        assert np.array_equal(res.tableaux[i], T)


# ---------------------------------------------------------------------------
# 6. shapes at the edges of the mapping (batches of 3 seeds)
# ---------------------------------------------------------------------------

MAX_M_128 = _lib.batch_max_m(128)

EDGE_SHAPES = [
    ("tall", 64, 16, 40),            # 65 rows on a one-wave block: rows strided
    ("tall", 1, 1, CAP),             # 1 x 1
    ("mixed", 63, 63, CAP),          # 64 x 127: one row short of the wave
    ("mixed", 64, 64, CAP),          # 64 x 128: 65 rows, over 64 KiB of LDS
    ("mixed", 31, 32, CAP),          # 32 x 64 = 2048 elements: the last one-wave shape
    ("mixed", 31, 33, CAP),          # 32 x 65: the first four-wave shape
    ("tall", MAX_M_128, 128, 24),    # the largest m lp_batch_create takes at n = 128
]


@pytest.mark.parametrize("kind,m,ns,cap", EDGE_SHAPES)
def test_shapes_at_the_edges_of_the_mapping(kind, m, ns, cap):
    stack = np.stack([gen.tableau(kind, m, ns, s) for s in (1, 2, 3)])
    basis0 = np.full((3, stack.shape[1] - 1), -1, dtype=np.int32)
    res = engine_solve(stack, cap=cap, basis=basis0, log_cap=min(cap, 512))
    assert res["npiv"].max() <= 512
    assert_matches_oracle(res, stack, cap=cap, basis0=basis0)
    assert res["npiv"].min() >= 1


def test_largest_shape_is_the_largest():
    assert MAX_M_128 == 155
    with pytest.raises(ValueError, match="too large"):
        _lib.BatchEngine(1, MAX_M_128 + 1, 128)


# ---------------------------------------------------------------------------
# 7. more LPs than resident workgroups
# ---------------------------------------------------------------------------

def test_more_lps_than_resident_workgroups():
    B = 12289
    stack = gen.mixed_stack(8, 10, range(1, B + 1))
    assert np.array_equal(stack[B - 1], gen.tableau("mixed", 8, 10, B))
    res = solve_batch(stack, max_pivots=CAP, log_cap=32)
    want = np.empty_like(stack)
    for i in range(B):
        st, log, nstd, want[i] = oracle_solve(stack[i])
        assert res.status_code[i] == st and res.npiv[i] == len(log) and res.nstd[i] == nstd, i
    assert np.array_equal(res.tableaux, want)
    assert res.npiv.max() <= 32
    for i in (0, 4095, B - 1):
        assert res.log(i).tolist() == oracle_solve(stack[i])[1].tolist()


# ---------------------------------------------------------------------------
# 8. windows
# ---------------------------------------------------------------------------

def test_upload_download_windows():
    first = np.stack([gen.tableau("mixed", 8, 10, s) for s in range(1, 7)])
    fresh = np.stack([gen.tableau("mixed", 8, 10, s) for s in (21, 22)])
    eng = _lib.BatchEngine(6, 8, 18, log_cap=16)
    eng.upload(first[:3])
    eng.upload(first[3:], first=3)
    assert np.array_equal(eng.download(), first)
    st, npiv, nstd = eng.solve(CAP)
    solved = eng.download()
    logs = [eng.log(i) for i in range(6)]
    for i in range(6):
        assert np.array_equal(solved[i], oracle_solve(first[i])[3])
    eng.upload(fresh, first=2)
    assert np.array_equal(eng.download(2, 2), fresh)
    assert np.array_equal(eng.download(0, 2), solved[:2])
    assert np.array_equal(eng.download(4), solved[4:])
    assert eng.log(2).shape == (0, 2) and eng.log(3).shape == (0, 2)       # state reset
    for i in (0, 1, 4, 5):
        assert np.array_equal(eng.log(i), logs[i])                         # untouched
    with pytest.raises(ValueError):
        eng.upload(fresh, first=5)
    st2, npiv2, _ = eng.solve(CAP)
    again = eng.download()
    for k, i in enumerate((2, 3)):
        o = oracle_solve(fresh[k])
        assert st2[i] == o[0] and np.array_equal(eng.log(i), o[1]) and np.array_equal(again[i], o[3])
    for i in (0, 1, 4, 5):      # a new solve of an optimal tableau: what the oracle does with it
        o = oracle_solve(solved[i])
        assert st2[i] == o[0] and npiv2[i] == len(o[1]) == 0 and np.array_equal(again[i], o[3])
    eng.close()


# ---------------------------------------------------------------------------
# 9. fixed rule
# ---------------------------------------------------------------------------

def test_fixed_rule_run(small_golden):
    fx = next(f for f in small_golden["solve"] if f["name"] == "km_deg_d6")
    stack = np.stack([fixture_input(fx)] + [gen.tableau("mixed", 6, 6, s) for s in (1, 2, 3)])
    res = solve_batch(stack, rule=_lib.RULE_MIN_INDEX, steps=7, log_cap=8)
    for i in range(stack.shape[0]):
        o = F64Tableau(stack[i])
        st, log = o.run(_lib.RULE_MIN_INDEX, 7)
        assert res.status_code[i] == st
        assert res.npiv[i] == len(log) and res.nstd[i] == 0
        assert res.log(i).tolist() == log.tolist()
        assert np.array_equal(res.tableaux[i], o.T)
    assert res.npiv[0] == 7 and res.status[0] == "pivoted"


# ---------------------------------------------------------------------------
# 10. a ratio that overflows to +inf is a candidate, not "no candidate"
# ---------------------------------------------------------------------------

def overflow_lp(all_inf):
    T = np.zeros((4, 6))
    T[0, 1:3] = [-1.0, 1.0]
    T[1] = [1e308, 1e-3, 0.0, 1.0, 0.0, 0.0]        # eligible, b / a = +inf, before the minimum
    T[2] = [4.0, 2.0, 0.0, 0.0, 1.0, 0.0]           # the finite minimum
    T[3] = [9.0, 3.0, 0.0, 0.0, 0.0, 1.0]
    if all_inf:                                     # every eligible ratio overflows: the first row leaves
        T[2] = [1e308, 2e-3, 0.0, 0.0, 1.0, 0.0]
        T[3] = [1e308, 4e-3, 0.0, 0.0, 0.0, 1.0]
    return T


def test_overflowing_ratio_takes_the_oracles_leaving_row():
    stack = np.stack([overflow_lp(False), overflow_lp(True), overflow_lp(False)])
    stack[2, 1, 0] = 1.0                            # a plain neighbour: every ratio finite
    res = solve_batch(stack, log_cap=8)
    want_first = [[1, 0], [0, 0], [1, 0]]
    for i in range(3):
        st, log, nstd, T = oracle_solve(stack[i])
        assert log[0].tolist() == want_first[i]
        assert res.status_code[i] == st and res.nstd[i] == nstd
        assert res.log(i).tolist() == log.tolist()
        assert same_bits(res.tableaux[i], T)
