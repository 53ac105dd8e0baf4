"""Device-placed batches on the GPU (lp_placed_*, place= of BatchEngine /
RaggedEngine / solve_batch / solve_ragged; csrc/batch.hip k_batch_dev): LPs
whose tableau stays in device memory for the whole launch, one workgroup each.

Every comparison is exact: status, pivot counts, the log, the basis and the
objective are equal to the oracle's (oracle/lp_f64.c through
oracle.f64.F64Tableau) or the golden fixture's, and the tableaux are
bit-identical (same_values where the input holds non-finite cells).  Every
device call carries a finite pivot cap."""
import numpy as np
import pytest

from conftest import fixture_input

import _contract_cases as cc
import _ragged_cases as rc
from lpsol_amd import _lib, solve_batch, solve_ragged
from lpsol_amd import generators as gen
from lpsol_amd.batch import canonical_basis

pytestmark = pytest.mark.gpu

CAP = 4096
LDS = _lib.BATCH_LDS_MAX
DEV_WORK = 32 << 20         # element updates per launch and LP (csrc/batch.hip)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


# ------------------------------------------------------------------ oracle
_ORACLE = {}


def oracle_solve(T, cap=CAP, tol=None):
    """cc.oracle_solve, computed once per input"""
    key = (T.shape, T.tobytes(), cap, tuple(sorted((tol or {}).items())))
    if key not in _ORACLE:
        with np.errstate(all="ignore"):
            _ORACLE[key] = cc.oracle_solve(T, cap, tol)
    return _ORACLE[key]


# ------------------------------------------------------------------ device
def records(eng, st, npiv, nstd, basis):
    T, z = eng.download(), eng.objective()
    bs = eng.get_basis() if basis is not None else None
    return [dict(status=int(st[i]), npiv=int(npiv[i]), nstd=int(nstd[i]), log=eng.log(i).tolist(), T=T[i], z=z[i],
                 basis=None if bs is None else bs[i].tolist()) for i in range(eng.count)]


def make_engine(stack, place, log_cap):
    if isinstance(stack, np.ndarray):
        return _lib.BatchEngine(stack.shape[0], stack.shape[1] - 1, stack.shape[2] - 1, log_cap=log_cap, place=place)
    return _lib.RaggedEngine([rc.shape_of(T) for T in stack], log_cap=log_cap, place=place)


def placed_solve(stack, *, place="device", cap=CAP, tol=None, chunk=None, log_cap=CAP, basis=None, expect=None):
    """one lp_batch_solve of a uniform stack or a list of LPs -> one record per LP"""
    eng = make_engine(stack, place, log_cap)
    try:
        if expect is not None:
            assert [eng.placement(i) for i in range(eng.count)] == expect
        if tol:
            eng.set_tol(**tol)
        if chunk is not None:
            eng.set_chunk(chunk)
        eng.upload(stack)
        if basis is not None:
            eng.set_basis(basis)
        return records(eng, *eng.solve(cap), basis)
    finally:
        eng.close()


def placed_run(stack, rule, k, *, place="device", chunk=None, log_cap=64):
    eng = make_engine(stack, place, log_cap)
    try:
        if chunk is not None:
            eng.set_chunk(chunk)
        eng.upload(stack)
        st, done = eng.run(rule, k)
        return records(eng, st, done, np.zeros_like(done), None)
    finally:
        eng.close()


def check(got, want, *, finite=True, what="", log_cap=None):
    """one LP's device record against the oracle's (or another device record)"""
    same = cc.same_bits if finite else cc.same_values
    assert got["status"] == want["status"], what
    assert (got["npiv"], got["nstd"]) == (want["npiv"], want["nstd"]), what
    assert got["log"] == (want["log"] if log_cap is None else want["log"][:log_cap]), what
    assert same(got["T"], want["T"]), what
    assert same(np.atleast_1d(np.float64(got["z"])), np.atleast_1d(np.float64(want["z"]))), what


def check_stack(got, stack, *, cap=CAP, tol=None, finite=True, basis0=None):
    want = [oracle_solve(T, cap, tol) for T in stack]
    for i, (g, w) in enumerate(zip(got, want)):
        check(g, w, finite=finite, what=f"LP {i}")
        if basis0 is not None:
            b = list(basis0[i])
            for r, c in w["log"]:
                b[r] = c
            assert g["basis"] == b, i
    return want


def dev_threads():
    """threads of the workgroup that solves a device-placed LP"""
    eng = _lib.BatchEngine(1, 8, 18, place="device")
    plan = _lib.ragged_plan(eng)
    eng.close()
    assert len(plan) == 1 and plan[0]["waves"] in (4, 8, 16)
    assert plan[0]["lds_bytes"] == _lib.batch_device_lds_bytes(8, 18) and plan[0]["lps"] == 1
    assert plan[0]["lps_per_cu"] >= 1
    return 64 * plan[0]["waves"]


# ---------------------------------------------------------------------------
# 1. forced "device" at the small golden shapes
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
def test_golden_solves_forced_device(small_golden, group):
    fxs = [fx for fx in small_golden["solve"] if GROUPS[group](fx["name"])]
    assert len(fxs) == GROUP_SIZES[group]
    stack = np.stack([fixture_input(fx) for fx in fxs])
    res = solve_batch(stack, log_cap=max(len(fx["seq"]) for fx in fxs) + 1, place="device", max_pivots=CAP)
    assert all(res._engine.placement(i) == "device" for i in range(len(fxs)))
    for i, fx in enumerate(fxs):
        w = oracle_solve(stack[i])
        assert res.status[i] == "optimal" and w["status"] == _lib.OPTIMAL, fx["name"]
        assert res.log(i).tolist() == fx["seq"] == w["log"], fx["name"]
        assert res.npiv[i] == len(fx["seq"]) and res.nstd[i] == fx["nstd"] == w["nstd"], fx["name"]
        assert res.basis[i].tolist() == fx["bfs"], fx["name"]
        assert cc.same_bits(res.tableaux[i], w["T"]), fx["name"]
        assert res.objective[i] == -w["T"][0, 0], fx["name"]


# ---------------------------------------------------------------------------
# 2. "auto" above LDS
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,seeds", [(100, (1, 2, 3, 4)), (150, (1, 2, 3)), (256, (1,))])
def test_auto_above_lds(m, seeds):
    stack = gen.mixed_stack(m, m, seeds)
    assert _lib.batch_lds_bytes(m, 2 * m) > LDS
    with pytest.raises(ValueError, match="too large"):
        solve_batch(stack)
    basis0 = canonical_basis(stack)
    got = placed_solve(stack, place="auto", basis=basis0, expect=["device"] * len(seeds))
    want = check_stack(got, stack, basis0=basis0)
    assert all(w["status"] == _lib.OPTIMAL for w in want)
    if seeds[0] == 1:
        assert want[0]["npiv"] == {100: 216, 150: 491, 256: 2157}[m]
    if m == 256:        # the work-based cap is below the pivot count: the solve took several launches
        assert want[0]["npiv"] > DEV_WORK // ((m + 1) * (2 * m + 1)) == 254
    res = solve_batch(stack, place="auto", log_cap=8, max_pivots=CAP)
    for i, w in enumerate(want):
        assert res.status_code[i] == w["status"] and res.log(i).tolist() == w["log"][:8]
        assert cc.same_bits(res.tableaux[i], w["T"]) and res.objective[i] == w["z"]
        assert res.basis[i].tolist() == got[i]["basis"]


# ---------------------------------------------------------------------------
# 3. the edges of the flat walk
# ---------------------------------------------------------------------------

def run_against_oracle(stack, rule, k):
    got = placed_run(stack, rule, k)
    for i, T in enumerate(stack):
        w = cc.oracle_run(T, rule, k)
        check(got[i], w, what=f"LP {i}")
        assert w["npiv"] >= 1
    return got


def test_fewer_elements_than_threads():
    nt = dev_threads()
    for kind, m, ns in (("tall", 1, 1), ("mixed", 8, 10)):
        stack = np.stack([gen.tableau(kind, m, ns, s) for s in (1, 2, 3)])      # E odd: LP 1 starts at an odd double
        assert stack.shape[1] * stack.shape[2] < nt and (stack.shape[1] * stack.shape[2]) % 2 == (kind == "mixed")
        basis0 = np.full((3, m), -1, dtype=np.int32)
        got = placed_solve(stack, basis=basis0, log_cap=64)
        want = check_stack(got, stack, basis0=basis0)
        assert min(w["npiv"] for w in want) >= 1


@pytest.mark.parametrize("extra", [1, 2], ids=["odd_row", "even_row"])
@pytest.mark.parametrize("rule", [_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX])
def test_rows_longer_than_one_stride(extra, rule):
    """m = 2 with n + 1 just above twice the thread count: a row is longer than
    one stride of pairs, and an odd row length makes pairs straddle rows"""
    nt = dev_threads()
    ns = 2 * nt + extra - 1
    stack = np.stack([gen.tableau("tall", 2, ns, s) for s in (1, 2)])
    assert stack.shape[1:] == (3, 2 * nt + extra)
    run_against_oracle(stack, rule, 3)


def test_more_rows_than_threads():
    nt = dev_threads()
    stack = np.stack([gen.tableau("tall", nt + 2, 7, s) for s in (1, 2)])
    assert stack.shape[1:] == (nt + 3, 8)
    got = run_against_oracle(stack, _lib.RULE_STANDARD, 4)
    assert all(g["npiv"] >= 2 for g in got)


def test_mixed_1100x60():
    T = gen.tableau("mixed", 1100, 60, 1)
    assert T.shape == (1101, 1161)
    got = placed_solve(T[None], place="auto", log_cap=256, expect=["device"])
    w = check_stack(got, T[None])[0]
    assert (w["status"], w["npiv"]) == (_lib.OPTIMAL, 142)
    assert w["npiv"] > DEV_WORK // T.size == 26            # several launches


# ---------------------------------------------------------------------------
# 4. chunk independence
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["km_std_d10", "km_deg_d10"])
def test_chunked_launches_give_identical_results(small_golden, name):
    fx = next(f for f in small_golden["solve"] if f["name"] == name)
    stack = np.stack([fixture_input(fx)] + [gen.tableau("mixed", 10, 10, s) for s in (1, 2, 3)])
    basis0 = canonical_basis(stack)
    results = [placed_solve(stack, chunk=c, basis=basis0, log_cap=1024) for c in (1, 5, 4096)]
    check_stack(results[2], stack, basis0=basis0)
    assert results[2][0]["log"] == fx["seq"] and results[2][0]["basis"] == fx["bfs"]
    assert (results[2][0]["npiv"], results[2][0]["nstd"]) == (len(fx["seq"]), fx["nstd"])
    for r in results[:2]:
        for a, b in zip(r, results[2]):
            check(a, b)
            assert a["basis"] == b["basis"]


def test_chunked_run_and_capped_solves():
    stack = gen.mixed_stack(8, 10, range(1, 5))
    for rule in (_lib.RULE_STANDARD, _lib.RULE_MIN_INDEX):
        want = placed_run(stack, rule, 7)
        for i, T in enumerate(stack):
            check(want[i], cc.oracle_run(T, rule, 7))
        for chunk in (1, 3):
            for a, b in zip(placed_run(stack, rule, 7, chunk=chunk), want):
                check(a, b)
    p = max(oracle_solve(T)["npiv"] for T in stack)
    assert p == 9
    for cap in (0, 1, 6, p, p + 1):         # LP 0 takes 6 pivots: cap 6 is reached exactly at its optimum
        whole = placed_solve(stack, cap=cap, log_cap=16)
        want = check_stack(whole, stack, cap=cap)
        for a, b in zip(placed_solve(stack, cap=cap, chunk=2, log_cap=16), whole):
            check(a, b)
    assert oracle_solve(stack[0], 6)["status"] == cc.CAP_REACHED and oracle_solve(stack[0], 7)["status"] == cc.OPTIMAL
    assert {w["status"] for w in want} == {cc.OPTIMAL}


# ---------------------------------------------------------------------------
# 5. the contract cases under forced "device"
# ---------------------------------------------------------------------------

def _groups():
    out = {}
    for c in cc.CASES:
        key = (tuple(sorted((c["tol"] or {}).items())), c["cap"])
        out.setdefault(key, []).append(c["name"])
    return list(out.values())


@pytest.mark.parametrize("chunk", [1, None], ids=["chunk1", "chunk_default"])
@pytest.mark.parametrize("m,n,row_at", cc.EMBEDDINGS)
def test_special_cases(m, n, row_at, chunk):
    seen = 0
    for names in _groups():
        cases, stack = cc.case_stack(m, n, row_at, names)
        tol, cap = cases[0]["tol"], cases[0]["cap"]
        got = placed_solve(stack, cap=cap, tol=tol, chunk=chunk, log_cap=8)
        check_stack(got, stack, cap=cap, tol=tol, finite=False)
        for c, g, T in zip(cases, got, stack):
            assert g["status"] == c["status"], c["name"]
            assert g["log"] == cc.mapped_log(c, row_at), c["name"]
            assert g["nstd"] == c["nstd"], c["name"]
            assert cc.same_values(g["T"], T) == c["untouched"], c["name"]
        seen += len(cases)
    assert seen == len(cc.CASES)


@pytest.mark.parametrize("m,ns,k", cc.DIRTY_SHAPES)
def test_dirty_stacks(m, ns, k):
    stack = cc.dirty_stack(m, ns, k, range(1, 33))
    got = placed_solve(stack, cap=cc.DIRTY_CAP, log_cap=cc.DIRTY_CAP)
    want = check_stack(got, stack, cap=cc.DIRTY_CAP, finite=False)
    assert max(w["npiv"] for w in want) < cc.DIRTY_CAP


@pytest.mark.parametrize("name,tol", cc.TOL_SETS, ids=cc.TOL_IDS)
@pytest.mark.parametrize("m,ns", [(8, 10), (31, 33)])
def test_each_tolerance_field(m, ns, name, tol):
    stack = gen.mixed_stack(m, ns, range(1, 9))
    got = placed_solve(stack, tol=tol, log_cap=512)
    want = check_stack(got, stack, tol=tol)
    plain = [oracle_solve(T) for T in stack]
    assert any(cc.result_differs(a, b) for a, b in zip(want, plain))
    if name == "zero" and (m, ns) == (31, 33):
        assert [g["status"] for g in got] == [cc.OBJ_INCREASED] * 8


@pytest.mark.parametrize("padded", [False, True])
def test_stall_field(padded):
    km = cc.km8_padded() if padded else gen.klee_minty(8)
    m, n = km.shape[0] - 1, km.shape[1] - 1
    stack = np.stack([km, km])
    tol = dict(stall=cc.STALL)
    got = placed_solve(stack, tol=tol, log_cap=256)
    check_stack(got, stack, tol=tol)
    assert got[0]["nstd"] == m + n < got[0]["npiv"]
    assert (got[0]["npiv"], got[0]["nstd"]) == ((253, 238) if padded else (89, 24))


@pytest.mark.parametrize("down", [False, True], ids=["wide", "denormal"])
@pytest.mark.parametrize("m,ns", cc.SCALED_SHAPES)
def test_scaled_rows(m, ns, down):
    stack = cc.scaled_stack(m, ns, range(1, 5), down)
    got = placed_solve(stack, tol=cc.SCALE_TOL, log_cap=512)
    want = check_stack(got, stack, tol=cc.SCALE_TOL)
    assert all(w["status"] == cc.OPTIMAL and w["npiv"] >= 2 for w in want)


# ---------------------------------------------------------------------------
# 6. the handle between calls
# ---------------------------------------------------------------------------

def test_handle_use_on_an_auto_batch():
    first = gen.mixed_stack(100, 100, (1, 2, 3, 4))
    fresh = gen.mixed_stack(100, 100, (11, 12))
    want = [oracle_solve(T) for T in first]
    LOG = 100                                   # below every pivot count
    assert min(w["npiv"] for w in want) > LOG
    eng = _lib.BatchEngine(4, 100, 200, log_cap=LOG, place="auto")
    assert [eng.placement(i) for i in range(4)] == ["device"] * 4
    with pytest.raises(ValueError):
        eng.placement(4)
    eng.upload(first[:3])
    eng.upload(first[3:], first=3)
    assert cc.same_bits(eng.download(), first)
    basis0 = canonical_basis(first)
    eng.set_basis(basis0)
    st, npiv, nstd = eng.solve(CAP)
    solved = eng.download()
    for i, w in enumerate(want):
        assert (st[i], npiv[i], nstd[i]) == (w["status"], w["npiv"], w["nstd"])
        assert eng.log(i).tolist() == w["log"][:LOG]            # log_cap below the pivot count
        assert cc.same_bits(solved[i], w["T"])
        b = basis0[i].copy()
        for r, c in w["log"]:
            b[r] = c
        assert eng.get_basis()[i].tolist() == b.tolist()
    assert eng.objective().tolist() == [w["z"] for w in want]
    # a window upload resets only its LPs
    eng.upload(fresh, first=1)
    assert cc.same_bits(eng.download(1, 2), fresh)
    assert cc.same_bits(eng.download(0, 1), solved[:1]) and cc.same_bits(eng.download(3), solved[3:])
    assert eng.log(1).shape == (0, 2) and eng.log(2).shape == (0, 2)
    assert eng.log(0).tolist() == want[0]["log"][:LOG] and eng.log(3).tolist() == want[3]["log"][:LOG]
    # a second solve on the same allocation, the basis detached
    eng.set_basis(None)
    with pytest.raises(ValueError, match="no basis attached"):
        eng.get_basis()
    st2, npiv2, _ = eng.solve(CAP)
    again = eng.download()
    for k, i in enumerate((1, 2)):
        w = oracle_solve(fresh[k])
        assert (st2[i], npiv2[i]) == (w["status"], w["npiv"]) and eng.log(i).tolist() == w["log"][:LOG]
        assert cc.same_bits(again[i], w["T"])
    for i in (0, 3):            # an optimal tableau solved again: no pivot
        assert st2[i] == _lib.OPTIMAL and npiv2[i] == 0 and cc.same_bits(again[i], solved[i])
    # a capped solve continued by a second one
    eng.upload(first[:1])
    eng.set_basis(basis0)
    a = oracle_solve(first[0], 50)
    st3, npiv3, _ = eng.solve(50)
    assert (st3[0], npiv3[0]) == (a["status"], 50) == (cc.CAP_REACHED, 50)
    assert cc.same_bits(eng.download(0, 1)[0], a["T"])
    b = oracle_solve(a["T"])
    st4, npiv4, _ = eng.solve(CAP)
    assert (st4[0], npiv4[0]) == (b["status"], b["npiv"]) and cc.same_bits(eng.download(0, 1)[0], b["T"])
    eng.close()


# ---------------------------------------------------------------------------
# 7. ragged batches
# ---------------------------------------------------------------------------

def ragged_mix():
    """8x10 and 40x40 fit LDS, 100x100 and 120x90 do not; the 3 x 3 LP in front
    of the first device-placed LP makes that LP start at an odd double"""
    lps = [gen.tableau("mixed", 8, 10, 1), gen.tableau("mixed", 40, 40, 3), gen.tableau("tall", 2, 2, 1),
           gen.tableau("mixed", 100, 100, 1), gen.tableau("mixed", 120, 90, 2), gen.tableau("mixed", 8, 10, 2),
           gen.tableau("mixed", 100, 100, 2)]
    assert lps[2].size == 9 and sum(T.size for T in lps[:3]) % 2 == 1
    return lps


def test_ragged_auto():
    lps = ragged_mix()
    where = ["device" if _lib.batch_lds_bytes(*rc.shape_of(T)) > LDS else "lds" for T in lps]
    assert where == ["lds", "lds", "lds", "device", "device", "lds", "device"]
    basis0 = [np.full(T.shape[0] - 1, -1, dtype=np.int32) for T in lps]
    with pytest.raises(ValueError, match="LP 3 "):
        _lib.RaggedEngine([rc.shape_of(T) for T in lps])
    eng = _lib.RaggedEngine([rc.shape_of(T) for T in lps], log_cap=512, place="auto")
    assert [eng.placement(i) for i in range(len(lps))] == where
    plan = eng.plan()
    nt = dev_threads()
    assert plan[0]["waves"] * 64 == nt and plan[0]["lps"] == 3           # the device bin first
    assert plan[0]["lds_bytes"] == max(_lib.batch_device_lds_bytes(*rc.shape_of(lps[i])) for i in (3, 4, 6))
    assert plan[0]["lps_per_cu"] >= 1
    alone = _lib.RaggedEngine([rc.shape_of(lps[i]) for i in (0, 1, 2, 5)])
    assert plan[1:] == alone.plan()                                      # the others binned as a batch of their own
    alone.close()
    eng.upload(lps)
    eng.set_basis(basis0)
    st, npiv, nstd = eng.solve(CAP)
    got = records(eng, st, npiv, nstd, basis0)
    eng.close()
    check_stack(got, lps, basis0=basis0)                                 # caller order kept
    for i, T in enumerate(lps):                                          # a uniform placed batch of its own shape
        one = placed_solve(T[None], place="auto", basis=basis0[i][None], log_cap=512, expect=[where[i]])[0]
        check(got[i], one, what=f"LP {i}")
        assert got[i]["basis"] == one["basis"]
    res = solve_ragged([lps[i] for i in (0, 1, 3, 4)], place="auto", log_cap=512, max_pivots=CAP)
    for k, i in enumerate((0, 1, 3, 4)):
        assert res.status_code[k] == got[i]["status"] and res.log(k).tolist() == got[i]["log"]
        assert cc.same_bits(res.tableaux[k], got[i]["T"])
    assert res.plan()[0]["lps"] == 2


def test_ragged_forced_device_equals_lds():
    """the shapes of the ragged suites' mixture, plain solves: device memory and LDS give the same bits"""
    lps = rc.twophase_list() + [gen.tableau("mixed", 8, 10, 1), gen.tableau("mixed", 40, 40, 1)]
    cap = 64
    a = placed_solve(lps, place="device", cap=cap, log_cap=cap, expect=["device"] * len(lps))
    b = placed_solve(lps, place="lds", cap=cap, log_cap=cap, expect=["lds"] * len(lps))
    for i, (x, y) in enumerate(zip(a, b)):
        check(x, y, what=f"LP {i}")
        check(x, oracle_solve(lps[i], cap), what=f"LP {i}")
    assert sum(x["npiv"] for x in a) > 50


# ---------------------------------------------------------------------------
# 8. unchanged neighbours
# ---------------------------------------------------------------------------

def test_twophase_does_not_depend_on_placement():
    stack = np.stack([gen.phase1_lp("ge", 8, 10, s) for s in (1, 2, 3, 4)])
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    out = []
    for place in ("lds", "device"):
        eng = _lib.BatchEngine(4, m, n, log_cap=64, place=place)
        eng.upload(stack)
        res = eng.solve_lp(400)
        out.append([a.tolist() for a in res] + [eng.download().tobytes(), eng.get_basis().tolist(),
                                               [eng.log(i).tolist() for i in range(4)]])
        eng.close()
    assert out[0] == out[1]
    assert _lib.OPTIMAL in out[0][0] and max(out[0][3]) >= 1        # phase 1 did pivot


def test_twophase_refuses_above_lds_and_the_batch_stays_usable():
    stack = gen.mixed_stack(100, 100, (1, 2))
    eng = _lib.BatchEngine(2, 100, 200, log_cap=8, place="auto")
    eng.upload(stack)
    with pytest.raises(ValueError, match="too large"):
        eng.solve_lp(CAP)
    assert cc.same_bits(eng.download(), stack)
    st, npiv, nstd = eng.solve(CAP)
    out = eng.download()
    for i in range(2):
        w = oracle_solve(stack[i])
        assert (st[i], npiv[i], nstd[i]) == (w["status"], w["npiv"], w["nstd"]) and cc.same_bits(out[i], w["T"])
    eng.close()
    lps = [gen.tableau("mixed", 8, 10, 1), stack[0]]
    reng = _lib.RaggedEngine([rc.shape_of(T) for T in lps], place="auto")
    reng.upload(lps)
    with pytest.raises(ValueError, match="LP 1 "):
        reng.solve_lp(CAP)
    st, npiv, _ = reng.solve(CAP)
    assert npiv.tolist() == [oracle_solve(T)["npiv"] for T in lps]
    reng.close()


def test_place_lds_refuses_as_before():
    with pytest.raises(ValueError, match="too large"):
        _lib.BatchEngine(2, 100, 200, place="lds")
    with pytest.raises(ValueError, match="too large"):
        solve_batch(gen.mixed_stack(100, 100, (1,)), place="lds")
    with pytest.raises(ValueError, match="LP 1 "):
        _lib.RaggedEngine([(8, 18), (100, 200)], place="lds")
    eng = _lib.BatchEngine(2, 8, 18, place="lds")
    assert [eng.placement(i) for i in range(2)] == ["lds", "lds"]
    eng.close()
    eng = _lib.BatchEngine(2, 8, 18, place="auto")           # fits LDS: AUTO keeps it there
    assert [eng.placement(i) for i in range(2)] == ["lds", "lds"]
    assert _lib.ragged_plan(eng)[0]["lds_bytes"] == _lib.batch_lds_bytes(8, 18)
    eng.close()
