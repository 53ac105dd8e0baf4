"""Teamed batches (lp_teamed_*, team= of BatchEngine / RaggedEngine /
solve_batch / solve_ragged): the parts that need no GPU.

The C-ABI refuses a bad team request before any device call, and the team
size, the ranges of a team and the workgroup table of csrc/batch_plan.h are
pure functions: csrc/batch_team_check.cpp drives them from stdin, built here
with -fsanitize=address,undefined and run as a child process, so a sanitizer
report fails the test that met it."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from lpsol_amd import _lib, solve_batch, solve_ragged
from lpsol_amd import generators as gen

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
NO_DEVICE = 1 << 20         # exists nowhere: a refusal with it comes before any device call
TEAMED_SYMBOLS = {"lp_teamed_create", "lp_teamed_create_ragged", "lp_teamed_size", "lp_teamed_plan",
                  "lp_teamed_set_window"}
LDS_, AUTO, DEVICE = _lib.PLACE_LDS, _lib.PLACE_AUTO, _lib.PLACE_DEVICE


def knob(name):
    text = open(os.path.join(CSRC, "knobs.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


TEAM_MAX, MIN_ELEMS, LP_ELEMS = knob("LPK_TEAM_MAX"), knob("LPK_TEAM_MIN_ELEMS"), knob("LPK_TEAM_LP_ELEMS")


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_teamed_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpgpu.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(lp_teamed_\w+)\s*\(", text)) == TEAMED_SYMBOLS
    assert {s for s in _lib.EXPORTS if s.startswith("lp_teamed_")} == TEAMED_SYMBOLS
    for name in TEAMED_SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        assert inspect.signature(cls.__init__).parameters["team"].default == 1
        assert hasattr(cls, "team_of") and hasattr(cls, "team_plan") and hasattr(cls, "set_window")
    for fn in (solve_batch, solve_ragged):
        assert inspect.signature(fn).parameters["team"].default == 1
    assert knob("LPK_TEAM_WAVES") in (4, 8, 16) and TEAM_MAX >= 2 and MIN_ELEMS >= 2 and knob("LPK_TEAM_WINDOW") >= 1


# ---------------------------------------------------------------------------
# refusals without a device
# ---------------------------------------------------------------------------

def create(count, m, n, place, team):
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    st = lib.lp_teamed_create(count, m, n, 0, NO_DEVICE, place, team, ctypes.byref(h))
    return st, h.value, lib.lp_batch_last_error(None).decode()


def create_ragged(shapes, place, teams):
    lib = _lib.load()
    m = np.array([s[0] for s in shapes], dtype=np.int64)
    n = np.array([s[1] for s in shapes], dtype=np.int64)
    t = None if teams is None else np.array(teams, dtype=np.int32).ctypes.data_as(_lib._P32)
    h = ctypes.c_void_p(1)
    st = lib.lp_teamed_create_ragged(len(shapes), m.ctypes.data_as(_lib._P64), n.ctypes.data_as(_lib._P64), 0,
                                     NO_DEVICE, place, t, ctypes.byref(h))
    return st, h.value, lib.lp_batch_last_error(None).decode()


def test_a_team_needs_a_device_placed_lp():
    st, h, msg = create(4, 100, 200, LDS_, 2)
    assert st == _lib.BAD_ARG and not h and "team" in msg and "LP_PLACE_LDS" in msg
    st, h, msg = create(4, 8, 18, LDS_, 2)
    assert st == _lib.BAD_ARG and not h and "team" in msg
    st, h, msg = create_ragged([(8, 18), (100, 200)], LDS_, [1, 3])
    assert st == _lib.BAD_ARG and not h and "LP 1:" in msg and "team" in msg
    for place in (AUTO, DEVICE):            # the same requests pass the checks and reach the device
        assert create(4, 100, 200, place, 2)[0] == _lib.DEVICE_ERROR
        assert create(4, 8, 18, place, 2)[0] == _lib.DEVICE_ERROR
        assert create_ragged([(8, 18), (100, 200)], place, [1, 3])[0] == _lib.DEVICE_ERROR
    with pytest.raises(ValueError, match="team"):
        _lib.BatchEngine(2, 100, 200, place="lds", team=2)
    with pytest.raises(ValueError, match="LP 0:"):
        _lib.RaggedEngine([(100, 200)], place="lds", team=2)
    with pytest.raises(ValueError, match="team"):
        solve_batch(gen.mixed_stack(8, 10, [1]), place="lds", team=2)
    with pytest.raises(ValueError, match="team"):
        solve_ragged([gen.tableau("mixed", 8, 10, 1)], team=[4])


@pytest.mark.parametrize("place", [AUTO, DEVICE])
def test_a_team_above_the_caps_is_refused(place):
    st, h, msg = create(2, 100, 200, place, TEAM_MAX + 1)
    assert st == _lib.BAD_ARG and not h and "largest team" in msg
    assert create(2, 100, 200, place, TEAM_MAX)[0] == _lib.DEVICE_ERROR
    # E = 3 x 5 = 15: seven workgroups have a pair each, eight do not
    assert 8 <= TEAM_MAX
    assert create(2, 2, 4, place, 7)[0] == _lib.DEVICE_ERROR
    st, h, msg = create(2, 2, 4, place, 8)
    assert st == _lib.BAD_ARG and not h and "(m+1)(n+1) / 2" in msg
    st, h, msg = create_ragged([(100, 200), (2, 4), (1, 1)], place, [2, 7, 3])
    assert st == _lib.BAD_ARG and not h and "LP 2:" in msg and "(m+1)(n+1) / 2" in msg
    assert create_ragged([(100, 200), (2, 4), (1, 1)], place, [2, 7, 2])[0] == _lib.DEVICE_ERROR
    st, h, msg = create(2, 100, 200, place, -1)
    assert st == _lib.BAD_ARG and not h and "team" in msg
    name = "auto" if place == AUTO else "device"
    with pytest.raises(ValueError, match="largest team"):
        _lib.BatchEngine(2, 100, 200, place=name, team=TEAM_MAX + 1)
    with pytest.raises(ValueError, match=r"\(m\+1\)\(n\+1\) / 2"):
        _lib.BatchEngine(2, 2, 4, place=name, team=8)
    with pytest.raises(ValueError, match="LP 1:"):
        _lib.RaggedEngine([(100, 200), (2, 4)], place=name, team=8)
    with pytest.raises(ValueError, match="largest team"):
        solve_batch(gen.mixed_stack(100, 100, [1]), place=name, team=TEAM_MAX + 1)


def test_team_one_is_the_placed_call():
    """what lp_placed_create refuses, lp_teamed_create refuses with the same message, at team 1, auto and forced"""
    lib = _lib.load()
    h = ctypes.c_void_p()
    for count, m, n, place in [(0, 8, 18, AUTO), (4, 0, 18, DEVICE), (4, 8, 18, 7), (4, 100, 200, LDS_),
                               (1, 10232, 10231, AUTO)]:
        assert lib.lp_placed_create(count, m, n, 0, NO_DEVICE, place, ctypes.byref(h)) == _lib.BAD_ARG
        old = lib.lp_batch_last_error(None).decode()
        for team in (1, 0) + ((2,) if place != LDS_ else ()):
            st, hv, msg = create(count, m, n, place, team)
            assert st == _lib.BAD_ARG and not hv and msg == old, (count, m, n, place, team)
    assert create(4, 100, 200, AUTO, 1)[0] == create(4, 100, 200, AUTO, 0)[0] == _lib.DEVICE_ERROR
    assert create_ragged([(8, 18), (100, 200)], AUTO, None)[0] == _lib.DEVICE_ERROR
    st, hv, msg = create_ragged([(8, 18), (100, 200)], LDS_, None)
    assert st == _lib.BAD_ARG and "LP 1 " in msg and "too large" in msg


def test_python_team_argument():
    assert _lib.team_code(1) == 1 and _lib.team_code(7) == 7 and _lib.team_code("auto") == 0
    for bad in (0, -2, "all", 2.0, None, True):
        with pytest.raises(ValueError, match="team"):
            _lib.team_code(bad)
    with pytest.raises(ValueError, match="team"):
        _lib.BatchEngine(1, 8, 18, place="device", team=0)
    with pytest.raises(ValueError, match="one request per LP"):
        _lib.RaggedEngine([(8, 18), (9, 9)], place="device", team=[2])


def test_teamed_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    T = gen.tableau("mixed", 100, 100, 1)
    for team in (2, "auto"):
        with pytest.raises(_lib.EngineUnavailable):
            solve_batch(T[None], place="auto", team=team)
        with pytest.raises(_lib.EngineUnavailable):
            solve_ragged([gen.tableau("mixed", 8, 10, 1), T], place="auto", team=team)
        with pytest.raises(_lib.EngineUnavailable):
            _lib.BatchEngine(2, 100, 200, place="device", team=team)


def test_null_batch_is_refused():
    lib = _lib.load()
    g = ctypes.c_int(-9)
    assert lib.lp_teamed_size(None, 0, ctypes.byref(g)) == _lib.BAD_ARG and g.value == -9
    assert lib.lp_teamed_plan(None, None, 0, None) == _lib.BAD_ARG
    assert lib.lp_teamed_set_window(None, 4) == _lib.BAD_ARG


# ---------------------------------------------------------------------------
# the team rules under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_team_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_team_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def fields(line):
    return dict(kv.split("=") for kv in line.split())


def size_line(request, ndev, m, n, slots=512, mx=64, mn=4096, lpe=0):
    return "size request=%d ndev=%d m=%d n=%d slots=%d max=%d min=%d lpe=%d" % (request, ndev, m, n, slots, mx, mn, lpe)


def sizes(check, requests):
    return [int(fields(ln)["team"]) for ln in check([size_line(*r) for r in requests])]


def ranges(check, E, toff, G):
    ends = [int(x) for x in fields(check(["ranges E=%d toff=%d G=%d" % (E, toff, G)])[0])["ends"].split(".")]
    return list(zip(ends[:-1], ends[1:]))


def test_ranges_cover_every_lp_exactly_once(check):
    """every E in 2..600 x toff parity x G in 1..min(64, E/2): the ranges cover
    [0, E) in order, none empty, interior ends at even toff + e, pair counts
    within one of each other"""
    f = fields(check(["sweep Emax=600 Gmax=64"])[0])
    want = 2 * sum(min(64, E // 2) for E in range(2, 601))
    assert (int(f["checked"]), int(f["bad"])) == (want, 0)


def test_pinned_ranges(check):
    # cfg1, E = 171: an even base, then the odd base of the LP behind it
    assert ranges(check, 171, 0, 2) == [(0, 86), (86, 171)]
    assert ranges(check, 171, 171, 2) == [(0, 85), (85, 171)]
    assert ranges(check, 171, 0, 3) == [(0, 56), (56, 114), (114, 171)]
    assert ranges(check, 171, 171, 7) == [(0, 23), (23, 47), (47, 71), (71, 97), (97, 121), (121, 145), (145, 171)]
    assert ranges(check, 4, 1, 2) == [(0, 1), (1, 4)]               # three pairs, two of them halves
    assert ranges(check, 4, 0, 2) == [(0, 2), (2, 4)]
    assert ranges(check, 2, 1, 1) == [(0, 2)]
    assert ranges(check, 132353, 0, 16)[0] == (0, 8272) and ranges(check, 132353, 0, 16)[-1][1] == 132353


def test_forced_sizes_and_refusals(check):
    got = sizes(check, [(1, 4, 100, 200), (2, 4, 100, 200), (64, 4, 100, 200), (65, 4, 100, 200),
                        (7, 1, 2, 4), (8, 1, 2, 4), (2, 1, 1, 1), (3, 1, 1, 1), (-1, 1, 8, 18),
                        (2, 1, 0, 18), (2, 1, 1 << 20, 4), (1, 1, 1, 1), (16, 9999, 256, 512, 1)])
    assert got == [1, 2, 64, -1, 7, -1, 2, -1, -1, -1, -1, 1, 16]
    # a forced team does not look at the chip or at the other LPs
    assert sizes(check, [(5, nd, 100, 200, s) for nd in (1, 600) for s in (0, 512)]) == [5] * 4


def test_auto_rule(check):
    E = lambda m, n: (m + 1) * (n + 1)
    cases = [(nd, m, n, slots, mx, mn, lpe) for nd in (1, 2, 3, 4, 16, 64, 255, 256, 257, 512, 4096)
             for m, n in ((100, 200), (150, 300), (256, 512), (512, 1024), (8, 18), (1, 1))
             for slots, mx, mn, lpe in ((512, 64, 4096, 0), (256, 16, 8192, 0), (512, 64, 2, 0), (0, 64, 4096, 0),
                                        (1024, 32, 1024, 1500), (1024, 32, 2, 1))]
    got = sizes(check, [(0,) + c for c in cases])
    for (nd, m, n, slots, mx, mn, lpe), g in zip(cases, got):
        want = 1 if lpe and nd > E(m, n) // lpe else max(1, min(slots // nd, E(m, n) // mn, mx))
        assert g == want, (nd, m, n, slots, mx, mn, lpe)
        assert 1 <= g <= max(1, E(m, n) // 2)
    # never more workgroups per LP when more LPs share the chip
    by = {}
    for (nd, *rest), g in zip(cases, got):
        by.setdefault(tuple(rest), []).append(g)
    assert all(v == sorted(v, reverse=True) for v in by.values())
    assert any(v[0] > v[-1] for v in by.values())
    # 4 LPs of mixed 100x100 get a team; 4096 of them fill the chip alone and get none
    four, many = sizes(check, [(0, 4, 100, 200, 1024, TEAM_MAX, MIN_ELEMS, LP_ELEMS),
                               (0, 4096, 100, 200, 1024, TEAM_MAX, MIN_ELEMS, LP_ELEMS)])
    assert 4 <= 101 * 201 // LP_ELEMS and four == max(1, min(256, 101 * 201 // MIN_ELEMS, TEAM_MAX)) > 1
    assert many == 1


def test_workgroup_table(check):
    shapes = [(8, 18), (2, 2), (100, 200), (8, 18), (40, 80), (1, 1)]
    teams = [3, 1, 5, 0, 2, 2]
    line = "table shapes=%s teams=%s" % (",".join("%d:%d" % s for s in shapes), ",".join(map(str, teams)))
    rows = [tuple(int(x) for x in w.split(":")) for w in fields(check([line])[0])["wgs"].split(";")]
    assert [r[0] for r in rows] == [0] * 3 + [2] * 5 + [4] * 2 + [5] * 2           # teamed LPs ascending
    toff = np.concatenate([[0], np.cumsum([(m + 1) * (n + 1) for m, n in shapes])])
    assert toff[2] % 2 == 0 and toff[5] % 2 == 1
    for lp in (0, 2, 4, 5):
        mine = [r for r in rows if r[0] == lp]
        assert [r[1] for r in mine] == list(range(teams[lp])) and {r[2] for r in mine} == {teams[lp]}
        E = (shapes[lp][0] + 1) * (shapes[lp][1] + 1)
        assert [(r[3], r[4]) for r in mine] == ranges(check, E, int(toff[lp]), teams[lp])
    assert fields(check(["table shapes=8:18 teams=1"])[0])["wgs"] == ""
