"""Phased batches (lp_phased_*, solve_lp_placed of BatchEngine / RaggedEngine,
place= of solve_lp_batch / solve_lp_ragged): the parts that need no GPU.

The C-ABI refuses bad requests before any device call, and the placement rule
and the plan of the two-phase call on a placed batch (csrc/batch_plan.h) are
pure functions: csrc/batch_phase_check.cpp drives them from stdin, built here
with -fsanitize=address,undefined and run as a child process, so a sanitizer
report fails the test that met it."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from lpsol_amd import _lib, solve_lp_batch, solve_lp_ragged
from lpsol_amd import generators as gen

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
LDS = 160 * 1024
ELEMS = 2048
WORK = 32 << 20             # LPK_BATCH_DEV_WORK of csrc/batch.hip
PHASED_SYMBOLS = {"lp_phased_solve", "lp_phased_lds_bytes", "lp_phased_placement", "lp_phased_plan"}
LDS_, AUTO, DEVICE = _lib.PLACE_LDS, _lib.PLACE_AUTO, _lib.PLACE_DEVICE
GE81 = (82, 163)            # phase1_lp("ge", 81, 81, s): plain LDS, phased device


# ---------------------------------------------------------------------------
# bindings and refusals without a device
# ---------------------------------------------------------------------------

def test_phased_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "lpgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(lp_phased_\w+)\s*\(", text)) == PHASED_SYMBOLS
    assert {s for s in _lib.EXPORTS if s.startswith("lp_phased_")} == PHASED_SYMBOLS
    for name in PHASED_SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    assert _lib._PROTOS["lp_phased_solve"] == _lib._PROTOS["lp_twophase_solve"]      # the same eight arguments
    for cls in (_lib.BatchEngine, _lib.RaggedEngine):
        for method in ("solve_lp_placed", "phased_placement", "plan_phased"):
            assert hasattr(cls, method)


def test_null_and_bad_arguments_are_refused():
    lib = _lib.load()
    st = np.zeros(2, dtype=np.int32)
    assert lib.lp_phased_solve(None, 10, st.ctypes.data_as(_lib._P32), None, None, None, None, None) == _lib.BAD_ARG
    p = ctypes.c_int(-9)
    assert lib.lp_phased_placement(None, 0, ctypes.byref(p)) == _lib.BAD_ARG and p.value == -9
    cnt = ctypes.c_int64(-9)
    assert lib.lp_phased_plan(None, None, 0, ctypes.byref(cnt)) == _lib.BAD_ARG and cnt.value == -9
    for m, n in [(0, 4), (4, 0), (-1, -1)]:
        assert lib.lp_phased_lds_bytes(m, n) == _lib.BAD_ARG


def test_lds_bytes_equal_the_python_formula():
    lib = _lib.load()
    for m in (1, 2, 7, 8, 82, 90, 91, 116, 257, 1100, 8000, (1 << 20) - 1):
        for n in (1, 2, 8, 60, 128, 163, 513, 4000):
            want = ((n + 1 + m) + (m + 1) + 16 + (m + 1) // 2) * 8
            assert _lib.phased_lds_bytes(m, n) == want == lib.lp_phased_lds_bytes(m, n), (m, n)
    assert lib.lp_phased_lds_bytes(1 << 20, 4) > LDS                # no formula is evaluated: never fits
    assert _lib.phased_lds_bytes(*GE81) == (246 + 83 + 16 + 41) * 8 == 3088
    assert _lib.twophase_lds_bytes(*GE81) == 167104 > LDS >= _lib.batch_lds_bytes(*GE81)


@pytest.mark.parametrize("place", ["bogus", "LDS", "", None, 1])
def test_an_unknown_place_raises_without_a_device(place):
    stack = np.stack([gen.phase1_lp("ge", 5, 6, s) for s in (1, 2)])
    with pytest.raises(ValueError, match="place"):
        solve_lp_batch(stack, place=place)
    with pytest.raises(ValueError, match="place"):
        solve_lp_ragged(list(stack), place=place)


def test_phased_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    T = gen.phase1_lp("ge", 81, 81, 1)
    for place in ("auto", "device"):
        with pytest.raises(_lib.EngineUnavailable):
            solve_lp_batch(T[None], place=place)
        with pytest.raises(_lib.EngineUnavailable):
            solve_lp_ragged([gen.phase1_lp("ge", 5, 6, 1), T], place=place)


# ---------------------------------------------------------------------------
# the rule and the plan under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_phase_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_phase_check")
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


def parse_plan(line):
    f = fields(line)
    bins = []
    for b in filter(None, f["bins"].split(";")):
        d, w, lds, per, order = b.split(":")
        bins.append(dict(device=int(d), waves=int(w), lds=int(lds), per_cu=int(per),
                         order=[int(x) for x in order.split(".")]))
    return int(f["too_large"]), bins


def shapes_arg(shapes):
    return ",".join("%d:%d" % s for s in shapes)


def plan_line(place, shapes, cap1=32, cap4=8, dwaves=16, dcap=1):
    return "plan place=%d cap1=%d cap4=%d elems=%d dwaves=%d dcap=%d shapes=%s" % (
        place, cap1, cap4, ELEMS, dwaves, dcap, shapes_arg(shapes))


def ragged_line(shapes, cap1=32, cap4=8):
    return "ragged cap1=%d cap4=%d elems=%d shapes=%s" % (cap1, cap4, ELEMS, shapes_arg(shapes))


def want_where(place, m, n):
    """the Python restatement of plan_place_phased"""
    if place not in (LDS_, AUTO, DEVICE):
        return -1
    valid = m < (1 << 20) and n < (1 << 20)
    fits = valid and _lib.twophase_lds_bytes(m, n) <= LDS
    dfits = valid and _lib.phased_lds_bytes(m, n) <= LDS
    if place != DEVICE and fits:
        return LDS_
    if place == LDS_:
        return -2
    return DEVICE if dfits else -2


def test_place_rule(check):
    # 90 | 91 at n = 128, 81 | 82 at n = 163 and 113 | 114 at n = 60 straddle 160 KiB for
    # plan_twophase_lds; (8184, 1) | (8185, 1) straddle it for plan_phased_lds
    grid = [(m, n) for m in (1, 8, 81, 82, 90, 91, 113, 114, 116, 256, 1100, 8184, 8185, 1 << 20)
            for n in (1, 8, 60, 128, 161, 163, 512, 4000)]
    assert _lib.twophase_lds_bytes(90, 128) <= LDS < _lib.twophase_lds_bytes(91, 128)
    assert _lib.twophase_lds_bytes(81, 163) <= LDS < _lib.twophase_lds_bytes(82, 163)
    assert _lib.twophase_lds_bytes(113, 60) <= LDS < _lib.twophase_lds_bytes(114, 60)
    assert _lib.phased_lds_bytes(8184, 1) <= LDS < _lib.phased_lds_bytes(8185, 1)
    places = (LDS_, AUTO, DEVICE, 5)
    got = check(["place place=%d m=%d n=%d" % (p, m, n) for p in places for m, n in grid])
    k = 0
    for p in places:
        for m, n in grid:
            f = {a: int(b) for a, b in fields(got[k]).items()}
            k += 1
            if m < (1 << 20):
                assert f["tplds"] == _lib.twophase_lds_bytes(m, n) and f["phlds"] == _lib.phased_lds_bytes(m, n)
            want = want_where(p, m, n)
            assert f["where"] == want, (p, m, n)
            if m < (1 << 20) and p != 5:
                assert (want == -2) == _lib.phased_too_large(p, m, n), (p, m, n)
                if want >= 0:
                    assert (want == DEVICE) == _lib.phased_on_device(p, m, n), (p, m, n)
    # ge(81, 81): LDS-placed for the plain call, device-placed for the phased one
    f = {a: int(b) for a, b in fields(check(["place place=%d m=%d n=%d" % (AUTO, *GE81)])[0]).items()}
    assert (f["plain"], f["where"]) == (LDS_, DEVICE)


def test_phased_chunk(check):
    cases = [(4096, WORK, 82, 163), (4096, WORK, 116, 60), (4096, WORK, 257, 513), (1, WORK, 82, 163),
             (7, WORK, 116, 60), (4096, 1000, 82, 163), (4096, WORK, 8184, 1)]
    got = check(["chunk chunk=%d work=%d m=%d n=%d" % c for c in cases])
    for (chunk, w, m, n), ln in zip(cases, got):
        assert int(fields(ln)["pivots"]) == max(1, min(chunk, w // ((m + 1) * (n + 1 + m))))
    assert [int(fields(ln)["pivots"]) for ln in got] == [1643, 1620, 168, 1, 7, 1, 1]


def random_shapes(rng):
    out = []
    for _ in range(rng.randint(1, 40)):
        pick = rng.random()
        if pick < 0.35:
            out.append((rng.randint(1, 12), rng.randint(1, 24)))
        elif pick < 0.6:
            out.append((rng.randint(1, 70), rng.randint(1, 140)))
        elif pick < 0.75:                       # around the two-phase LDS bound at n = 128, 163, 60
            out.append(rng.choice([(90, 128), (91, 128), (81, 163), (82, 163), (113, 60), (114, 60)]))
        elif pick < 0.95:
            out.append((rng.randint(1, 400), rng.randint(1, 600)))
        else:
            out.append((rng.randint(1, 9000), rng.randint(1, 8000)))
    return out


def test_random_lists_auto_and_device(check):
    rng = random.Random(4111)
    requests = []
    for k in range(1500):
        place = AUTO if k % 4 else DEVICE
        shapes = [s for s in random_shapes(rng) if _lib.phased_lds_bytes(*s) <= LDS]
        if not shapes:
            shapes = [(8, 18)]
        if k % 5 == 0:
            shapes.insert(rng.randrange(len(shapes) + 1), GE81)
        caps = (32, 8, 16, 1) if k % 3 else (rng.randint(1, 40), rng.randint(1, 10), rng.choice((8, 16)),
                                             rng.randint(1, 8))
        requests.append((place, shapes, caps))
    lines = []
    for place, shapes, (c1, c4, dw, dc) in requests:
        lines.append(plan_line(place, shapes, c1, c4, dw, dc))
        lds_only = [s for s in shapes if place == AUTO and _lib.twophase_lds_bytes(*s) <= LDS]
        lines.append(ragged_line(lds_only or [(1, 1)], c1, c4))
    got = check(lines)
    some_dev = some_both = 0
    for k, (place, shapes, (c1, c4, dw, dc)) in enumerate(requests):
        too_large, bins = parse_plan(got[2 * k])
        assert too_large == -1
        want_dev = [i for i, s in enumerate(shapes) if want_where(place, *s) == DEVICE]
        assert sorted(i for b in bins for i in b["order"]) == list(range(len(shapes)))     # each LP in one bin
        for b in bins:
            assert b["order"] == sorted(b["order"])                 # ascending inside a bin
        dev = [b for b in bins if b["device"]]
        assert len(dev) == (1 if want_dev else 0)
        if dev:
            assert bins[0] is dev[0]                                # the device bin comes first
            assert dev[0]["order"] == want_dev
            assert dev[0]["waves"] == dw
            assert dev[0]["lds"] == max(_lib.phased_lds_bytes(*shapes[i]) for i in want_dev)
            assert dev[0]["per_cu"] == min(dc, LDS // dev[0]["lds"]) >= 1
            some_dev += 1
        # the LDS-placed LPs: plan_ragged's two-phase bins of a batch of their own, indices mapped back
        lds_at = [i for i in range(len(shapes)) if i not in set(want_dev)]
        rest = [b for b in bins if not b["device"]]
        if lds_at:
            _, alone = parse_plan(got[2 * k + 1])
            assert [dict(b, order=[lds_at[i] for i in b["order"]]) for b in alone] == rest
            some_both += bool(dev)
        else:
            assert rest == []
    assert some_dev > 200 and some_both > 200


def test_all_lds_input_gives_the_two_phase_plan_unchanged(check):
    rng = random.Random(8)
    lists = []
    while len(lists) < 200:
        shapes = [s for s in random_shapes(rng) if _lib.twophase_lds_bytes(*s) <= LDS]
        if shapes:
            lists.append(shapes)
    lines = []
    for shapes in lists:
        lines += [plan_line(AUTO, shapes), plan_line(LDS_, shapes), ragged_line(shapes)]
    got = check(lines)
    for k in range(len(lists)):
        assert got[3 * k] == got[3 * k + 1] == got[3 * k + 2]
        assert all(not b["device"] for b in parse_plan(got[3 * k])[1])


def test_pinned_plans(check):
    mixed = [(8, 18), GE81, (6, 12), (116, 60), (40, 50)]
    got = [parse_plan(ln) for ln in check([plan_line(AUTO, mixed), plan_line(DEVICE, mixed), plan_line(LDS_, mixed),
                                           plan_line(AUTO, [(8, 18), (8185, 1)]),
                                           plan_line(AUTO, [GE81] * 3, dwaves=8, dcap=4),
                                           plan_line(7, mixed)])]
    ge81, dep = (246 + 83 + 16 + 41) * 8, (177 + 117 + 16 + 58) * 8
    assert (ge81, dep) == (3088, 2944)
    too_large, bins = got[0]
    assert too_large == -1
    assert bins[0] == dict(device=1, waves=16, lds=ge81, per_cu=1, order=[1, 3])
    assert sorted(i for b in bins[1:] for i in b["order"]) == [0, 2, 4]
    assert [b["lds"] for b in bins[1:]] == sorted((b["lds"] for b in bins[1:]), reverse=True)
    assert bins[1]["lds"] == _lib.twophase_lds_bytes(40, 50) and bins[1]["waves"] == 4
    assert got[1] == (-1, [dict(device=1, waves=16, lds=ge81, per_cu=1, order=[0, 1, 2, 3, 4])])
    assert got[2] == (1, [])                    # LDS only: the first LP whose widened tableau does not fit
    assert got[3] == (1, [])                    # above the device bound as well
    assert got[4] == (-1, [dict(device=1, waves=8, lds=ge81, per_cu=4, order=[0, 1, 2])])
    assert got[5] == (0, [])                    # an unknown place is refused at the first LP
