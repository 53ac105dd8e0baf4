"""Placed batches (lp_placed_*, place= of BatchEngine / RaggedEngine /
solve_batch / solve_ragged): the parts that need no GPU.

The C-ABI refuses bad requests before any device call, and the placement rule
and the placed launch plan of csrc/batch_plan.h are pure functions:
csrc/batch_place_check.cpp drives them from stdin, built here with
-fsanitize=address,undefined and run as a child process, so a sanitizer report
fails the test that met it."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from lpsol_amd import _lib, solve_batch, solve_ragged
from lpsol_amd import generators as gen

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
LDS = 160 * 1024
ELEMS = 2048
NO_DEVICE = 1 << 20         # exists nowhere: a refusal with it comes before any device call
PLACED_SYMBOLS = {"lp_placed_create", "lp_placed_create_ragged", "lp_placed_placement", "lp_placed_lds_bytes"}
LDS_, AUTO, DEVICE = _lib.PLACE_LDS, _lib.PLACE_AUTO, _lib.PLACE_DEVICE


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------

def test_placed_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "lpgpu.h")).read()
    assert [int(re.search(r"#define\s+LP_PLACE_%s\s+(\d+)" % k, text).group(1)) for k in ("LDS", "AUTO", "DEVICE")] \
        == [LDS_, AUTO, DEVICE] == [0, 1, 2]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(lp_placed_\w+)\s*\(", text)) == PLACED_SYMBOLS
    assert PLACED_SYMBOLS <= set(_lib.EXPORTS)
    for name in PLACED_SYMBOLS:
        fn = getattr(lib, name)
        res, argt = _lib._PROTOS[name]
        assert fn.restype is res and list(fn.argtypes) == list(argt), name
    assert hasattr(_lib.BatchEngine, "placement")
    assert _lib.PLACES == {"lds": 0, "auto": 1, "device": 2}


# ---------------------------------------------------------------------------
# refusals without a device
# ---------------------------------------------------------------------------

def create(count, m, n, place, log_cap=0):
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    st = lib.lp_placed_create(count, m, n, log_cap, NO_DEVICE, place, ctypes.byref(h))
    return st, h.value, lib.lp_batch_last_error(None).decode()


def create_ragged(shapes, place, log_cap=0):
    lib = _lib.load()
    m = np.array([s[0] for s in shapes], dtype=np.int64)
    n = np.array([s[1] for s in shapes], dtype=np.int64)
    h = ctypes.c_void_p(1)
    st = lib.lp_placed_create_ragged(len(shapes), m.ctypes.data_as(_lib._P64), n.ctypes.data_as(_lib._P64), log_cap,
                                     NO_DEVICE, place, ctypes.byref(h))
    return st, h.value, lib.lp_batch_last_error(None).decode()


@pytest.mark.parametrize("place", [-1, 3, 7])
def test_an_unknown_place_is_refused(place):
    st, h, msg = create(4, 8, 18, place)
    assert st == _lib.BAD_ARG and not h and "place" in msg
    st, h, msg = create_ragged([(8, 18), (16, 32)], place)
    assert st == _lib.BAD_ARG and not h and "place" in msg
    with pytest.raises(ValueError, match="place"):
        _lib.BatchEngine(1, 8, 18, place="hbm")
    with pytest.raises(ValueError, match="place"):
        _lib.RaggedEngine([(8, 18)], place="")
    with pytest.raises(ValueError, match="place"):
        solve_batch(gen.mixed_stack(8, 10, [1]), place="LDS")


@pytest.mark.parametrize("place", [LDS_, AUTO, DEVICE])
@pytest.mark.parametrize("count,m,n,log_cap", [(0, 8, 18, 0), (4, 0, 18, 0), (4, 8, -1, 0), (4, 8, 18, -1)])
def test_what_the_old_calls_refuse_is_refused(place, count, m, n, log_cap):
    st, h, msg = create(count, m, n, place, log_cap)
    assert st == _lib.BAD_ARG and not h and "count > 0" in msg
    st, h, msg = create_ragged([(8, 18), (0, 3)], place)
    assert st == _lib.BAD_ARG and not h and "LP 1:" in msg
    lib = _lib.load()
    assert lib.lp_placed_create(1, 8, 18, 0, NO_DEVICE, place, None) == _lib.BAD_ARG         # out is NULL
    assert lib.lp_placed_create_ragged(1, None, None, 0, NO_DEVICE, place, ctypes.byref(ctypes.c_void_p())) \
        == _lib.BAD_ARG


def test_place_lds_refuses_as_lp_batch_create_does():
    lib = _lib.load()
    T = gen.tableau("mixed", 100, 100, 1)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    assert (m, n) == (100, 200) and _lib.batch_lds_bytes(m, n) == 164952 > LDS
    h = ctypes.c_void_p()
    assert lib.lp_batch_create(4, m, n, 0, NO_DEVICE, ctypes.byref(h)) == _lib.BAD_ARG
    old = lib.lp_batch_last_error(None).decode()
    st, h, msg = create(4, m, n, LDS_)
    assert st == _lib.BAD_ARG and not h
    assert msg == old and "too large" in msg and "use lp_create" in msg
    # ragged: the same message as lp_ragged_create, with the LP's index
    ms = np.array([8, m], dtype=np.int64)
    ns = np.array([18, n], dtype=np.int64)
    hh = ctypes.c_void_p()
    assert lib.lp_ragged_create(2, ms.ctypes.data_as(_lib._P64), ns.ctypes.data_as(_lib._P64), 0, NO_DEVICE,
                                ctypes.byref(hh)) == _lib.BAD_ARG
    old = lib.lp_batch_last_error(None).decode()
    st, h, msg = create_ragged([(8, 18), (m, n)], LDS_)
    assert st == _lib.BAD_ARG and msg == old and "too large" in msg and "LP 1 " in msg
    # the other two requests take the shape: the argument checks pass and the call reaches the device
    for place in (AUTO, DEVICE):
        assert create(4, m, n, place)[0] == _lib.DEVICE_ERROR
        assert create_ragged([(8, 18), (m, n)], place)[0] == _lib.DEVICE_ERROR
    with pytest.raises(ValueError, match="too large"):
        _lib.BatchEngine(4, m, n)
    with pytest.raises(ValueError, match="too large"):
        _lib.BatchEngine(4, m, n, place="lds")
    with pytest.raises(ValueError, match="too large"):
        solve_batch(T[None])
    with pytest.raises(ValueError, match="too large"):
        solve_ragged([gen.tableau("mixed", 8, 10, 1), T])


def test_the_side_buffer_bound():
    """(n+1) + (m+1) + 16 doubles of LDS: m + n = 20462 is the last sum that fits"""
    lib = _lib.load()
    assert lib.lp_placed_lds_bytes(0, 4) == _lib.BAD_ARG
    for m, n in [(1, 1), (100, 200), (1100, 1160), (10231, 10231), (10232, 10231), (1 << 20, 1)]:
        want = ((n + 1) + (m + 1) + 16) * 8
        assert _lib.batch_device_lds_bytes(m, n) == want
        if m < (1 << 20):
            assert lib.lp_placed_lds_bytes(m, n) == want
    below, above = (10231, 10231), (10232, 10231)
    assert _lib.batch_device_lds_bytes(*below) == LDS < _lib.batch_device_lds_bytes(*above)
    for place in (AUTO, DEVICE):
        assert create(1, *below, place)[0] == _lib.DEVICE_ERROR        # passes the checks, reaches the device
        st, h, msg = create(1, *above, place)
        assert st == _lib.BAD_ARG and not h and "too large" in msg
        st, h, msg = create(1, 1 << 20, 4, place)
        assert st == _lib.BAD_ARG and "too large" in msg
        assert create_ragged([(8, 18), below, (20000, 461)], place)[0] == _lib.DEVICE_ERROR
        st, h, msg = create_ragged([(8, 18), below, above, (30000, 4)], place)
        assert st == _lib.BAD_ARG and not h and "too large" in msg and "LP 2 " in msg
        name = _lib.PLACE_NAMES.get(place, "auto")
        with pytest.raises(ValueError, match="too large"):
            _lib.BatchEngine(1, *above, place=name)
        with pytest.raises(ValueError, match="LP 1 "):
            _lib.RaggedEngine([(8, 18), above], place=name)
    # forced device placement does not care whether the LP would fit LDS
    assert create(1, 8, 18, DEVICE)[0] == _lib.DEVICE_ERROR


def test_placed_calls_have_no_host_fallback():
    if _lib.device_count() > 0:
        return                                  # a GPU is visible: nothing to refuse
    T = gen.tableau("mixed", 100, 100, 1)
    for place in ("auto", "device"):
        with pytest.raises(_lib.EngineUnavailable):
            solve_batch(T[None], place=place)
        with pytest.raises(_lib.EngineUnavailable):
            solve_ragged([gen.tableau("mixed", 8, 10, 1), T], place=place)
        with pytest.raises(_lib.EngineUnavailable):
            _lib.BatchEngine(2, 100, 200, place=place)


def test_null_batch_is_refused():
    lib = _lib.load()
    p = ctypes.c_int(-9)
    assert lib.lp_placed_placement(None, 0, ctypes.byref(p)) == _lib.BAD_ARG and p.value == -9


# ---------------------------------------------------------------------------
# the placement rule and the placed plan under the host sanitizers
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_place_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_place_check")
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


def plan_line(place, shapes, cap1=32, cap4=8, dwaves=16, dcap=2):
    return "plan place=%d cap1=%d cap4=%d elems=%d dwaves=%d dcap=%d shapes=%s" % (
        place, cap1, cap4, ELEMS, dwaves, dcap, shapes_arg(shapes))


def ragged_line(shapes, cap1=32, cap4=8):
    return "ragged cap1=%d cap4=%d elems=%d shapes=%s" % (cap1, cap4, ELEMS, shapes_arg(shapes))


def test_place_rule(check):
    grid = [(m, n) for m in (1, 8, 64, 100, 155, 156, 256, 1100, 10231, 10232, 1 << 20)
            for n in (1, 18, 128, 200, 512, 1160, 10231)]
    got = check(["place place=%d m=%d n=%d" % (p, m, n) for p in (LDS_, AUTO, DEVICE, 5) for m, n in grid])
    k = 0
    for p in (LDS_, AUTO, DEVICE, 5):
        for m, n in grid:
            f = {a: int(b) for a, b in fields(got[k]).items()}
            k += 1
            valid = m < (1 << 20)
            fits = valid and _lib.batch_lds_bytes(m, n) <= LDS
            dfits = valid and _lib.batch_device_lds_bytes(m, n) <= LDS
            if valid:
                assert f["lds"] == _lib.batch_lds_bytes(m, n) and f["devlds"] == _lib.batch_device_lds_bytes(m, n)
            if p == 5:
                want = -1
            elif p == LDS_:
                want = LDS_ if fits else -2
            elif p == AUTO:
                want = LDS_ if fits else DEVICE if dfits else -2
            else:
                want = DEVICE if dfits else -2
            assert f["where"] == want, (p, m, n)
            if valid and p != 5:
                assert (want == -2) == _lib.placed_too_large(p, m, n), (p, m, n)
                if want >= 0:
                    assert (want == DEVICE) == _lib.placed_on_device(p, m, n), (p, m, n)


def test_device_chunk(check):
    work = 32 << 20             # LPK_BATCH_DEV_WORK of csrc/batch.hip
    cases = [(4096, work, 100, 200), (4096, work, 256, 512), (4096, work, 1100, 1160), (1, work, 100, 200),
             (5, work, 8, 18), (4096, 1000, 100, 200), (4096, work, 10231, 10231)]
    got = check(["chunk chunk=%d work=%d m=%d n=%d" % c for c in cases])
    for (chunk, w, m, n), ln in zip(cases, got):
        assert int(fields(ln)["pivots"]) == max(1, min(chunk, w // ((m + 1) * (n + 1))))
    assert [int(fields(ln)["pivots"]) for ln in got] == [1652, 254, 26, 1, 5, 1, 1]


def random_shapes(rng):
    out = []
    for _ in range(rng.randint(1, 40)):
        pick = rng.random()
        if pick < 0.4:
            out.append((rng.randint(1, 12), rng.randint(1, 24)))
        elif pick < 0.7:
            out.append((rng.randint(1, 70), rng.randint(1, 140)))
        elif pick < 0.95:
            out.append((rng.randint(1, 400), rng.randint(1, 600)))
        else:
            out.append((rng.randint(1, 12000), rng.randint(1, 8000)))
    return out


def test_random_lists_auto_and_device(check):
    rng = random.Random(4100)
    requests = []
    for k in range(2000):
        place = AUTO if k % 4 else DEVICE
        shapes = [s for s in random_shapes(rng) if _lib.batch_device_lds_bytes(*s) <= LDS]
        if not shapes:
            shapes = [(8, 18)]
        caps = (32, 8, 16, 2) if k % 3 else (rng.randint(1, 40), rng.randint(1, 10), rng.choice((4, 8, 16)),
                                             rng.randint(1, 8))
        requests.append((place, shapes, caps))
    lines = []
    for place, shapes, (c1, c4, dw, dc) in requests:
        lines.append(plan_line(place, shapes, c1, c4, dw, dc))
        lds_only = [s for s in shapes if place == AUTO and _lib.batch_lds_bytes(*s) <= LDS]
        lines.append(ragged_line(lds_only or [(1, 1)], c1, c4))
    got = check(lines)
    some_dev = some_both = 0
    for k, (place, shapes, (c1, c4, dw, dc)) in enumerate(requests):
        too_large, bins = parse_plan(got[2 * k])
        assert too_large == -1
        want_dev = [i for i, s in enumerate(shapes) if place == DEVICE or _lib.batch_lds_bytes(*s) > LDS]
        seen = sorted(i for b in bins for i in b["order"])
        assert seen == list(range(len(shapes)))                     # every LP in exactly one bin
        for b in bins:
            assert b["order"] == sorted(b["order"])                 # ascending inside a bin
        dev = [b for b in bins if b["device"]]
        assert len(dev) == (1 if want_dev else 0)
        if dev:
            assert bins[0] is dev[0]                                # the device bin comes first
            assert dev[0]["order"] == want_dev                      # exactly the LPs above a CU's LDS (or all)
            assert dev[0]["waves"] == dw
            assert dev[0]["lds"] == max(_lib.batch_device_lds_bytes(*shapes[i]) for i in want_dev)
            assert dev[0]["per_cu"] == min(dc, LDS // dev[0]["lds"]) >= 1
            some_dev += 1
        # the LDS-placed LPs: plan_ragged's bins of a batch of their own, indices mapped back
        lds_at = [i for i in range(len(shapes)) if i not in set(want_dev)]
        rest = [b for b in bins if not b["device"]]
        if lds_at:
            _, alone = parse_plan(got[2 * k + 1])
            assert [dict(b, order=[lds_at[i] for i in b["order"]]) for b in alone] == rest
            some_both += bool(dev)
        else:
            assert rest == []
    assert some_dev > 200 and some_both > 200


def test_all_lds_input_gives_plan_ragged_unchanged(check):
    rng = random.Random(7)
    lists = []
    while len(lists) < 300:
        shapes = [s for s in random_shapes(rng) if _lib.batch_lds_bytes(*s) <= LDS]
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
    mixed = [(8, 18), (40, 80), (100, 200), (2, 2), (120, 210)]
    got = [parse_plan(ln) for ln in check([plan_line(AUTO, mixed), plan_line(DEVICE, mixed), plan_line(LDS_, mixed),
                                           plan_line(AUTO, [(8, 18), (10232, 10231)]),
                                           plan_line(AUTO, [(100, 200)] * 5, dwaves=8, dcap=4)])]
    too_large, bins = got[0]
    assert too_large == -1
    assert bins[0] == dict(device=1, waves=16, lds=(211 + 121 + 16) * 8, per_cu=2, order=[2, 4])
    assert sorted(i for b in bins[1:] for i in b["order"]) == [0, 1, 3]
    assert [b["lds"] for b in bins[1:]] == sorted((b["lds"] for b in bins[1:]), reverse=True)
    assert got[1] == (-1, [dict(device=1, waves=16, lds=(211 + 121 + 16) * 8, per_cu=2, order=[0, 1, 2, 3, 4])])
    assert got[2] == (2, [])                                        # LDS only: the first LP that does not fit
    assert got[3] == (1, [])
    assert got[4] == (-1, [dict(device=1, waves=8, lds=(201 + 101 + 16) * 8, per_cu=4, order=[0, 1, 2, 3, 4])])
