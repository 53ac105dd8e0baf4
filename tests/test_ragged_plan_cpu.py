"""Launch planning of ragged batches on the CPU.

csrc/batch_plan.h sorts the LPs of a ragged batch into launch bins as a pure
function of their shapes and of the workgroups a CU holds of each kernel
instantiation.  csrc/batch_plan_check.cpp drives it from stdin; it is built
here with -fsanitize=address,undefined and run as a child process, so a
sanitizer report fails the test that met it."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, fixture_input, load_golden

import _ragged_cases as rc

from lpsol_amd import _lib

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
LDS = 160 * 1024
ELEMS = 2048
KINDS = ("plain", "twophase")
# workgroups per CU by wave slots and registers: k_batch, k_twophase
CAPS = {"plain": (32, 8), "twophase": (16, 4)}

# the 17 LPs of test_gpu_ragged.py's two-phase list, as (m, n)
TWOPHASE_17 = [rc.shape_of(T) for T in rc.twophase_list()]


@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_plan_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "batch_plan_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def plans(check, requests):
    """requests: (kind, cap1, cap4, shapes) -> per request (too_large, bins);
    a bin is dict(waves, lds, per_cu, order)"""
    lines = ["plan kind=%s cap1=%d cap4=%d elems=%d shapes=%s"
             % (kind, c1, c4, ELEMS, ",".join("%d:%d" % s for s in shapes)) for kind, c1, c4, shapes in requests]
    out = []
    for ln in check(lines):
        f = dict(kv.split("=") for kv in ln.split())
        bins = []
        for b in filter(None, f["bins"].split(";")):
            w, lds, per, order = b.split(":")
            bins.append(dict(waves=int(w), lds=int(lds), per_cu=int(per), order=[int(x) for x in order.split(".")]))
        out.append((int(f["too_large"]), bins))
    return out


def need(kind, m, n):
    return _lib.batch_lds_bytes(m, n) if kind == "plain" else _lib.twophase_lds_bytes(m, n)


def waves(kind, m, n):
    return (1 if (m + 1) * (n + 1) <= ELEMS else 4) if kind == "plain" else _lib.twophase_waves(m, n)


def random_shapes(rng, kind):
    """a list of shapes that fit the call kind, tiny ones and ones near the LDS limit among them"""
    out = []
    while len(out) < rng.randint(1, 40):
        pick = rng.random()
        if pick < 0.5:
            m, n = rng.randint(1, 12), rng.randint(1, 24)
        elif pick < 0.9:
            m, n = rng.randint(1, 70), rng.randint(1, 140)
        else:
            m, n = rng.randint(1, 400), rng.randint(1, 400)
        if need(kind, m, n) <= LDS:
            out.append((m, n))
    return out


def check_plan(kind, caps, shapes, too_large, bins):
    assert too_large == -1
    cap = {1: caps[0], 4: caps[1]}
    seen = sorted(i for b in bins for i in b["order"])
    assert seen == list(range(len(shapes)))                         # every LP in exactly one bin
    assert len(bins) <= caps[0] + caps[1]
    assert [b["lds"] for b in bins] == sorted((b["lds"] for b in bins), reverse=True)   # launch order
    for b in bins:
        assert b["order"] == sorted(b["order"])
        needs = [need(kind, *shapes[i]) for i in b["order"]]
        assert b["lds"] == max(needs)
        assert LDS // b["lds"] >= 1
        assert b["per_cu"] == min(cap[b["waves"]], LDS // b["lds"])
        for i, nd in zip(b["order"], needs):
            assert waves(kind, *shapes[i]) == b["waves"]
            # no fewer LPs per CU by LDS than a uniform batch of its own shape
            assert LDS // b["lds"] >= min(cap[b["waves"]], LDS // nd)


@pytest.mark.parametrize("kind", KINDS)
def test_random_shape_lists(check, kind):
    rng = random.Random(20240 + KINDS.index(kind))
    requests = []
    for k in range(3000):
        caps = CAPS[kind] if k % 3 else (rng.randint(1, 40), rng.randint(1, 10))
        requests.append((kind, caps[0], caps[1], random_shapes(rng, kind)))
    got = plans(check, requests)
    for (_, c1, c4, shapes), (too_large, bins) in zip(requests, got):
        check_plan(kind, (c1, c4), shapes, too_large, bins)
    assert max(len(b) for _, b in got) >= 6                         # the lists do spread over bins
    assert {b["waves"] for _, bins in got for b in bins} == {1, 4}


@pytest.mark.parametrize("kind", KINDS)
def test_uniform_list_is_one_bin(check, kind):
    shapes = [(8, 18), (40, 80), (1, 1), (64, 128) if kind == "plain" else (60, 60), (31, 63)]
    got = plans(check, [(kind, *CAPS[kind], [s] * 7) for s in shapes])
    for (m, n), (too_large, bins) in zip(shapes, got):
        assert too_large == -1 and len(bins) == 1
        assert bins[0]["order"] == list(range(7))
        assert bins[0]["lds"] == need(kind, m, n)
        assert bins[0]["waves"] == waves(kind, m, n)


def test_pinned_plans(check):
    golden = [fixture_input(fx).shape for fx in load_golden("small.json")["solve"]]
    golden = [(r - 1, c - 1) for r, c in golden]
    assert len(golden) == 39
    mmax = _lib.batch_max_m(128)
    assert mmax == 155
    got = plans(check, [("plain", 32, 8, golden),
                        ("plain", 32, 8, [(1, 1), (mmax, 128)]),
                        ("plain", 32, 8, [(31, 63), (31, 64)]),
                        ("twophase", 16, 4, TWOPHASE_17)])
    for (too_large, bins), (kind, shapes) in zip(got, [("plain", golden), ("plain", [(1, 1), (mmax, 128)]),
                                                      ("plain", [(31, 63), (31, 64)]),
                                                      ("twophase", TWOPHASE_17)]):
        check_plan(kind, CAPS[kind], shapes, too_large, bins)
    assert len(got[0][1]) == 6
    assert {b["waves"] for b in got[0][1]} == {1, 4}
    assert [(b["waves"], b["lds"], b["order"]) for b in got[1][1]] == [(4, 163400, [1]), (1, 216, [0])]
    assert [(b["waves"], b["order"]) for b in got[2][1]] == [(4, [1]), (1, [0])]
    assert len(got[3][1]) == 4
    # the last four of the first fifteen are four-wave, every other LP one-wave
    four = sorted(i for b in got[3][1] if b["waves"] == 4 for i in b["order"])
    assert four == list(rc.TWOPHASE_FOUR_WAVE)


def test_too_large_names_the_first_lp(check):
    mmax, tmax = _lib.batch_max_m(128), _lib.twophase_max_m(128)
    got = plans(check, [("plain", 32, 8, [(1, 1), (mmax, 128), (mmax + 1, 128), (300, 300)]),
                        ("twophase", 16, 4, [(tmax, 128), (1, 1), (tmax + 1, 128)]),
                        ("twophase", 16, 4, [(tmax, 128), (1, 1)]),
                        ("plain", 32, 8, [(1 << 20, 1)])])
    assert [g[0] for g in got] == [2, 2, -1, 0]
    assert got[0][1] == [] and got[1][1] == [] and got[3][1] == []


def test_needs_equal_the_python_mirrors(check):
    grid = [(m, n) for m in (1, 2, 7, 8, 31, 32, 64, 90, 155, 156) for n in (1, 2, 9, 63, 64, 65, 128, 129)]
    got = check(["need m=%d n=%d elems=%d" % (m, n, ELEMS) for m, n in grid])
    lib = _lib.load()
    for (m, n), ln in zip(grid, got):
        f = {k: int(v) for k, v in (kv.split("=") for kv in ln.split())}
        assert f["plain"] == _lib.batch_lds_bytes(m, n), (m, n)
        assert f["twophase"] == _lib.twophase_lds_bytes(m, n) == lib.lp_twophase_lds_bytes(m, n), (m, n)
        assert f["wplain"] == (1 if (m + 1) * (n + 1) <= ELEMS else 4), (m, n)
        assert f["wtwophase"] == _lib.twophase_waves(m, n), (m, n)
