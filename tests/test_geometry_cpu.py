"""Launch planning and the environment knobs on the CPU.

csrc/geometry.h decides every launch's kernel, grid and row/column split as
pure functions, csrc/knobs.h parses every LPGPU_* variable.  csrc/geometry_check.cpp
drives both from stdin; it is built here with -fsanitize=address,undefined and
run as a child process, so a sanitizer report fails the test that met it."""
import glob
import itertools
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "linear-program-solver_amd", "csrc")
GROUP_LDS_MAX = 96 * 1024
GROUP_MAXBLOCKS = 256
# the variants the library compiles (csrc/geometry.h GROUP_VARIANTS; select.hip sel_kernel)
GROUP_VARIANTS = {(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 3, 1), (2, 3, 1), (1, 4, 1), (2, 4, 1), (4, 4, 1),
                  (4, 2, 2), (4, 4, 2), (4, 2, 4), (4, 4, 4)}


@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "geometry_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(CSRC, "build", "geometry_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(requests):
        """requests: (name, {field: value}) -> one dict of numbers per request"""
        text = "".join(name + "".join(" %s=%s" % kv for kv in fields.items()) + "\n" for name, fields in requests)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(requests)
        return [{k: float(v) if "." in v or "e" in v else int(v) for k, v in (kv.split("=") for kv in ln.split())}
                for ln in lines]
    return run


def pitches(check, ns):
    return {n: p["ld"] for n, p in zip(ns, check([("pitch", {"n": n, "raw": 0}) for n in ns]))}


# ---- the sweep ---------------------------------------------------------------
SWEEP_ROWS = [2, 9, 63, 64, 65, 257, 4097, 16384, 16385, 32769, 40001]
SWEEP_NCOL = [2, 64, 65, 128, 129, 255, 256, 257, 8101, 8193]
SWEEP_DEPTH = [1, 16, 17, 32, 48, 49, 63, 64]
SWEEP_SPLITS = [0, 0.55, 0.62, 0.7]


def cdiv(a, b):
    """C's integer division (truncates towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def up(a, b):
    return (a + b - 1) // b * b


def expected_split(rows, nsg, cus, bpc, split):
    """k_sweep_rl's row runs, restated from DESIGN.md 4e: equal runs of whole
    8-row batches over the resident slots; with two workgroups per CU and an
    even number of runs the first half takes `split` of the rows -- unless
    those runs would not cover the tableau or one would start past its end.
    -> (nrun, run, runb, na)"""
    nrun = max(1, cus * bpc // nsg)
    run = up(-(-rows // nrun), 8)
    nrun = -(-rows // run)
    if 0.0 < split < 1.0 and bpc == 2 and nrun >= 2 and nrun % 2 == 0:
        h = nrun // 2
        ra = up(int(split * float(rows)) // h, 8)
        rb = cdiv(cdiv(rows - h * ra + h - 1, h) + 7, 8) * 8
        if ra > 0 and rb > 0 and h * (ra + rb) >= rows and h * ra + (h - 1) * rb < rows:
            return nrun, ra, rb, h
    return nrun, run, run, nrun


def runs_cover(rows, nrun, run, runb, na):
    """the kernel's own arithmetic (k_sweep_rl: r0, r1 of run ri): every run
    starts inside the tableau, and they tile [0, rows) in order"""
    at = 0
    for ri in range(nrun):
        r0 = ri * run if ri < na else na * run + (ri - na) * runb
        r1 = min(rows, r0 + (run if ri < na else runb))
        if r0 != at or r0 >= rows or r1 <= r0:
            return False
        at = r1
    return at == rows


def test_sweep_plans(check):
    ld_of = pitches(check, [c - 1 for c in SWEEP_NCOL])
    cases = [dict(rows=rows, n=ncol - 1, ld=ld_of[ncol - 1], nd_max=nd, cnt=-1, share=share,
                  second=int(rows * ld_of[ncol - 1] * 8 > 512 << 20), cus=cus, bpc=bpc, tail=tail, split=split)
             for rows, ncol, nd, cus, bpc, tail, split, share in itertools.product(
                 SWEEP_ROWS, SWEEP_NCOL, SWEEP_DEPTH, [8, 256], [1, 2, 3], [0, 1, 2], SWEEP_SPLITS, [1, 2])]
    plans = check([("sweep", c) for c in cases])
    covered = {}
    seen = {"rl": 0, "dp2": 0, "w8": 0, "split": 0, "spread": 0, "tailed": 0, "zero": 0, "oop": 0}
    for c, p in zip(cases, plans):
        rows, n, ld = c["rows"], c["n"], c["ld"]
        nb = 16 if c["nd_max"] <= 16 else 32 if c["nd_max"] <= 32 else 48 if c["nd_max"] <= 48 else 64
        assert p["nb"] == nb
        assert p["rl"] == int(nb == 64 and ld % 64 == 0 and ld >= 128), (c, p)
        batch = 8 if p["rl"] else 4
        assert p["run"] % batch == 0 and p["runb"] % batch == 0 and p["tail"] % batch == 0, (c, p)
        assert p["run"] > 0 and p["runb"] > 0 and 0 < p["na"] <= p["nrun"]
        assert p["grid"] == p["nrun"] * p["nsg"] and p["grid"] < 1 << 31, (c, p)
        key = (rows, p["nrun"], p["run"], p["runb"], p["na"])
        if key not in covered:
            covered[key] = runs_cover(*key)
        assert covered[key], (c, p)
        if p["tail"] > 0:
            assert p["tail"] * p["grid"] >= rows, (c, p)
            assert c["tail"] != 0
        if p["rl"]:
            w8 = c["share"] > 1 and rows >= 16384
            assert (p["W"], p["D"]) == ((8, 4) if w8 else (4, 2)), (c, p)
            assert p["oop"] == c["second"]
            assert p["nexp"] == c["nd_max"] and p["zero"] == int(c["nd_max"] < 64)
            strip = 64 * p["W"]
            assert p["tend"] == n + 1
            if p["tail"] > 0:   # spread: whole strips, then at most 64 columns from tcol
                assert p["tcol"] == p["nsg"] * strip and p["tcol"] < p["tend"] <= p["tcol"] + 64, (c, p)
            else:
                assert p["nsg"] * strip >= n + 1 > (p["nsg"] - 1) * strip, (c, p)
            nfull, rest = (n + 1) // strip, (n + 1) % strip
            assert (p["tail"] > 0) == (c["tail"] != 0 and nfull >= 1 and 0 < rest <= 64), (c, p)
            want = expected_split(rows, p["nsg"], c["cus"], c["bpc"], c["split"])
            assert (p["nrun"], p["run"], p["runb"], p["na"]) == want, (c, p, want)
            seen["split"] += p["na"] != p["nrun"]
            seen["w8"] += w8
            seen["spread"] += p["tail"] > 0
            seen["zero"] += p["zero"]
            seen["oop"] += p["oop"]
        else:
            assert (p["W"], p["oop"], p["zero"]) == (10, 0, 0) and p["na"] == p["nrun"] and p["runb"] == p["run"]
            ns = (ld + 127) // 128
            assert p["nsg"] == (ns - 1 if p["tail"] > 0 else ns) and p["nsg"] >= 1, (c, p)
            seen["tailed"] += p["tail"] > 0
        seen["rl" if p["rl"] else "dp2"] += 1
    assert all(v > 0 for v in seen.values()), seen   # every path was planned somewhere


@pytest.mark.parametrize("rows,second,want", [
    (4097, 0, dict(grid=512, nsg=32, nrun=16, run=320, runb=200, na=8, tail=16, tcol=8192)),      # cfg3, in place
    (32769, 1, dict(grid=512, nsg=32, nrun=16, run=2544, runb=1560, na=8, tail=72, tcol=8192)),   # cfg4, out of place
], ids=["cfg3", "cfg4"])
def test_sweep_plan_of_the_bench_shapes(check, rows, second, want):
    """the bench's two sweeps on a 256-CU device, two workgroups per CU: the
    split (na, run, runb) engages -- what no GPU test can see"""
    ld = pitches(check, [8192])[8192]
    assert ld == 8320
    p, = check([("sweep", dict(rows=rows, n=8192, ld=ld, nd_max=64, cnt=-1, share=1, second=second, cus=256, bpc=2,
                               tail=1, split=0.62))])
    assert (p["rl"], p["W"], p["D"], p["oop"], p["nb"], p["nexp"], p["zero"]) == (1, 4, 2, second, 64, 64, 0)
    assert {k: p[k] for k in want} == want
    assert p["tend"] == 8193


# ---- the persistent selections -----------------------------------------------
SEL_RC = [1, 63, 64, 65, 4096, 4097, 8192, 32768, 40000, 65537]
SEL_N = [1, 255, 256, 257, 4096, 8192, 16385]
MODELS = [("const", 1), ("const", 2), ("const", 8), ("lds", 8), ("missing", 0)]


def model_occupancy(occ, k, lds):
    return k if occ == "const" else min(k, 160 * 1024 // up(lds, 2048))


def check_geom(c, p, xcd_cus, xr, nshard, ld):
    """the invariants of one planned persistent launch (g > 0); xr None:
    plan_sel asked directly"""
    rc, n, bmax, share = c["rc"], c["n"], c["bmax"], c["share"]
    g, per_cu = p["g"], p["per_cu"]
    assert c["occ"] != "missing", (c, p)
    assert p["xs"] in (0, 8) and (p["xs"] == 0 or bmax > 32), (c, p)
    assert rc <= 64 * g * p["rpl"] * max(p["xs"], 1), (c, p)
    assert per_cu >= 1 and per_cu == model_occupancy(c["occ"], c["k"], p["lds"]), (c, p)
    if p["sel"]:
        assert xr is None or (xr != 1 and nshard == 1 and (share == 1 or xr == 2)), (c, p)
        assert p["sel"] == (32 if bmax <= 32 else 64) and (p["xs"] == 0 or p["sel"] == 64)
        assert p["ipl"] in (1, 2, 4) and (p["nr"], p["rpl"], p["xmode"], p["hk"]) == (1, 1, 1, 0), (c, p)
        assert g <= 64 and n <= 64 * p["ipl"] * g, (c, p)
        assert p["lds"] == (-(-n // g) * (p["sel"] + 2) + 8) * 8, (c, p)
        assert p["xs"] == (8 if rc > 64 * 64 else 0) and (p["xs"] == 0 or c["xs_ok"]), (c, p)
        need = share * g if p["xs"] else g + 1 if share > 1 else g
        assert need <= per_cu * xcd_cus, (c, p)
        return
    assert (p["nr"], p["ipl"], p["rpl"]) in GROUP_VARIANTS and p["xs"] == 0, (c, p)
    assert g <= 64 * p["nr"] and g <= GROUP_MAXBLOCKS and ld <= 64 * p["ipl"] * g, (c, p)
    rpb, cpb = -(-rc // g), -(-ld // g)
    assert p["lds"] == ((rpb + cpb) * (bmax + 1) + cpb + rpb + 8) * 8 and p["lds"] <= GROUP_LDS_MAX, (c, p)
    if p["xmode"]:
        assert xr != 1 and nshard == 1 and share == 1 and not p["hk"] and g <= per_cu * xcd_cus, (c, p)
    else:
        per_cu_job = per_cu - 1 if share > 1 else per_cu
        assert (g * nshard * share + 7) // 8 <= per_cu_job * xcd_cus, (c, p)
        assert not p["hk"] or (g % 8 == 0 and g >= 64 and xr == 0 and nshard == 1 and c.get("hier", 1)), (c, p)


def test_group_plans(check):
    ld_of = pitches(check, SEL_N)
    cases = [dict(rc=rc, ld=ld_of[n], n=n, bmax=bmax, xr=xr, nshard=nshard, share=share, xs_ok=xs_ok, cus=cus, hier=1,
                  occ=occ, k=k)
             for rc, n, bmax, xr, nshard, share, xs_ok, (occ, k), cus in itertools.product(
                 SEL_RC, SEL_N, [16, 32, 48, 64], [0, 1, 2], [1, 3, 8], [1, 2, 4], [0, 1], MODELS, [256, 64])]
    plans = check([("group", c) for c in cases])
    seen = {"sel": 0, "xs": 0, "one": 0, "spread": 0, "hk": 0, "none": 0}
    for c, p in zip(cases, plans):
        if p["g"] == 0:
            seen["none"] += 1
            continue
        check_geom(c, p, c["cus"] // 8, c["xr"], c["nshard"], c["ld"])
        seen["sel"] += p["sel"] > 0
        seen["xs"] += p["xs"] > 0
        seen["one"] += p["sel"] == 0 and p["xmode"] == 1
        seen["spread"] += p["xmode"] == 0
        seen["hk"] += p["hk"]
    assert all(v > 0 for v in seen.values()), seen
    # the flat exchange (LPGPU_HIER=0) never takes the two-level variant
    flat = [dict(c, hier=0) for c in cases[::7]]
    assert not any(p["hk"] for p in check([("group", c) for c in flat]))


def test_sel_plans(check):
    cases = [dict(rc=rc, n=n, bmax=bmax, xcd_cus=xcd_cus, xr=xr, xs_ok=xs_ok, share=share, occ=occ, k=k)
             for rc, n, bmax, xr, share, xs_ok, (occ, k), xcd_cus in itertools.product(
                 SEL_RC, SEL_N, [16, 32, 48, 64], [0, 1], [1, 2, 4], [0, 1], MODELS, [32, 8])]
    plans = check([("sel", c) for c in cases])
    fit = 0
    for c, p in zip(cases, plans):
        if p["g"] == 0:
            continue
        assert p["sel"] > 0
        check_geom(c, p, c["xcd_cus"], None, 1, None)
        fit += 1
    assert fit > 0
    # the bench's selections, two blocks per CU resident: cfg3 on one XCD, cfg4 as XCD shards
    cfg3, cfg4 = check([("sel", dict(rc=rc, n=8192, bmax=64, xcd_cus=32, xr=0, xs_ok=1, share=1, occ="lds", k=8))
                        for rc in (4096, 32768)])
    assert (cfg3["g"], cfg3["ipl"], cfg3["xs"], cfg3["sel"]) == (64, 2, 0, 64)
    assert (cfg4["g"], cfg4["ipl"], cfg4["xs"], cfg4["sel"]) == (64, 2, 8, 64)


# ---- the knobs -------------------------------------------------------------------
DEFAULTS = dict(sweep_oop=2, oop_room_mb=1024, oop_fail_alloc=0, sweep_cus=0, sweep_tail=1, sweep_split=0.62, coop=0,
                hier=1, gmaj=1, ld_raw=0, persistent=1, spin_max=1 << 22, xwait_ms=30000, fault_launch=0, fault_t=0,
                fault_xcc=0, strict=0, xs_ok=1, peer_enable=1, stamps=0, xr_xcd=-1)
# knob -> (an accepted value, a junk value) and the fields each gives: atoi /
# strtoul / atof read junk as 0, the flags compare the first character only
KNOBS = {
    "LPGPU_SWEEP_OOP": (("1", dict(sweep_oop=1)), ("junk", dict(sweep_oop=0))),
    "LPGPU_OOP_ROOM_MB": (("100000000", dict(oop_room_mb=100000000)), ("junk", dict(oop_room_mb=0))),
    "LPGPU_OOP_FAIL_ALLOC": (("1", dict(oop_fail_alloc=1)), ("yes", {})),
    "LPGPU_SWEEP_CUS": (("8", dict(sweep_cus=8)), ("junk", {})),
    "LPGPU_SWEEP_TAIL": (("2", dict(sweep_tail=2)), ("junk", dict(sweep_tail=0))),
    "LPGPU_SWEEP_SPLIT": (("0.55", dict(sweep_split=0.55)), ("junk", dict(sweep_split=0))),
    "LPGPU_COOP": (("1", dict(coop=1)), ("on", {})),
    "LPGPU_HIER": (("0", dict(hier=0)), ("junk", dict(hier=0))),
    "LPGPU_GMAJ": (("0", dict(gmaj=0)), ("junk", dict(gmaj=0))),
    "LPGPU_LD_RAW": (("1", dict(ld_raw=1)), ("true", {})),
    "LPGPU_SELECT": (("kernels", dict(persistent=0)), ("Kernels", {})),
    "LPGPU_SPIN_MAX": (("20000", dict(spin_max=20000)), ("junk", dict(spin_max=0))),
    "LPGPU_XWAIT_MS": (("3000", dict(xwait_ms=3000)), ("junk", dict(xwait_ms=0))),
    "LPGPU_FAULT": (("3:4", dict(fault_launch=3, fault_t=4)), ("5", dict(fault_launch=5))),
    "LPGPU_FAULT_XCC": (("2", dict(fault_xcc=2)), ("junk", {})),
    "LPGPU_STRICT": (("1", dict(strict=1)), ("true", {})),
    "LPGPU_SEL_XS": (("0", dict(xs_ok=0)), ("no", {})),
    "LPGPU_PEER": (("0", dict(peer_enable=0)), ("no", {})),
    "LPGPU_STAMPS": (("1", dict(stamps=1)), ("2", {})),
    "LPGPU_XR_XCD": (("1", dict(xr_xcd=1)), ("junk", dict(xr_xcd=2))),
}


def test_knob_values(check):
    requests = [("knobs", {})] + [("knobs", {name: value}) for name, pair in KNOBS.items() for value, _ in pair]
    got = check(requests)
    assert got[0] == DEFAULTS
    want = [dict(DEFAULTS, **fields) for pair in KNOBS.values() for _, fields in pair]
    assert got[1:] == want
    assert check([("knobs", {"LPGPU_XR_XCD": "0", "LPGPU_FAULT": "junk"})]) == [dict(DEFAULTS, xr_xcd=0)]


def test_knob_table_is_complete():
    """every LPGPU_* name in csrc is in knobs.h's table (the only getenv) and
    in INTEGRATION.md.  LPGPU_BATCH_ONE_WAVE_ELEMS is a compile-time define
    (batch.hip, scripts/batch_waves.py), not an environment variable."""
    names, getenv_files = set(), set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        if path.endswith((".h", ".hip", ".cpp")):
            text = open(path).read()
            names |= set(re.findall(r"LPGPU_[A-Z0-9_]+", text))
            if "getenv" in text:
                getenv_files.add(os.path.basename(path))
    names.discard("LPGPU_BATCH_ONE_WAVE_ELEMS")
    table = set(re.findall(r'get\("(LPGPU_[A-Z0-9_]+)"\)', open(os.path.join(CSRC, "knobs.h")).read()))
    assert names == table == set(KNOBS)
    assert getenv_files == {"knobs.h"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(table) if "`" + n not in doc] == []
