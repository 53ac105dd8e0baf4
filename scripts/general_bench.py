#!/usr/bin/env python3
"""General-form upload against what the library offered before it: the
standard form built, shifted and undone on the device (lp_general_upload,
lp_general_solution; k_general_shift, k_general_assemble, k_general_recover)
against standard-form tableaux the host builds with general_standard_form,
ships whole through upload() and undoes with general_recover.

Five seeded workloads: all-BOXED mixed 8x10 x 16384 and 24x24 x 4096, kinds
cycling 0..4 at mixed 40x40 x 1024 (place="lds"), all-BOXED mixed 64x64 x 512
under place="auto" (its standard form is 129 x 193 doubles: device-placed),
and phase1_lp("ge", 24, 24) x 2048 with every variable LOWER for the two-phase
path.  For each, in one process, 5 timed repetitions after a warm-up (host
clock, every call synchronous), the legs alternating and taking turns at going
first:

  (a)  on one reused engine: upload_general + derive_basis where the plain
       path applies + solve + general_solution
  (b)  on the same engine: upload of standard-form tableaux the host built
       beforehand + the same solve + solution() + general_recover on the host
  (b') (b) with general_standard_form on the host inside the timed region
  the upload step of (a) and of (b) alone, and general_duals() against
  download() + the host's general_duals

Before anything is timed (a) is checked against (b): equal status and pivot
counts, and the bits of x and the objective.  The condition: at every workload
the slowest of (a)'s five is not above the fastest of (b)'s five.

Prints one JSON line (profiles/r16/general_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/general_bench.py
With --trace it only runs each workload's (a) leg three times, for a kernel
trace of the new kernels taken in a run of its own.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "linear-program-solver_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from lpsol_amd import _lib                      # noqa: E402
from lpsol_amd import generators as gen         # noqa: E402
from lpsol_amd import problem as pr             # noqa: E402

PLAIN, LOWER, BOXED, UPPER, FREE = range(5)
# name, generator kind, m, ns, LPs, place, kinds of the variables
WORKLOADS = [("boxed", "mixed", 8, 10, 16384, "lds", lambda ns: [BOXED] * ns),
             ("boxed", "mixed", 24, 24, 4096, "lds", lambda ns: [BOXED] * ns),
             ("cycling", "mixed", 40, 40, 1024, "lds", lambda ns: [j % 5 for j in range(ns)]),
             ("boxed", "mixed", 64, 64, 512, "auto", lambda ns: [BOXED] * ns),
             ("lower", "ge", 24, 24, 2048, "lds", lambda ns: [LOWER] * ns)]
CAP = 1 << 16
REPS = 5


def med(xs):
    return statistics.median(xs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def inputs(gkind, m, ns, B, kinds):
    """-> (problem blocks, senses, kind, lb, ub): dyadic bounds, a zero shift
    where the plain path is wanted (b stays >= 0)"""
    if gkind == "mixed":
        T, sense = gen.mixed_stack(m, ns, range(1, B + 1)), np.zeros(m, dtype=np.int8)
    else:
        T = np.stack([gen.phase1_lp("ge", m, ns, s) for s in range(1, B + 1)])
        sense = np.array([_lib.SENSE_GE] * m + [_lib.SENSE_LE], dtype=np.int8)
    kind = np.array(kinds(ns), dtype=np.int8)
    j = np.arange(ns)
    lb = np.where(np.isin(kind, (LOWER, BOXED)), 0.0 if gkind == "mixed" else 0.125,
                  np.where(kind == PLAIN, 0.0, -np.inf))
    ub = np.where(np.isin(kind, (BOXED, UPPER)), 1.5 + (j % 4) / 4.0, np.inf)
    return np.ascontiguousarray(T[:, :, :ns + 1]), sense, kind, lb, ub


def bench(name, gkind, m, ns, B, place, kinds, trace=False):
    P, sense, kind, lb, ub = inputs(gkind, m, ns, B, kinds)
    G = pr.pack_general(P, lb, ub)
    Th = pr.general_standard_form(P, lb, ub, sense, kind, False)
    rows, n = Th.shape[1] - 1, Th.shape[2] - 1
    all_le = bool((sense == _lib.SENSE_LE).all())
    placed = place != "lds"
    eng = _lib.BatchEngine(B, rows, n, place=place)
    eng.set_form(sense, kind, False)

    def leg_a():
        eng.upload_general(G)
        out = pr._run(eng, all_le, placed, CAP)
        return out, eng.general_solution()

    def rest_b():
        out = pr._run(eng, all_le, placed, CAP)
        xs, z = eng.solution()
        return out, pr.general_recover(xs, -z, lb, ub, kind, False)

    def leg_b():
        eng.upload(Th)
        return rest_b()

    def leg_b2():
        eng.upload(pr.general_standard_form(P, lb, ub, sense, kind, False))
        return rest_b()

    if trace:
        for _ in range(3):
            leg_a()
        eng.close()
        return {"shape": f"{name} {m}x{ns}", "lps": B}

    # the check, before anything is timed
    (sa, xa), (sb, xb) = leg_a(), leg_b()
    assert sa[0] == sb[0], "another path"
    assert all(same_bits(p, q) for p, q in zip(sa[1:], sb[1:])), "status or pivot counts differ"
    assert same_bits(xa[0], xb[0]) and same_bits(xa[1], xb[1]), "x or objective bits differ"
    optimal = int(np.count_nonzero(sa[1] == _lib.OPTIMAL))

    def host_duals():
        out = eng.download()
        got = [pr.general_duals(t, sense, kind, False) for t in out]
        return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])

    keys = ("a", "b", "b2", "up_a", "up_b", "duals", "host_duals")
    t = {k: [] for k in keys}
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        legs = [("a", leg_a), ("b", leg_b), ("b2", leg_b2)]
        legs = legs[rep % 3:] + legs[:rep % 3]  # they take turns at going first
        got = {k: clock(fn)[0] for k, fn in legs}
        ups = [("up_a", lambda: eng.upload_general(G)), ("up_b", lambda: eng.upload(Th))]
        for k, fn in (ups if rep % 2 else ups[::-1]):
            got[k] = clock(fn)[0]
        pr._run(eng, all_le, placed, CAP)
        dd = [("duals", eng.general_duals), ("host_duals", host_duals)]
        for k, fn in (dd if rep % 2 else dd[::-1]):
            got[k] = clock(fn)[0]
        if rep:
            for k in keys:
                t[k].append(got[k])
    assert all(same_bits(p, q) for p, q in zip(eng.general_duals(), host_duals()))
    eng.close()
    return {
        "shape": f"{name} {m}x{ns}", "m": m, "ns": ns, "rows": rows, "n": n, "lps": B, "place": place,
        "path": sa[0], "optimal_lps": optimal,
        "general_s": med(t["a"]), "general_s_runs": t["a"],
        "tableau_s": med(t["b"]), "tableau_s_runs": t["b"],
        "tableau_with_host_build_s": med(t["b2"]), "tableau_with_host_build_s_runs": t["b2"],
        "tableau_over_general": med(t["b"]) / med(t["a"]),
        "slowest_general_over_fastest_tableau": max(t["a"]) / min(t["b"]),
        "condition_met": max(t["a"]) <= min(t["b"]),
        "upload_general_s": med(t["up_a"]), "upload_general_s_runs": t["up_a"],
        "upload_tableaux_s": med(t["up_b"]), "upload_tableaux_s_runs": t["up_b"],
        "general_duals_s": med(t["duals"]), "general_duals_s_runs": t["duals"],
        "download_and_host_duals_s": med(t["host_duals"]), "download_and_host_duals_s_runs": t["host_duals"],
        "bytes_in_general": int(G.nbytes), "bytes_in_tableaux": int(Th.nbytes),
        "bytes_ratio": G.nbytes / Th.nbytes,
        "bit_identical_to_tableau_path": True,
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("general_bench.py needs a GPU")
    trace = "--trace" in sys.argv[1:]
    out = [bench(*w, trace=trace) for w in WORKLOADS]
    if trace:
        print(json.dumps({"bench": "general_bench", "trace_only": True, "workloads": out}))
        return 0
    ok = all(r["condition_met"] for r in out)
    print(json.dumps({"bench": "general_bench", "reps": REPS, "workloads": out,
                      "general_leg_never_slower_than_tableau_leg": ok}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
