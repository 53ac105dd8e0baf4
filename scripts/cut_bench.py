#!/usr/bin/env python3
"""Warm cuts against a cold solve of the same LPs: two rows appended to solved
LPs (lp_cut_extend: k_cut_copy, k_cut_rows, k_cut_basis, then the dual simplex
from the basis at hand) against uploading the LPs with m + 2 rows and solving
them from scratch, which is what the library offered before.

Four seeded workloads on `mixed` LPs, two cuts each with a_j = U{0..8}/8 on the
LP's own seed: `le` (both a.x <= floor(48 a.x*) / 64) at 8x10 x 16384 and
40x40 x 4096 in LDS and at 100x100 x 2048 under place="auto", and `lege` (the
second cut a.x >= ceil(64 a.x*) / 64 + 0.25) at 40x40 x 4096.  For each, in one
process on engines that are reused, 5 timed repetitions after a warm-up (host
clock, every call synchronous), the legs alternating and taking turns at going
first:

  (a)  warm: extend_into a kept destination from the source, which holds the
       optimal tableaux, + run(RULE_DUAL, cap) + solution()
  (b)  cold: upload_problems of the LPs with m + 2 rows + derive_basis + solve
       (`le`) or the two-phase solve (`lege`) + solution()
  the extend_into call of (a) alone: two copies, three launches, one synchronise

Before anything is timed, (a) is compared bit for bit with the host statement
(lpsol_amd.problem.extend_tableau, then the host dual walk of the tests) on the
first 16 LPs, and with (b) over the whole batch: equal verdicts, the optima
within 1e-12 relative.  Reported per workload: the medians, every run, the
pivots per LP of both legs and "slowest a / fastest b".  No figure here is a
condition of anything: the README states what was measured.

Prints one JSON line (profiles/r20/cut_bench.json).  Run it once, under a time
limit:  timeout 900 python scripts/cut_bench.py
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
for p in (os.path.join(ROOT, "linear-program-solver_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lpsol_amd import _lib, solution_x          # noqa: E402
from lpsol_amd import generators as gen         # noqa: E402
from lpsol_amd import problem as pr             # noqa: E402

# name, m, ns, LPs, place
WORKLOADS = [("le", 8, 10, 16384, "lds"), ("le", 40, 40, 4096, "lds"), ("le", 100, 100, 2048, "auto"),
             ("lege", 40, 40, 4096, "lds")]
S_CUT = 31
CAP = 1 << 16
REPS = 5
REL = 1e-12
CHECKED = 16
LE, GE = _lib.SENSE_LE, _lib.SENSE_GE


def med(xs):
    return statistics.median(xs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def legs(name, m, ns, B, place):
    T = gen.mixed_stack(m, ns, range(1, B + 1))
    P = np.ascontiguousarray(T[:, :, :ns + 1])
    n = ns + m
    src = _lib.BatchEngine(B, m, n, place=place)
    src.set_senses(np.zeros(m, dtype=np.int8))
    src.upload_problems(P)
    src.derive_basis()
    st, _, _ = src.solve(CAP)
    assert (st == _lib.OPTIMAL).all()
    x = src.solution()[0][:, :ns]
    j = np.arange(ns, dtype=np.uint64)
    a = np.stack([np.stack([gen.uint_range(2000 + 1 + i, S_CUT + k, j, 0, 8) / 8.0 for k in range(2)])
                  for i in range(B)])
    ax = (a * x[:, None, :]).sum(axis=2)
    beta = np.floor(48 * ax) / 64
    sense = np.array([LE, LE], dtype=np.int8)
    if name == "lege":
        beta[:, 1] = np.ceil(64 * ax[:, 1]) / 64 + 0.25
        sense[1] = GE
    rows = np.zeros((B, 2, n + 1))
    rows[:, :, 0] = beta
    rows[:, :, 1:ns + 1] = a
    dst = _lib.BatchEngine(B, m + 2, n + 2, place=place, log_cap=64 if B else 0)
    cap = 10 * (m + 2 + n + 2)
    P2 = np.zeros((B, m + 3, ns + 1))
    P2[:, :m + 1] = P
    P2[:, m + 1:, 0] = beta
    P2[:, m + 1:, 1:] = a
    cold_eng = _lib.BatchEngine(B, m + 2, n + 2, place=place)
    cold_eng.set_senses(np.concatenate([np.zeros(m, dtype=np.int8), sense]))
    placed = place != "lds"

    def leg_a():
        src.extend_into(dst, rows, sense)
        st, done = dst.run(_lib.RULE_DUAL, cap)
        return (st, done), dst.solution()

    def leg_b():
        cold_eng.upload_problems(P2)
        if name == "le":
            cold_eng.derive_basis()
            st, npiv, _ = cold_eng.solve(CAP)
        else:
            out = (cold_eng.solve_lp_placed if placed else cold_eng.solve_lp)(CAP)
            st, npiv = out[0], out[3] + out[4]
        return (st, npiv), cold_eng.solution()

    return src, dst, cold_eng, rows, sense, cap, leg_a, leg_b, lambda: src.extend_into(dst, rows, sense)


def host_check(src, dst, rows, sense, cap, ra, xa, za):
    """(a) on the first LPs against the host statement and the host dual walk, bit for bit"""
    import _dual_cases as dc
    k = min(CHECKED, src.count)
    tabs, bases = src.download(0, k), src.get_basis()
    for i in range(k):
        D, basis = pr.extend_tableau(tabs[i], bases[i], rows[i], sense)
        w = dc.walk(D, cap)
        for r, c in w["log"]:
            basis[r] = c
        assert (ra[0][i], ra[1][i]) == (w["status"], w["npiv"]), ("walk", i)
        assert dst.log(i).tolist() == w["log"][:64], ("log", i)
        assert xa[i].tobytes() == solution_x(w["T"], basis).tobytes() and za[i] == -w["T"][0, 0], ("x", i)
        assert dst.download(i, 1)[0].tobytes() == np.ascontiguousarray(w["T"]).tobytes(), ("T", i)


def bench(name, m, ns, B, place, trace=False):
    src, dst, cold_eng, rows, sense, cap, leg_a, leg_b, step = legs(name, m, ns, B, place)
    if trace:
        for _ in range(3):
            leg_a()
        return {"shape": f"{name} {m}x{ns}", "lps": B}
    # the checks, before anything is timed
    (ra, (xa, za)), (rb, (_, zb)) = leg_a(), leg_b()
    host_check(src, dst, rows, sense, cap, ra, xa, za)
    assert np.array_equal(ra[0], rb[0]), "verdicts differ"
    ok = ra[0] == _lib.OPTIMAL
    err = np.abs(za[ok] - zb[ok]) / np.maximum(1.0, np.abs(zb[ok]))
    assert (err <= REL).all(), "optima differ"
    t = {k: [] for k in ("a", "b", "step")}
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        both = [("a", leg_a), ("b", leg_b)]
        got = {}
        for k, fn in (both if rep % 2 else both[::-1]):     # they take turns at going first
            got[k] = clock(fn)[0]
        got["step"] = clock(step)[0]
        if rep:
            for k in t:
                t[k].append(got[k])
    for e in (src, dst, cold_eng):
        e.close()
    return {
        "shape": f"{name} {m}x{ns}", "m": m, "ns": ns, "lps": B, "place": place, "cuts": 2,
        "optimal_lps": int(np.count_nonzero(ok)), "infeasible_lps": int(np.count_nonzero(ra[0] == _lib.INFEASIBLE)),
        "largest_relative_objective_difference": float(err.max()) if ok.any() else 0.0,
        "lps_checked_bit_for_bit_against_the_host": min(CHECKED, B),
        "warm_s": med(t["a"]), "warm_s_runs": t["a"], "cold_s": med(t["b"]), "cold_s_runs": t["b"],
        "warm_over_cold": med(t["a"]) / med(t["b"]),
        "slowest_warm_over_fastest_cold": max(t["a"]) / min(t["b"]),
        "extend_call_s": med(t["step"]), "extend_call_s_runs": t["step"],
        "warm_pivots_per_lp": float(np.mean(ra[1])), "cold_pivots_per_lp": float(np.mean(rb[1])),
        "lps_without_a_warm_pivot": int(np.count_nonzero(np.asarray(ra[1]) == 0)),
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("cut_bench.py needs a GPU")
    trace = "--trace" in sys.argv[1:]
    out = [bench(*w, trace=trace) for w in WORKLOADS]
    if trace:
        print(json.dumps({"bench": "cut_bench", "trace_only": True, "workloads": out}))
        return 0
    print(json.dumps({"bench": "cut_bench", "reps": REPS, "workloads": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
