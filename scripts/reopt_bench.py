#!/usr/bin/env python3
"""Warm re-optimisation against a cold solve of the same LPs: new costs on the
stored tableaux (lp_reopt_set_costs, k_cost, then the primal solve from the
basis at hand) and a bound change on general-form LPs (lp_reopt_set_general,
k_general_restage + k_general_shift + k_rhs, then the dual simplex) against
uploading the changed LPs and solving them from the slack basis.

Four seeded workloads: `tilt` costs (c_j * U{0..128}/64 on each LP's own seed)
on mixed 8x10 x 16384 and 40x40 x 4096 in LDS and 100x100 x 2048 under
place="auto" (device-placed), and branch-down (ub_j = floor x_j of the first
fractional x_j) on all-BOXED [0, 2] mixed 24x24 x 4096.  For each, in one
process on one reused engine, 5 timed repetitions after a warm-up (host clock,
every call synchronous), the legs alternating and taking turns at going first:

  (a)  warm: from the optimum of the original LPs (restored, untimed, before
       every repetition): set_costs + solve + solution(), or set_general +
       run(RULE_DUAL) + general_solution()
  (b)  cold: upload of the changed LPs (upload_problems / upload_general) +
       derive_basis + solve + the same gather
  the set_costs / set_general call of (a) alone: one copy, its launches, one
  synchronise

Before anything is timed (a) is checked against (b): equal verdicts, and the
optima within 1e-9 relative.  Reported per workload: the medians, every run,
the pivots per LP of both legs and "slowest a / fastest b".  No figure here is
a condition of anything: the README states what was measured.

Prints one JSON line (profiles/r19/reopt_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/reopt_bench.py
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

BOXED = _lib.VAR_BOXED
# name, m, ns, LPs, place
WORKLOADS = [("tilt", 8, 10, 16384, "lds"), ("tilt", 40, 40, 4096, "lds"), ("tilt", 100, 100, 2048, "auto"),
             ("branch-down", 24, 24, 4096, "lds")]
S_TILT = 21
CAP = 1 << 16
REPS = 5
REL = 1e-9


def med(xs):
    return statistics.median(xs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def tilt(c, seed):
    i = np.arange(len(c), dtype=np.uint64)
    return c * (gen.uint_range(1000 + seed, S_TILT, i, 0, 128) / 64.0)


def agree(sa, za, sb, zb):
    assert np.array_equal(sa, sb), "verdicts differ"
    ok = sa == _lib.OPTIMAL
    err = np.abs(za[ok] - zb[ok]) / np.maximum(1.0, np.abs(zb[ok]))
    assert (err <= REL).all(), "optima differ"
    return float(err.max()) if ok.any() else 0.0


def costs_legs(m, ns, B, place):
    T = gen.mixed_stack(m, ns, range(1, B + 1))
    P = np.ascontiguousarray(T[:, :, :ns + 1])
    c2 = np.stack([tilt(P[i, 0, 1:], 1 + i) for i in range(B)])
    P2 = P.copy()
    P2[:, 0, 1:] = c2
    rows = np.concatenate([np.zeros((B, 1)), c2, np.zeros((B, m))], axis=1)
    eng = _lib.BatchEngine(B, m, ns + m, place=place)
    eng.set_senses(np.zeros(m, dtype=np.int8))

    def cold(blocks):
        eng.upload_problems(blocks)
        eng.derive_basis()
        return eng.solve(CAP), eng.solution()

    def restore():
        cold(P)

    def leg_a():
        eng.set_costs(rows)
        return eng.solve(CAP), eng.solution()

    return eng, restore, leg_a, lambda: cold(P2), lambda: eng.set_costs(rows)


def branch_legs(m, ns, B, place):
    T = gen.mixed_stack(m, ns, range(1, B + 1))
    P = np.ascontiguousarray(T[:, :, :ns + 1])
    sense, kind = np.zeros(m, dtype=np.int8), np.full(ns, BOXED, dtype=np.int8)
    lb, ub = np.zeros((B, ns)), np.full((B, ns), 2.0)
    rows, n = pr.general_shape(sense, kind)
    eng = _lib.BatchEngine(B, rows, n, place=place)
    eng.set_form(sense, kind, False)
    G = pr.pack_general(P, lb, ub)

    def cold(blocks):
        eng.upload_general(blocks)
        eng.derive_basis()
        (st, npiv, _) = eng.solve(CAP)
        return (st, npiv), eng.general_solution()

    x = cold(G)[1][0]
    frac = np.abs(x - np.round(x)) > 1e-6
    ub2 = ub.copy()
    for i in np.nonzero(frac.any(axis=1))[0]:
        j = int(np.argmax(frac[i]))
        ub2[i, j] = np.floor(x[i, j])
    G2 = pr.pack_general(P, lb, ub2)
    border = np.concatenate([P[:, 0, :], P[:, 1:, 0], lb, ub2], axis=1)
    cap = 10 * (rows + n)

    def leg_a():
        eng.set_general(border)
        return eng.run(_lib.RULE_DUAL, cap), eng.general_solution()

    return eng, lambda: cold(G), leg_a, lambda: cold(G2), lambda: eng.set_general(border)


def bench(name, m, ns, B, place, trace=False):
    eng, restore, leg_a, leg_b, step = (costs_legs if name == "tilt" else branch_legs)(m, ns, B, place)
    if trace:
        for _ in range(3):
            restore()
            leg_a()
        eng.close()
        return {"shape": f"{name} {m}x{ns}", "lps": B}
    # the check, before anything is timed
    restore()
    (ra, (_, za)), (rb, (_, zb)) = leg_a(), leg_b()
    err = agree(ra[0], za, rb[0], zb)
    t = {k: [] for k in ("a", "b", "step")}
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        legs = [("a", leg_a), ("b", leg_b)]
        got = {}
        for k, fn in (legs if rep % 2 else legs[::-1]):     # they take turns at going first
            if k == "a":
                restore()
            got[k] = clock(fn)[0]
        restore()
        got["step"] = clock(step)[0]
        if rep:
            for k in t:
                t[k].append(got[k])
    eng.close()
    return {
        "shape": f"{name} {m}x{ns}", "m": m, "ns": ns, "lps": B, "place": place,
        "optimal_lps": int(np.count_nonzero(ra[0] == _lib.OPTIMAL)),
        "largest_relative_objective_difference": err,
        "warm_s": med(t["a"]), "warm_s_runs": t["a"], "cold_s": med(t["b"]), "cold_s_runs": t["b"],
        "cold_over_warm": med(t["b"]) / med(t["a"]),
        "slowest_warm_over_fastest_cold": max(t["a"]) / min(t["b"]),
        "set_call_s": med(t["step"]), "set_call_s_runs": t["step"],
        "warm_pivots_per_lp": float(np.mean(ra[1])), "cold_pivots_per_lp": float(np.mean(rb[1])),
        "lps_without_a_warm_pivot": int(np.count_nonzero(np.asarray(ra[1]) == 0)),
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("reopt_bench.py needs a GPU")
    trace = "--trace" in sys.argv[1:]
    out = [bench(*w, trace=trace) for w in WORKLOADS]
    if trace:
        print(json.dumps({"bench": "reopt_bench", "trace_only": True, "workloads": out}))
        return 0
    print(json.dumps({"bench": "reopt_bench", "reps": REPS, "workloads": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
