#!/usr/bin/env python3
"""Warm re-solve against a cold solve of the same LPs with new right-hand sides.

Four seeded workloads (generators.mixed_stack, seeds 1..B; the perturbations
of tests/_dual_cases.py, LP i on seed 1 + i): mixed 8x10 x 16384 and 40x40 x
4096 under place="lds" and 100x100 x 2048 under place="auto" with `scale`
(b_i * U{0..128}/64, so b >= 0), and 40x40 x 4096 with `shift` (b_i -
U{0..64}/64 on a quarter of the rows, so some b < 0).  For each, in one process
on one reused engine, 5 timed repetitions after a warm-up (host clock, every
call synchronous), the legs alternating and taking turns at going first:

  (a) warm: set_rhs + run(RULE_DUAL, cap) + solution(), from the optimal
      tableaux and basis of the original LPs, put back before each repetition
      outside the timed region
  (b) cold: what the library offered before -- upload_problems with the new b
      + derive_basis + solve + solution() where b >= 0 (the plain path, its
      cheapest), upload_problems + the two-phase solve + solution() for `shift`
  set_rhs alone and the dual run alone, in repetitions of their own

Before anything is timed (a) is checked on the first 16 LPs against the host
loop and the host walk of tests/_dual_cases.py, bit for bit: status, pivots, x
and objective.  (a)'s verdicts and optima are compared with (b)'s over the
whole batch and the figures reported.  The condition: the slowest of (a)'s
five is not above the fastest of (b)'s five.

Prints one JSON line (profiles/r18/dual_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/dual_bench.py
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

from lpsol_amd import _lib, solution_x           # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402
import _dual_cases as dc                         # noqa: E402

# m, ns, LPs, place, perturbation
WORKLOADS = [(8, 10, 16384, "lds", "scale"), (40, 40, 4096, "lds", "scale"), (100, 100, 2048, "auto", "scale"),
             (40, 40, 4096, "lds", "shift")]
CAP = 1 << 16
REPS = 5
CHECKED = 16


def med(xs):
    return statistics.median(xs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def bench(m, ns, B, place, how):
    T = gen.mixed_stack(m, ns, range(1, B + 1))
    n = T.shape[2] - 1
    P = np.ascontiguousarray(T[:, :, :ns + 1])
    b2 = np.stack([dc.PERTURB[how](T[i, 1:, 0], 1 + i) for i in range(B)])
    P2 = P.copy()
    P2[:, 1:, 0] = b2
    rhs = np.ascontiguousarray(P2[:, :, 0])             # the stored _z cell (+0.0), then the new b
    sense = np.zeros(m, dtype=np.int8)
    slack = dc.slack_table(sense, ns)
    plain = how == "scale"
    placed = place != "lds"
    cap = 10 * (m + n)

    eng = _lib.BatchEngine(B, m, n, place=place)
    eng.set_senses(sense)
    eng.upload_problems(P)
    assert eng.derive_basis()[1] < 0
    st0, cold0, _ = eng.solve(CAP)
    assert (st0 == _lib.OPTIMAL).all()
    Topt, basis = eng.download(), eng.get_basis()

    def restore():
        eng.upload(Topt)
        eng.set_basis(basis)

    def leg_a():
        eng.set_rhs(rhs)
        out = eng.run(_lib.RULE_DUAL, cap)
        return out, eng.solution()

    def leg_b():
        eng.upload_problems(P2)
        if plain:
            eng.derive_basis()
            st, npiv, _ = eng.solve(CAP)
            return (st, npiv), eng.solution()
        st, _, _, ninit, npiv, _ = (eng.solve_lp_placed if placed else eng.solve_lp)(CAP)
        return (st, ninit + npiv), eng.solution()

    # the checks, before anything is timed
    restore()
    (sa, da), (xa, za) = leg_a()
    for i in range(CHECKED):
        w = dc.walk(dc.set_rhs(Topt[i], slack, rhs[i]), cap)
        bs = basis[i].copy()
        for r, c in w["log"]:
            bs[r] = c
        assert (sa[i], da[i]) == (w["status"], w["npiv"]), "status or pivots differ from the host walk"
        assert dc.same_bits(xa[i], solution_x(w["T"], bs)) and dc.same_bits(za[i], -w["T"][0, 0]), "bits differ"
    (sb, pb), (xb, zb) = leg_b()
    # over the whole batch the two legs are compared and the figures reported: these seeds are not vetted
    # one by one, and a verdict within a tolerance of the boundary may fall either way
    differ = int(np.count_nonzero((sa == _lib.INFEASIBLE) != (sb == _lib.INFEASIBLE)))
    both = (sa == _lib.OPTIMAL) & (sb == _lib.OPTIMAL)
    other = int(np.count_nonzero(~np.isin(sa, (_lib.OPTIMAL, _lib.INFEASIBLE))))
    rel = float(np.max(np.abs(za[both] - zb[both]) / np.maximum(1.0, np.abs(zb[both]))))

    keys = ("a", "b", "set_rhs", "dual_run")
    t = {k: [] for k in keys}
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        got = {}
        for k in (("a", "b") if rep % 2 else ("b", "a")):       # they take turns at going first
            if k == "a":
                restore()
                got["a"] = clock(leg_a)[0]
            else:
                got["b"] = clock(leg_b)[0]
        restore()
        got["set_rhs"] = clock(lambda: eng.set_rhs(rhs))[0]
        got["dual_run"] = clock(lambda: eng.run(_lib.RULE_DUAL, cap))[0]
        if rep:
            for k in keys:
                t[k].append(got[k])
    eng.close()
    ms = {k: [1e3 * v for v in t[k]] for k in keys}
    return {
        "shape": f"mixed {m}x{ns}", "m": m, "n": n, "lps": B, "place": place, "perturbation": how,
        "cold_path": "plain" if plain else "twophase",
        "infeasible_lps": int(np.count_nonzero(sa == _lib.INFEASIBLE)),
        "lps_needing_a_dual_pivot": int(np.count_nonzero(da > 0)),
        "warm_pivots_mean": float(np.mean(da)), "warm_pivots_max": int(np.max(da)),
        "cold_pivots_mean": float(np.mean(pb)), "cold_pivots_max": int(np.max(pb)),
        "original_solve_pivots_mean": float(np.mean(cold0)),
        "warm_ms": med(ms["a"]), "warm_ms_runs": ms["a"],
        "cold_ms": med(ms["b"]), "cold_ms_runs": ms["b"],
        "set_rhs_ms": med(ms["set_rhs"]), "set_rhs_ms_runs": ms["set_rhs"],
        "dual_run_ms": med(ms["dual_run"]), "dual_run_ms_runs": ms["dual_run"],
        "warm_over_cold": med(ms["a"]) / med(ms["b"]),
        "slowest_warm_over_fastest_cold": max(ms["a"]) / min(ms["b"]),
        "condition_met": max(ms["a"]) <= min(ms["b"]),
        "max_relative_objective_difference": rel, "verdicts_that_differ": differ,
        "warm_lps_neither_optimal_nor_infeasible": other,
        "bit_identical_to_host_walk_on": CHECKED,
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("dual_bench.py needs a GPU")
    out = [bench(*w) for w in WORKLOADS]
    print(json.dumps({"bench": "dual_bench", "reps": REPS, "workloads": out,
                      "warm_never_slower_than_cold": all(r["condition_met"] for r in out)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
