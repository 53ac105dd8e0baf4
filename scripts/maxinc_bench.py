#!/usr/bin/env python3
"""The max-increase rule on the batch path (lp_batch_run with
LP_RULE_MAX_INCREASE) against what the single-LP engine offers for the rule,
and against the standard solve of the same LPs.

Seeded workloads (generators.mixed_stack, seeds 1..B): 8x10 x 16384, 40x40 x
4096 and 64x64 x 1024 structural under place="lds", and 100x100 x 2048 under
place="auto" (device-placed).  For each, in one process, 5 timed repetitions
after a warm-up (host clock, every call synchronous), the three taking turns at
going first:

  (a) on one reused BatchEngine: upload + derive_basis + run(RULE_MAX_INCREASE,
      cap) + solution(); and run() alone after an untimed upload
  (b) the rule without this path: one reused single-LP Engine, per LP upload +
      find_max_increase(do_pivot=True) until 'optimal', over the first 64 LPs
      of the batch only
  (c) on the engine of (a): upload + derive_basis + solve() + solution(), the
      standard rule with its stall switch; and solve() alone

Before anything is timed, (a)'s status, pivot count, log and final tableau of
the first 16 LPs are compared bit for bit with the host walk of
tests/_maxinc_cases.py; whether (b)'s pivot counts equal (a)'s is recorded.

Reported per shape: total pivots under each rule, us per pivot from the
solve-alone times, (a) over (c), and the condition against (b): the slowest of
(a)'s five whole-batch times is not above the fastest of (b)'s five 64-LP times.
There is no condition against (c).

Prints one JSON line (profiles/r14/maxinc_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/maxinc_bench.py
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

from lpsol_amd import _lib                       # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402
import _maxinc_cases as mc                       # noqa: E402

WORKLOADS = [(8, 10, 16384, "lds"), (40, 40, 4096, "lds"), (64, 64, 1024, "lds"), (100, 100, 2048, "auto")]
CAP = 1 << 16
REPS = 5
SUBSET = 64         # LPs of (b)
CHECKED = 16        # LPs compared with the host walk


def med(xs):
    return statistics.median(xs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def bench(m, ns, B, place):
    stack = gen.mixed_stack(m, ns, range(1, B + 1))
    n = ns + m
    eng = _lib.BatchEngine(B, m, n, log_cap=1024, place=place)
    one = _lib.Engine(m, n)

    def batch(call):
        eng.upload(stack)
        eng.derive_basis()
        out = call()
        eng.solution()
        return out

    def alone(call):
        eng.upload(stack)
        return clock(call)

    def single():
        counts = []
        for T in stack[:SUBSET]:
            one.upload(T)
            k = 0
            while one.find_max_increase(True) != "optimal":
                k += 1
            counts.append(k)
        return counts

    run = lambda: eng.run(_lib.RULE_MAX_INCREASE, CAP)     # noqa: E731
    solve = lambda: eng.solve(CAP)                          # noqa: E731

    # the checks, before anything is timed
    st, done = batch(run)
    assert set(st.tolist()) == {_lib.OPTIMAL}
    got = eng.download(0, CHECKED)
    for i in range(CHECKED):
        w = mc.walk(stack[i], CAP)
        assert (int(st[i]), int(done[i]), eng.log(i).tolist()) == (w["status"], w["npiv"], w["log"]), i
        assert mc.same_bits(got[i], w["T"]), i
    same_counts = single() == done[:SUBSET].tolist()
    st_c, npiv_c, _ = batch(solve)
    assert set(st_c.tolist()) == {_lib.OPTIMAL}

    t = {k: [] for k in ("a", "a_alone", "b", "c", "c_alone")}
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        steps = [("a", lambda: clock(lambda: batch(run))[0]), ("a_alone", lambda: alone(run)[0]),
                 ("c", lambda: clock(lambda: batch(solve))[0]), ("c_alone", lambda: alone(solve)[0]),
                 ("b", lambda: clock(single)[0])]
        for name, fn in (steps if rep % 2 else steps[::-1]):
            dt = fn()
            if rep:
                t[name].append(dt)
    eng.close()
    one.close()
    piv_a, piv_c, piv_b = int(done.sum()), int(npiv_c.sum()), int(done[:SUBSET].sum())
    return {
        "shape": f"{m}x{ns}", "m": m, "n": n, "lps": B, "place": place,
        "maxinc_s": med(t["a"]), "maxinc_s_runs": t["a"],
        "maxinc_run_alone_s": med(t["a_alone"]), "maxinc_run_alone_s_runs": t["a_alone"],
        "standard_s": med(t["c"]), "standard_s_runs": t["c"],
        "standard_solve_alone_s": med(t["c_alone"]), "standard_solve_alone_s_runs": t["c_alone"],
        "single_engine_lps": SUBSET, "single_engine_s": med(t["b"]), "single_engine_s_runs": t["b"],
        "pivots_maxinc": piv_a, "pivots_standard": piv_c, "pivots_single_engine": piv_b,
        "us_per_pivot_maxinc": 1e6 * med(t["a_alone"]) / piv_a,
        "us_per_pivot_standard": 1e6 * med(t["c_alone"]) / piv_c,
        "us_per_pivot_single_engine": 1e6 * med(t["b"]) / piv_b,
        "maxinc_over_standard": med(t["a"]) / med(t["c"]),
        "maxinc_over_standard_alone": med(t["a_alone"]) / med(t["c_alone"]),
        "slowest_maxinc_over_fastest_single_engine": max(t["a"]) / min(t["b"]),
        "condition_met": max(t["a"]) <= min(t["b"]),
        "bit_identical_to_walk": True, "single_engine_pivot_counts_equal": same_counts,
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("maxinc_bench.py needs a GPU")
    rows = []
    for w in WORKLOADS:
        rows.append(bench(*w))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    ok = all(r["condition_met"] for r in rows)
    print(json.dumps({"bench": "maxinc_bench", "reps": REPS, "workloads": rows,
                      "batch_never_slower_than_single_engine": ok}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
