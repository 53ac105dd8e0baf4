#!/usr/bin/env python3
"""Small batches of LPs too large for one CU's LDS: team="auto" against the
two roads there were before it.

`mixed` 100x100, 150x150 and 256x256 at B = 1, 4, 16, 64 and 256, and one
512x512 LP (generators.mixed_stack, seeds 1..B).  For each point, in one
process and alternating, 5 runs after a warm-up:

  (a) place="auto", team="auto": upload + lp_batch_solve + download on one
      reused BatchEngine (host clock, every call synchronous), and the solve
      alone
  (b) place="auto" with one workgroup per LP (team 1: the placed batch), the
      solve alone
  (c) one reused Engine, upload + solve per LP, over the same LPs

(a)'s tableaux are checked bit for bit against (b)'s outside the timed
regions.  Reported per point: the medians, every run, the team auto chose,
the time per launch of (a) (a launch is one pivot of every LP: the solve
takes as many as its longest LP has pivots), and whether (a)'s slowest solve
is within `SPREAD` of the fastest run of the better of (b) and (c) -- the
condition the auto rule has to meet at every point.

Prints one JSON line (profiles/r12/team_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/team_bench.py
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

from lpsol_amd import _lib                       # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402

POINTS = [(m, m, B) for m in (100, 150, 256) for B in (1, 4, 16, 64, 256)] + [(512, 512, 1)]
CAP = 1 << 16
REPS = 5
# the placed batch's own run-to-run spread, slowest over fastest of five solves:
# 1.009, 1.004 and 1.004 on the three workloads of profiles/r10/place_bench.json
SPREAD = 1.009


def point(m, ns, B):
    stack = gen.mixed_stack(m, ns, range(1, B + 1))
    n = ns + m
    auto = _lib.BatchEngine(B, m, n, place="auto", team="auto")
    solo = _lib.BatchEngine(B, m, n, place="auto")
    one = _lib.Engine(m, n)
    assert auto.placement(0) == solo.placement(0) == "device" and solo.team_of(0) == 1
    t_e2e, t_a, t_b, t_c = [], [], [], []
    npiv = None
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        t0 = time.perf_counter()
        auto.upload(stack)
        t1 = time.perf_counter()
        st, npiv, _ = auto.solve(CAP)
        t2 = time.perf_counter()
        got = auto.download()
        t3 = time.perf_counter()
        solo.upload(stack)
        t4 = time.perf_counter()
        _, npiv_b, _ = solo.solve(CAP)
        t5 = time.perf_counter()
        want = solo.download()
        t6 = time.perf_counter()
        for i in range(B):
            one.upload(stack[i])
            one.solve(CAP)
        t7 = time.perf_counter()
        if rep:
            t_e2e.append(t3 - t0)
            t_a.append(t2 - t1)
            t_b.append(t5 - t4)
            t_c.append(t7 - t6)
        assert set(st.tolist()) == {_lib.OPTIMAL} and np.array_equal(npiv, npiv_b)
        assert np.array_equal(got, want), "team=auto differs from the placed batch"
    team = auto.team_of(0)
    for e in (auto, solo, one):
        e.close()
    best_before = min(min(t_b), min(t_c))
    longest = int(npiv.max())
    return {
        "shape": f"{m}x{ns}", "m": m, "n": n, "lps": B, "elems": (m + 1) * (n + 1), "pivots": int(npiv.sum()),
        "launches": longest, "team": team,
        "auto_end_to_end_s": statistics.median(t_e2e), "auto_solve_s": statistics.median(t_a), "auto_solve_s_runs": t_a,
        "placed_solve_s": statistics.median(t_b), "placed_solve_s_runs": t_b,
        "single_s": statistics.median(t_c), "single_s_runs": t_c,
        "auto_us_per_launch": 1e6 * statistics.median(t_a) / longest,
        "speedup_over_placed": statistics.median(t_b) / statistics.median(t_a),
        "speedup_over_single": statistics.median(t_c) / statistics.median(t_a),
        "slowest_auto_over_fastest_before": max(t_a) / best_before,
        "auto_not_slower": max(t_a) <= best_before * SPREAD,
        "bit_identical_to_placed": True,
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("team_bench.py needs a GPU")
    rows = [point(m, ns, B) for m, ns, B in POINTS]
    ok = all(r["auto_not_slower"] for r in rows)
    print(json.dumps({"bench": "team_bench", "reps": REPS, "spread": SPREAD, "points": rows,
                      "auto_not_slower_anywhere": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
