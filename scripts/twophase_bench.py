#!/usr/bin/env python3
"""Batched two-phase solve against the one-LP front-end and one host core.

Three seeded workloads of LPs that need phase 1 (generators.phase1_lp("ge", m,
ns, seed), seeds 1..B): 8x10, 24x24 and 40x40 structural.  For each, in one
process:

  (a) the batch path: upload + lp_twophase_solve + download on one reused
      BatchEngine (host clock, every call synchronous); the solve also alone
  (b) what there was before for these inputs, on a 256-LP subset:
      Simplex(Tableau.fromArray(T)) followed by solve(), per LP
  (c) oracle.phase1.solve_lp on one host core over the whole batch

(a) and (b) are the median of `reps` repetitions after a warm-up, (c) runs
once.  Outside the timed regions (a) is checked bit for bit against (c):
status, sizes, pivot counts, bases and tableaux.  The cap is the one the
oracle's wrapper has built in (2^20 pivots per solve).  Prints one JSON line
(profiles/r08/twophase_bench.json).  Run it once, under a time limit:
    timeout 600 python scripts/twophase_bench.py
"""
import argparse
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

from lpsol_amd import Simplex, Tableau, _lib     # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402
from oracle import phase1                        # noqa: E402

WORKLOADS = [(8, 10, 16384), (24, 24, 4096), (40, 40, 1024)]
SUBSET = 256
CAP = 1 << 20


def med(xs):
    return statistics.median(xs)


def bench(m, ns, B, reps):
    stack = np.stack([gen.phase1_lp("ge", m, ns, s) for s in range(1, B + 1)])
    M, n = stack.shape[1] - 1, stack.shape[2] - 1
    sub = stack[:SUBSET]

    # (c) one host core, once
    t0 = time.perf_counter()
    want = [phase1.solve_lp(stack[i]) for i in range(B)]
    t_c = time.perf_counter() - t0
    assert not any("error" in o for o in want), "a workload LP is infeasible"
    ninit = sum(len(o["init_seq"]) for o in want)
    npiv = sum(len(o["seq"]) for o in want)

    beng = _lib.BatchEngine(B, M, n)
    t_a, t_solve, t_b = [], [], []
    for rep in range(reps + 1):                 # rep 0 is the warm-up
        t0 = time.perf_counter()
        beng.upload(stack)
        t1 = time.perf_counter()
        st, stage, rows, ni, nP, _ = beng.solve_lp(CAP)
        t2 = time.perf_counter()
        got = beng.download()
        t3 = time.perf_counter()
        for i in range(SUBSET):
            Simplex(Tableau.fromArray(sub[i])).solve()
        t4 = time.perf_counter()
        if rep:
            t_a.append(t3 - t0)
            t_solve.append(t2 - t1)
            t_b.append(t4 - t3)
    # checks, outside the timed regions
    basis = beng.get_basis()
    assert set(st.tolist()) == {_lib.OPTIMAL} and set(stage.tolist()) == {_lib.STAGE_PHASE2}
    for i, o in enumerate(want):
        mp = o["init_size"][0]
        assert rows[i] == mp and ni[i] == len(o["init_seq"]) and nP[i] == len(o["seq"]), i
        assert basis[i, :mp].tolist() == o["bfs"], i
        assert np.array_equal(got[i, :mp + 1].view(np.uint64), o["T"].view(np.uint64)), \
            f"LP {i}: batch tableau differs from the oracle"
    beng.close()

    a, s, b = med(t_a), med(t_solve), med(t_b)
    return {
        "shape": f"{m}x{ns}", "m": M, "n": n, "lps": B, "phase1_pivots": ninit, "phase2_pivots": npiv,
        "waves": _lib.twophase_waves(M, n), "lds_bytes": _lib.twophase_lds_bytes(M, n),
        "batch_end_to_end_s": a, "batch_solve_s": s,
        "batch_lps_per_s": B / a, "batch_solve_only_lps_per_s": B / s,
        "batch_solve_only_pivots_per_s": (ninit + npiv) / s,
        "frontend_subset_lps": SUBSET, "frontend_subset_s": b, "frontend_lps_per_s": SUBSET / b,
        "host_core_s": t_c, "host_core_lps_per_s": B / t_c,
        "batch_over_frontend": (B / a) / (SUBSET / b),
        "batch_over_host_core": (B / a) / (B / t_c),
        "bit_identical_to_oracle": True,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions per workload (median)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if _lib.device_count() < 1:
        raise SystemExit("twophase_bench.py needs a GPU")
    rows = [bench(m, ns, B, args.reps) for m, ns, B in WORKLOADS]
    ok = all(r["batch_over_frontend"] >= 1.0 for r in rows)
    print(json.dumps({"bench": "twophase_bench", "reps": args.reps, "workloads": rows,
                      "batch_not_slower_than_frontend_anywhere": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
