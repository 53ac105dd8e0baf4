#!/usr/bin/env python3
"""Batches of LPs too large for one CU's LDS: place="auto" against what there
was before it, and the same shape under both placements at the boundary.

Part 1, three seeded workloads (generators.mixed_stack, seeds 1..B): 100x100
(B = 2048), 150x150 (B = 1024) and 256x256 (B = 256) structural.  For each, in
one process and alternating, the median of 5 after a warm-up:

  (a) place="auto": upload + lp_batch_solve + download on one reused
      BatchEngine (host clock, every call synchronous), and the solve alone
  (b) what there was before: one reused Engine, upload + solve per LP, on a
      64-LP subset
  (c) oracle.f64.F64Tableau.solve on one host core, on a 16-LP subset (the
      256x256 oracle takes most of a second per LP)

and the achieved bytes/s of the update pass, 16 E pivots / solve time, against
the 8 TB/s peak.  Outside the timed regions (a)'s tableaux are checked bit for
bit against (b)'s on its subset and against (c)'s on its.

Part 2, the cliff: 40x40, 64x64 and the largest square `mixed` shape that
still fits LDS, each solved under place="lds" and place="device".

Prints one JSON line (profiles/r10/place_bench.json).  Run it once, under a
time limit:  timeout 600 python scripts/place_bench.py
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
from oracle.f64 import F64Tableau                # noqa: E402

WORKLOADS = [(100, 100, 2048), (150, 150, 1024), (256, 256, 256)]
SUBSET, HOST_SUBSET = 64, 16
CAP = 1 << 16
REPS = 5
HBM_PEAK = 8e12


def med(xs):
    return statistics.median(xs)


def largest_square_in_lds():
    k = 1
    while _lib.batch_lds_bytes(k + 1, 2 * (k + 1)) <= _lib.BATCH_LDS_MAX:
        k += 1
    return k


def bench(m, ns, B):
    stack = gen.mixed_stack(m, ns, range(1, B + 1))
    n = ns + m
    elems = (m + 1) * (n + 1)
    sub = stack[:SUBSET]

    # (c) one host core, on its subset
    want = np.empty_like(stack[:HOST_SUBSET])
    t0 = time.perf_counter()
    for i in range(HOST_SUBSET):
        o = F64Tableau(stack[i])
        o.solve(cap=CAP, logcap=CAP)
        want[i] = o.T
    t_c = time.perf_counter() - t0

    beng = _lib.BatchEngine(B, m, n, place="auto")
    assert beng.placement(0) == "device"
    eng = _lib.Engine(m, n)
    t_a, t_solve, t_b = [], [], []
    piv = sub_piv = 0
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        t0 = time.perf_counter()
        beng.upload(stack)
        t1 = time.perf_counter()
        st, npiv, _ = beng.solve(CAP)
        t2 = time.perf_counter()
        got = beng.download()
        t3 = time.perf_counter()
        sub_piv = 0
        for i in range(SUBSET):
            eng.upload(sub[i])
            sub_piv += eng.solve(CAP)[1]
        t4 = time.perf_counter()
        if rep:
            t_a.append(t3 - t0)
            t_solve.append(t2 - t1)
            t_b.append(t4 - t3)
        piv = int(npiv.sum())
        assert set(st.tolist()) == {_lib.OPTIMAL}
        assert np.array_equal(got[:HOST_SUBSET], want), "batch tableaux differ from the oracle"
    for i in range(SUBSET):
        eng.upload(sub[i])
        eng.solve(CAP)
        assert np.array_equal(eng.download(), got[i]), "single-LP engine differs from the batch"
    assert sub_piv == int(npiv[:SUBSET].sum())
    beng.close()
    eng.close()

    a, s, b = med(t_a), med(t_solve), med(t_b)
    return {
        "shape": f"{m}x{ns}", "m": m, "n": n, "lps": B, "elems": elems, "pivots": piv,
        "batch_end_to_end_s": a, "batch_solve_s": s, "batch_solve_s_runs": t_solve,
        "batch_lps_per_s": B / a, "batch_solve_only_lps_per_s": B / s,
        "batch_solve_only_lps_per_s_slowest": B / max(t_solve),
        "single_subset_lps": SUBSET, "single_subset_s": b, "single_subset_s_runs": t_b,
        "single_lps_per_s": SUBSET / b, "single_lps_per_s_fastest": SUBSET / min(t_b),
        "host_core_subset_lps": HOST_SUBSET, "host_core_s": t_c, "host_core_lps_per_s": HOST_SUBSET / t_c,
        "solve_only_over_single": (B / s) / (SUBSET / b),
        "slowest_solve_over_fastest_single": (B / max(t_solve)) / (SUBSET / min(t_b)),
        "end_to_end_over_single": (B / a) / (SUBSET / b),
        "solve_only_over_host_core": (B / s) / (HOST_SUBSET / t_c),
        "update_bytes_per_s": 16.0 * elems * piv / s,
        "fraction_of_hbm_peak": 16.0 * elems * piv / s / HBM_PEAK,
        "bit_identical_to_oracle_and_single": True,
    }


def cliff(m, ns, B):
    stack = gen.mixed_stack(m, ns, range(1, B + 1))
    row = {"shape": f"{m}x{ns}", "lps": B, "lds_bytes": _lib.batch_lds_bytes(m, ns + m)}
    engines = {p: _lib.BatchEngine(B, m, ns + m, place=p) for p in ("lds", "device")}
    ts = {p: [] for p in engines}
    outs = {}
    for rep in range(REPS + 1):
        for p, eng in engines.items():          # alternating
            eng.upload(stack)
            t0 = time.perf_counter()
            _, npiv, _ = eng.solve(CAP)
            if rep:
                ts[p].append(time.perf_counter() - t0)
            row["pivots"] = int(npiv.sum())
            outs[p] = eng.download()
    assert np.array_equal(outs["lds"], outs["device"]), "the two placements differ"
    for p, eng in engines.items():
        eng.close()
        row[p + "_solve_s"] = med(ts[p])
        row[p + "_solve_s_runs"] = ts[p]
        row[p + "_lps_per_s"] = B / med(ts[p])
    row["device_over_lds_time"] = row["device_solve_s"] / row["lds_solve_s"]
    return row


def main():
    if _lib.device_count() < 1:
        raise SystemExit("place_bench.py needs a GPU")
    rows = [bench(m, ns, B) for m, ns, B in WORKLOADS]
    k = largest_square_in_lds()
    cliffs = [cliff(40, 40, 4096), cliff(64, 64, 1024), cliff(k, k, 1024)]
    ok = all(r["slowest_solve_over_fastest_single"] > 1.0 for r in rows)
    print(json.dumps({"bench": "place_bench", "reps": REPS, "workloads": rows, "cliff": cliffs,
                      "batch_beats_single_everywhere": ok,
                      "lds_ahead_wherever_it_fits": all(c["device_over_lds_time"] > 1.0 for c in cliffs)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
