#!/usr/bin/env python3
"""Two-phase batches above the LDS limit: place="auto" (lp_phased_solve, the
working tableau in device memory) against what there was before it, and one
shape under both placements at the boundary.

Part 1, three seeded workloads of LPs that need phase 1
(generators.phase1_lp("ge", s, s, seed), seeds 1..B): s = 100 (B = 1024), 150
(B = 512) and 256 (B = 128).  For each, in one process and alternating, the
median of 5 after a warm-up:

  (a) place="auto": upload + lp_phased_solve + download on one reused
      BatchEngine (host clock, every call synchronous), and the solve alone
  (b) what there was before for these inputs, on a 16-LP subset:
      Simplex(Tableau.fromArray(T)) followed by solve(), per LP
  (c) oracle.phase1.solve_lp on one host core, on an 8-LP subset (once)

Outside the timed regions (a) is checked bit for bit against (c) on its subset:
status, stage, rows, pivot counts, bases and tableaux.  Every device call is
capped (CAP pivots per solve); the statuses of the whole batch are reported.

Part 2, the step at the boundary: ge(80, 80), the largest square `ge` shape
whose widened tableau still fits LDS, solved under place="lds" and
place="device", solve alone.

Prints one JSON line (profiles/r11/phased_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/phased_bench.py
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

from lpsol_amd import Simplex, Tableau, _lib     # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402
from oracle import phase1                        # noqa: E402

WORKLOADS = [(100, 1024), (150, 512), (256, 128)]
SUBSET, HOST_SUBSET = 16, 8
CAP = 1 << 14
REPS = 5
BOUNDARY = (80, 1024)


def med(xs):
    return statistics.median(xs)


def stack_of(s, B):
    return np.stack([gen.phase1_lp("ge", s, s, seed) for seed in range(1, B + 1)])


def bench(s, B):
    stack = stack_of(s, B)
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    sub = stack[:SUBSET]

    # (c) one host core, on its subset
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        want = [phase1.solve_lp(stack[i], None, cap=CAP, report=True) for i in range(HOST_SUBSET)]
    t_c = time.perf_counter() - t0
    assert all((o["status"], o["stage"]) == (_lib.OPTIMAL, _lib.STAGE_PHASE2) for o in want)

    beng = _lib.BatchEngine(B, m, n, place="auto")
    assert beng.phased_placement(0) == "device"
    t_a, t_solve, t_b = [], [], []
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        t0 = time.perf_counter()
        beng.upload(stack)
        t1 = time.perf_counter()
        st, stage, rows, ni, nP, _ = beng.solve_lp_placed(CAP)
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
    for i, o in enumerate(want):
        r = o["rows"]
        assert (st[i], stage[i], rows[i]) == (o["status"], o["stage"], r), i
        assert (ni[i], nP[i]) == (len(o["init_seq"]), len(o["seq"])), i
        assert basis[i].tolist() == o["bfs"], i
        assert np.array_equal(got[i, :r + 1].view(np.uint64), o["T"].view(np.uint64)), \
            f"LP {i}: batch tableau differs from the oracle"
    plan = beng.plan_phased()
    beng.close()

    a, sv, b = med(t_a), med(t_solve), med(t_b)
    piv = int(ni.sum() + nP.sum())
    elems = (m + 1) * (n + 1 + m)
    return {
        "shape": f"ge({s},{s})", "m": m, "n": n, "lps": B, "widened_elems": elems,
        "twophase_lds_bytes": _lib.twophase_lds_bytes(m, n), "phased_lds_bytes": _lib.phased_lds_bytes(m, n),
        "waves": plan[0]["waves"], "lps_per_cu": plan[0]["lps_per_cu"],
        "statuses": {_lib.STATUS_NAMES[int(k)]: int(v) for k, v in zip(*np.unique(st, return_counts=True))},
        "phase1_pivots": int(ni.sum()), "phase2_pivots": int(nP.sum()),
        "batch_end_to_end_s": a, "batch_solve_s": sv, "batch_solve_s_runs": t_solve,
        "batch_lps_per_s": B / a, "batch_solve_only_lps_per_s": B / sv,
        "batch_solve_only_lps_per_s_slowest": B / max(t_solve),
        "batch_solve_only_pivots_per_s": piv / sv,
        "frontend_subset_lps": SUBSET, "frontend_subset_s": b, "frontend_subset_s_runs": t_b,
        "frontend_lps_per_s": SUBSET / b, "frontend_lps_per_s_fastest": SUBSET / min(t_b),
        "host_core_subset_lps": HOST_SUBSET, "host_core_s": t_c, "host_core_lps_per_s": HOST_SUBSET / t_c,
        "solve_only_over_frontend": (B / sv) / (SUBSET / b),
        "end_to_end_over_frontend": (B / a) / (SUBSET / b),
        "slowest_end_to_end_over_fastest_frontend": (B / max(t_a)) / (SUBSET / min(t_b)),
        "end_to_end_over_host_core": (B / a) / (HOST_SUBSET / t_c),
        "bit_identical_to_oracle_on_subset": True,
    }


def boundary(s, B):
    stack = stack_of(s, B)
    m, n = stack.shape[1] - 1, stack.shape[2] - 1
    assert _lib.twophase_lds_bytes(m, n) <= _lib.BATCH_LDS_MAX < _lib.twophase_lds_bytes(m + 1, n + 2)
    row = {"shape": f"ge({s},{s})", "m": m, "n": n, "lps": B, "twophase_lds_bytes": _lib.twophase_lds_bytes(m, n)}
    engines = {p: _lib.BatchEngine(B, m, n, place=p) for p in ("lds", "device")}
    ts = {p: [] for p in engines}
    outs = {}
    for rep in range(REPS + 1):
        for p, eng in engines.items():          # alternating
            eng.upload(stack)
            t0 = time.perf_counter()
            st, _, _, ni, nP, _ = eng.solve_lp_placed(CAP)
            if rep:
                ts[p].append(time.perf_counter() - t0)
            row["pivots"] = int(ni.sum() + nP.sum())
            outs[p] = (st.tolist(), eng.download())
    assert outs["lds"][0] == outs["device"][0] and np.array_equal(outs["lds"][1], outs["device"][1]), \
        "the two placements differ"
    for p, eng in engines.items():
        eng.close()
        row[p + "_solve_s"] = med(ts[p])
        row[p + "_solve_s_runs"] = ts[p]
        row[p + "_lps_per_s"] = B / med(ts[p])
    row["device_over_lds_time"] = row["device_solve_s"] / row["lds_solve_s"]
    return row


def main():
    if _lib.device_count() < 1:
        raise SystemExit("phased_bench.py needs a GPU")
    rows = []
    for s, B in WORKLOADS:
        rows.append(bench(s, B))
        print(f"ge({s},{s}) x {B}: solve {rows[-1]['batch_solve_s']:.3f} s", file=sys.stderr, flush=True)
    edge = boundary(*BOUNDARY)
    ok = all(r["slowest_end_to_end_over_fastest_frontend"] > 1.0 for r in rows)
    print(json.dumps({"bench": "phased_bench", "reps": REPS, "cap": CAP, "workloads": rows, "boundary": edge,
                      "batch_beats_frontend_everywhere": ok,
                      "slowest_batch_over_fastest_frontend":
                          min(r["slowest_end_to_end_over_fastest_frontend"] for r in rows),
                      "lds_not_slower_where_it_fits": edge["device_over_lds_time"] >= 1.0}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
