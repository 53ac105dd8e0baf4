#!/usr/bin/env python3
"""Ragged batches against what a caller had before them: group the LPs by shape
on the host and run one BatchEngine per shape.

Seeded workloads (generators "mixed", seeds 1..B), in one process, alternating:

  (i)   16384 LPs whose shapes cycle through 8x10, 16x16, 24x32 and 40x40
  (ii)  1024 LPs no two of which share a shape, m in 4..35, ns in 6..37
  (iii) the uniform 8x10 (16384 LPs) and 40x40 (4096 LPs) batches of
        batch_bench.py run through the ragged path: the price of the table
        lookup, solve alone, against the lp_batch path (both uploaded first,
        the two solves taking turns to go first)

For (i) and (ii) the ragged side is one reused RaggedEngine: upload + solve +
download (host clock, every call synchronous), and the solve alone.  The
grouped side reuses one BatchEngine per shape (created outside the timed
region): stack each group on the host, upload + solve + download per engine,
and hand the results back in the caller's order; its "solve alone" is the sum
of its engines' solves.  Outside the timed regions the two sides' tableaux are
compared bit for bit.  Medians of --reps runs after one warm-up.  Prints one
JSON line (profiles/r09/ragged_bench.json).
Run it once, under a time limit:  timeout 500 python scripts/ragged_bench.py
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

from lpsol_amd import _lib                       # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402

CAP = 4096
CYCLE = [(8, 10), (16, 16), (24, 32), (40, 40)]


def med(xs):
    return statistics.median(xs)


def mixture_cycle(B=16384):
    """LP i is mixed(m, ns, seed i + 1) with (m, ns) = CYCLE[i % 4]"""
    lps = [None] * B
    for k, (m, ns) in enumerate(CYCLE):
        idx = range(k, B, len(CYCLE))
        stack = gen.mixed_stack(m, ns, [i + 1 for i in idx])
        for j, i in enumerate(idx):
            lps[i] = stack[j]
    return lps


def mixture_distinct():
    """1024 LPs, every (m, ns) of 4..35 x 6..37 once, in a seeded shuffle"""
    shapes = [(m, ns) for m in range(4, 36) for ns in range(6, 38)]
    order = np.random.default_rng(9).permutation(len(shapes))
    return [gen.tableau("mixed", *shapes[k], 1 + i) for i, k in enumerate(order)]


def bench_mixture(name, lps, reps):
    B = len(lps)
    shapes = [(T.shape[0] - 1, T.shape[1] - 1) for T in lps]
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    reng = _lib.RaggedEngine(shapes)
    gengs = {s: _lib.BatchEngine(len(idx), s[0], s[1]) for s, idx in groups.items()}
    t_r, t_rs, t_g, t_gs = [], [], [], []
    piv = 0
    for rep in range(reps + 1):                 # rep 0 is the warm-up
        t0 = time.perf_counter()
        reng.upload(lps)
        t1 = time.perf_counter()
        st, npiv, _ = reng.solve(CAP)
        t2 = time.perf_counter()
        got = reng.download()
        t3 = time.perf_counter()
        # the alternative: group on the host, one engine per shape, results back in order
        out = [None] * B
        gstatus = np.empty(B, dtype=np.int32)
        solves = 0.0
        for s, idx in groups.items():
            stack = np.stack([lps[i] for i in idx])
            e = gengs[s]
            e.upload(stack)
            ta = time.perf_counter()
            gst, gnpiv, _ = e.solve(CAP)
            solves += time.perf_counter() - ta
            res = e.download()
            gstatus[idx] = gst
            for k, i in enumerate(idx):
                out[i] = res[k]
        t4 = time.perf_counter()
        if rep:
            t_r.append(t3 - t0)
            t_rs.append(t2 - t1)
            t_g.append(t4 - t3)
            t_gs.append(solves)
        # checks, outside the timed regions
        assert np.array_equal(st, gstatus) and _lib.CAP_REACHED not in st.tolist()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, out)), "ragged and grouped tableaux differ"
        piv = int(npiv.sum())
    plan = reng.plan()
    reng.close()
    for e in gengs.values():
        e.close()
    r, rs, g, gs = med(t_r), med(t_rs), med(t_g), med(t_gs)
    return {
        "mixture": name, "lps": B, "shapes": len(groups), "pivots": piv, "bins": plan,
        "ragged_end_to_end_s": r, "ragged_solve_s": rs, "grouped_end_to_end_s": g, "grouped_solve_s": gs,
        "ragged_lps_per_s": B / r, "ragged_solve_only_lps_per_s": B / rs,
        "grouped_lps_per_s": B / g, "grouped_solve_only_lps_per_s": B / gs,
        "ragged_over_grouped_end_to_end": g / r, "ragged_over_grouped_solve": gs / rs,
        "bit_identical_to_grouped": True,
    }


def bench_uniform(m, ns, B, reps):
    stack = gen.mixed_stack(m, ns, range(1, B + 1))
    n = ns + m
    beng = _lib.BatchEngine(B, m, n)
    reng = _lib.RaggedEngine([(m, n)] * B)
    lps = list(stack)
    t_b, t_r = [], []
    for rep in range(reps + 1):
        beng.upload(stack)      # both uploads first: each solve starts from the same host state
        reng.upload(lps)
        for which in ((0, 1) if rep % 2 else (1, 0)):   # and the two take turns to go first
            t0 = time.perf_counter()
            (reng if which else beng).solve(CAP)
            dt = time.perf_counter() - t0
            if rep:
                (t_r if which else t_b).append(dt)
        assert np.array_equal(beng.download(), np.stack(reng.download())), "ragged and lp_batch tableaux differ"
    plan = reng.plan()
    beng.close()
    reng.close()
    b, r = med(t_b), med(t_r)
    return {
        "shape": f"{m}x{ns}", "lps": B, "bins": plan,
        "batch_solve_s": b, "batch_solve_min_s": min(t_b), "batch_solve_max_s": max(t_b),
        "ragged_solve_s": r, "ragged_solve_min_s": min(t_r), "ragged_solve_max_s": max(t_r),
        "ragged_over_batch_time": r / b,
        "inside_batch_spread": min(t_b) <= r <= max(t_b),
        "bit_identical_to_batch": True,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions per workload (median)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if _lib.device_count() < 1:
        raise SystemExit("ragged_bench.py needs a GPU")
    rows = [bench_mixture("cycle_8x10_16x16_24x32_40x40", mixture_cycle(), args.reps),
            bench_mixture("distinct_1024", mixture_distinct(), args.reps)]
    uni = [bench_uniform(8, 10, 16384, args.reps), bench_uniform(40, 40, 4096, args.reps)]
    print(json.dumps({"bench": "ragged_bench", "reps": args.reps, "mixtures": rows, "uniform": uni}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
