#!/usr/bin/env python3
"""Solve-only time of the device-placed two-phase kernel (k_twophase_dev) at
the three shapes of scripts/phased_bench.py, for the A/B of its waves per LP
and of the occupancy request.

Run once per library build, each in its own process, on the same box:

  make -C linear-program-solver_amd/csrc variant NAME=ph_w16 DEFS=-DLPK_PHASED_WAVES=16
  make -C linear-program-solver_amd/csrc variant NAME=ph_w16_occ8 \
      DEFS="-DLPK_PHASED_WAVES=16 -DLPK_PHASED_OCC8=1"
  make -C linear-program-solver_amd/csrc variant NAME=ph_w8 DEFS=-DLPK_PHASED_WAVES=8
  make -C linear-program-solver_amd/csrc variant NAME=ph_w8_occ8 \
      DEFS="-DLPK_PHASED_WAVES=8 -DLPK_PHASED_OCC8=1"
  LPGPU_LIB=.../variants/ph_w16.so timeout 300 python scripts/phased_waves.py
  ...

Prints one JSON line: per shape the median lp_phased_solve seconds of 5 after a
warm-up (tableaux re-uploaded before each) and the LPs/s that gives.
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

LADDER = [(100, 1024), (150, 512), (256, 128)]
CAP = 1 << 14


def main():
    rows = []
    for s, B in LADDER:
        stack = np.stack([gen.phase1_lp("ge", s, s, seed) for seed in range(1, B + 1)])
        m, n = stack.shape[1] - 1, stack.shape[2] - 1
        eng = _lib.BatchEngine(B, m, n, place="auto")
        plan = eng.plan_phased()[0]
        ts, piv = [], 0
        for rep in range(6):
            eng.upload(stack)
            t0 = time.perf_counter()
            st, _, _, ni, nP, _ = eng.solve_lp_placed(CAP)
            if rep:
                ts.append(time.perf_counter() - t0)
            piv = int(ni.sum() + nP.sum())
        not_optimal = int((st != _lib.OPTIMAL).sum())
        eng.close()
        t = statistics.median(ts)
        rows.append({"shape": f"ge({s},{s})", "lps": B, "waves": plan["waves"], "lps_per_cu": plan["lps_per_cu"],
                     "pivots": piv, "not_optimal": not_optimal, "solve_s": t, "solve_s_min": min(ts),
                     "solve_s_max": max(ts), "lps_per_s": B / t})
    print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "ladder": rows}))


if __name__ == "__main__":
    main()
