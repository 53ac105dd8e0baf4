#!/usr/bin/env python3
"""Solve-only time of the batch kernel over a ladder of shapes, for the A/B of
its one-wave / four-wave threshold (DESIGN.md "Batched solve").

Run once per library build, each in its own process, on the same box:

  make -C linear-program-solver_amd/csrc variant NAME=batch_w1 DEFS=-DLPGPU_BATCH_ONE_WAVE_ELEMS=1073741824
  make -C linear-program-solver_amd/csrc variant NAME=batch_w4 DEFS=-DLPGPU_BATCH_ONE_WAVE_ELEMS=0
  LPGPU_LIB=.../variants/batch_w1.so timeout 120 python scripts/batch_waves.py
  LPGPU_LIB=.../variants/batch_w4.so timeout 120 python scripts/batch_waves.py

Prints one JSON line: per shape the median lp_batch_solve seconds of 7 after a
warm-up (tableaux re-uploaded before each), and the LPs/s that gives.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "linear-program-solver_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from lpsol_amd import _lib                       # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402

# (m, ns, B): (m+1)(n+1) = 171, 561, 1425, 1881, 2145, 3321, 8385
LADDER = [(8, 10, 16384), (16, 16, 8192), (24, 32, 4096), (32, 24, 4096), (32, 32, 4096),
          (40, 40, 4096), (64, 64, 1024)]


def main():
    rows = []
    for m, ns, B in LADDER + [(m, ns, 256) for m, ns, _ in LADDER]:   # full chip, then one LP per CU
        stack = gen.mixed_stack(m, ns, range(1, B + 1))
        eng = _lib.BatchEngine(B, m, ns + m)
        ts, piv = [], 0
        for rep in range(8):
            eng.upload(stack)
            t0 = time.perf_counter()
            _, npiv, _ = eng.solve(4096)
            if rep:
                ts.append(time.perf_counter() - t0)
            piv = int(npiv.sum())
        eng.close()
        t = statistics.median(ts)
        rows.append({"shape": f"{m}x{ns}", "elems": (m + 1) * (ns + m + 1), "lps": B, "pivots": piv,
                     "solve_s": t, "lps_per_s": B / t})
    print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "ladder": rows}))


if __name__ == "__main__":
    main()
