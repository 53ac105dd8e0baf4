#!/usr/bin/env python3
"""Solve-only time of the device-placed batch kernel (k_batch_dev) over a
ladder of shapes, for the A/B of its waves per LP (the A/B of
the 16-byte accesses in its update pass was run with a one-double-per-access
build that batch.hip no longer carries).

Run once per library build, each in its own process, on the same box:

  make -C linear-program-solver_amd/csrc variant NAME=dev_w4 DEFS=-DLPK_BATCH_DEV_WAVES=4
  make -C linear-program-solver_amd/csrc variant NAME=dev_w8 DEFS=-DLPK_BATCH_DEV_WAVES=8
  make -C linear-program-solver_amd/csrc variant NAME=dev_w16 DEFS=-DLPK_BATCH_DEV_WAVES=16
  LPGPU_LIB=.../variants/dev_w4.so timeout 300 python scripts/place_waves.py
  ...

Prints one JSON line: per shape the median lp_batch_solve seconds of 5 after a
warm-up (tableaux re-uploaded before each), the LPs/s that gives and the
bytes/s of the update pass, 16 bytes per element and applied pivot.
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

# (m, ns, B): the chip filled several times over, then one LP per CU; the
# small shapes show what the kernel costs where LDS would have done
LADDER = [(100, 100, 2048), (150, 150, 1024), (256, 256, 256), (100, 100, 256), (150, 150, 256),
          (40, 40, 4096), (64, 64, 1024), (8, 10, 16384)]


def main():
    rows = []
    for m, ns, B in LADDER:
        stack = gen.mixed_stack(m, ns, range(1, B + 1))
        eng = _lib.BatchEngine(B, m, ns + m, place="device")
        waves = _lib.ragged_plan(eng)[0]["waves"]
        ts, piv = [], 0
        for rep in range(6):
            eng.upload(stack)
            t0 = time.perf_counter()
            _, npiv, _ = eng.solve(1 << 16)
            if rep:
                ts.append(time.perf_counter() - t0)
            piv = int(npiv.sum())
        eng.close()
        t = statistics.median(ts)
        elems = (m + 1) * (ns + m + 1)
        rows.append({"shape": f"{m}x{ns}", "elems": elems, "lps": B, "waves": waves, "pivots": piv,
                     "solve_s": t, "solve_s_min": min(ts), "solve_s_max": max(ts), "lps_per_s": B / t,
                     "update_bytes_per_s": 16.0 * elems * piv / t})
    print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "ladder": rows}))


if __name__ == "__main__":
    main()
