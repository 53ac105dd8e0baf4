#!/usr/bin/env python3
"""Solve-only time of the teamed batch kernel (k_batch_team) over team size,
launches per read-back and batch size, for the choice of LPK_TEAM_WAVES,
LPK_TEAM_MAX, LPK_TEAM_MIN_ELEMS and LPK_TEAM_WINDOW (knobs.h).

Run once per library build, each in its own process, on the same box:

  make -C linear-program-solver_amd/csrc variant NAME=team_w4 DEFS="-DLPK_TEAM_WAVES=4 -DLPK_TEAM_MAX=64"
  make -C linear-program-solver_amd/csrc variant NAME=team_w8 DEFS="-DLPK_TEAM_WAVES=8 -DLPK_TEAM_MAX=64"
  make -C linear-program-solver_amd/csrc variant NAME=team_w16 DEFS="-DLPK_TEAM_WAVES=16 -DLPK_TEAM_MAX=64"
  LPGPU_LIB=.../variants/team_w4.so timeout 600 python scripts/team_sweep.py
  ...

`mixed` 150x150 and 256x256 at B = 4, 16 and 64; team 1 (the placed path, one
workgroup per LP) and forced teams of 2 .. 64; 16, 64 and 256 launches per
read-back.  Prints one JSON line: per point the median lp_batch_solve seconds
of 5 after a warm-up (tableaux re-uploaded before each), the fastest and the
slowest, and the time per launch -- a launch is one pivot of every LP, so a
solve takes as many as its longest LP has pivots.  Every teamed result is
checked bit for bit against team 1's.
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

SHAPES = [(150, 150), (256, 256)]
BATCHES = [4, 16, 64]
TEAMS = [2, 4, 8, 16, 32, 64]
WINDOWS = [16, 64, 256]
CAP = 1 << 16
REPS = 5


def timed(eng, stack):
    ts, npiv = [], None
    for rep in range(REPS + 1):                  # rep 0 is the warm-up
        eng.upload(stack)
        t0 = time.perf_counter()
        st, npiv, _ = eng.solve(CAP)
        if rep:
            ts.append(time.perf_counter() - t0)
        assert set(st.tolist()) == {_lib.OPTIMAL}
    return ts, npiv


def main():
    if _lib.device_count() < 1:
        raise SystemExit("team_sweep.py needs a GPU")
    rows = []
    for m, ns in SHAPES:
        for B in BATCHES:
            stack = gen.mixed_stack(m, ns, range(1, B + 1))
            base = _lib.BatchEngine(B, m, ns + m, place="device")
            ts, npiv = timed(base, stack)
            want = base.download()
            base.close()
            longest = int(npiv.max())
            common = {"shape": f"{m}x{ns}", "elems": (m + 1) * (ns + m + 1), "lps": B, "pivots": int(npiv.sum()),
                      "launches": longest}
            rows.append(dict(common, team=1, window=None, solve_s=statistics.median(ts), solve_s_min=min(ts),
                             solve_s_max=max(ts)))
            for G in TEAMS:
                eng = _lib.BatchEngine(B, m, ns + m, place="device", team=G)
                for K in WINDOWS:
                    eng.set_window(K)
                    ts, got_piv = timed(eng, stack)
                    assert np.array_equal(got_piv, npiv) and np.array_equal(eng.download(), want), (m, B, G, K)
                    t = statistics.median(ts)
                    rows.append(dict(common, team=G, window=K, solve_s=t, solve_s_min=min(ts), solve_s_max=max(ts),
                                     us_per_launch=1e6 * t / longest))
                eng.close()
    print(json.dumps({"bench": "team_sweep", "lib": os.path.basename(_lib.LIB_PATH), "reps": REPS, "points": rows,
                      "bit_identical_to_team_1": True}))


if __name__ == "__main__":
    main()
