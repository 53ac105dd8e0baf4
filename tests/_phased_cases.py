"""Shared inputs of the phased-batch tests (test_phased_cases_cpu.py,
test_gpu_twophase_device.py): LPs whose widened tableau is above one CU's LDS,
so that lp_twophase_solve refuses them and lp_phased_solve runs them from
device memory.  The shapes are the smallest above the limit: ge(81, 81) is
m = 82, n = 163 (167,104 bytes), dep(114, 60) and eq(115, 60) are m = 116,
n = 60 (168,616 bytes).  A plain module: no fixtures, no GPU.  Every input is
a generator call; a batch is _twophase_cases._batch's record."""
import numpy as np

import _twophase_cases as tc
from lpsol_amd import generators as gen

LDS = 160 * 1024
GE_SHAPE, DEP_SHAPE = (82, 163), (116, 60)
GE_LDS, DEP_LDS = 167104, 168616

U2, C2 = (tc.UNBOUNDED, tc.PHASE2), (tc.CAP_REACHED, tc.PHASE2)
UA, OA, CA = (tc.UNBOUNDED, tc.ARTIFICIAL), (tc.OBJ_INCREASED, tc.ARTIFICIAL), (tc.CAP_REACHED, tc.ARTIFICIAL)


def shape_of(T):
    """(m, n) of an engine-layout tableau"""
    return T.shape[0] - 1, T.shape[1] - 1


def ge81(seed):
    return gen.phase1_lp("ge", 81, 81, seed)


def ge81_stack(seeds=(1, 2, 3, 4)):
    """OPTIMAL in phase 2 after 86-94 phase-1 and 193-249 phase-2 pivots; no dropped rows"""
    return np.stack([ge81(s) for s in seeds])


# dep(114, 60) s = 1, 2 and eq(115, 60) s = 2, 4: OPTIMAL, 56 rows dropped,
# with drive-out pivots (7, 3, -, 4)
DROP_SPECS = [("dep", 114, 60, 1), ("dep", 114, 60, 2), ("eq", 115, 60, 2), ("eq", 115, 60, 4)]
DROP_ROWS = 60
DROP_DRIVE_OUT = {0: 7, 1: 3, 3: 4}     # LP -> drive-out pivots
DROP_NART = {0: 646, 1: 349}            # LP -> pivots of the artificial solve


def drop_stack():
    return np.stack([gen.phase1_lp(*s) for s in DROP_SPECS])


# these cycle in the artificial solve under the standard rule and the stall
# switch alike: (CAP_REACHED, ARTIFICIAL) under any cap, so a batch of their
# own with a small one
CYCLE_SPECS = [("eq", 115, 60, 1), ("eq", 115, 60, 3), ("dep", 114, 60, 3), ("dep", 114, 60, 4)]
CYCLE_CAP = 64


def large_batches():
    """the large outcomes other than OPTIMAL, as _twophase_cases.outcome_batches gives the small ones"""
    return [
        tc._batch("large_cycling", [gen.phase1_lp(*s) for s in CYCLE_SPECS], {i: CA for i in range(4)},
                  cap=CYCLE_CAP, optimal_neighbours=False),
        tc._batch("large_unbounded_phase2", [tc.unbounded("ge", 81, 81, s) for s in (1, 2, 3)], {1: U2, 2: U2}),
        tc._batch("large_cap_artificial", [ge81(1), ge81(2)], {0: CA, 1: CA}, cap=40, optimal_neighbours=False),
        tc._batch("large_cap_phase2", [ge81(1), ge81(2)], {0: C2, 1: C2}, cap=150, optimal_neighbours=False),
        tc._batch("large_pivot_minus_one", [ge81(1), ge81(2), ge81(3)], {0: UA, 1: OA, 2: OA},
                  tol=dict(pivot=-1.0), optimal_neighbours=False),
    ]


# ---------------------------------------------------------------------------
# the ragged list: small LPs that run two-phase in LDS, ge(81, 81) (plain LDS,
# phased device), ge(100, 100) (device for both), and device LPs at an odd and
# at an even offset into W and T
# ---------------------------------------------------------------------------

RAGGED_SPECS = [
    ("ge", 5, 6, 2),            # 0  LDS, one wave: slot 7 x 13 = 91 in T, 7 x 19 = 133 in W (both odd)
    ("ge", 81, 81, 1),          # 1  device: toff 91, woff 133 -> head 1
    ("eq", 10, 12, 3),          # 2  LDS
    ("ge", 100, 100, 1),        # 3  device for the plain call as well
    ("dep", 114, 60, 2),        # 4  device, rows dropped
    ("ge", 32, 32, 2),          # 5  LDS, four waves
    ("ge", 81, 81, 3),          # 6  device
    ("neg", 1, 1, 1),           # 7  LDS
]
RAGGED_DEVICE = (1, 3, 4, 6)
RAGGED_CAP = 600


def ragged_list():
    return [gen.phase1_lp(*s) for s in RAGGED_SPECS]


def slot_offsets(items):
    """-> (toff, woff) per LP: the packed offsets of lp_ragged_create, in doubles"""
    toff, woff, t, w = [], [], 0, 0
    for a in items:
        m, n = a.shape[0] - 1, a.shape[1] - 1
        toff.append(t)
        woff.append(w)
        t += (m + 1) * (n + 1)
        w += (m + 1) * (n + 1 + m)
    return toff, woff
