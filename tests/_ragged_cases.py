"""Shared inputs of the ragged-batch tests (test_ragged_plan_cpu.py,
test_gpu_ragged.py).  A plain module: no fixtures, no GPU.  Every input is a
generator call."""
from lpsol_amd import generators as gen

# the two-phase list: one-wave LPs of several shapes, an infeasible one, four
# four-wave LPs, and two 1x1 LPs at the end
TWOPHASE_SPECS = [
    ("ge", 3, 4, 1), ("ge", 5, 6, 2), ("ge", 8, 10, 3), ("eq", 5, 6, 4), ("dep", 3, 4, 5), ("neg", 5, 6, 6),
    ("infeasible", 2, 4, 1),
    ("ge", 24, 24, 7), ("eq", 10, 12, 3), ("dep", 6, 8, 2), ("neg", 16, 20, 1),
    ("ge", 32, 32, 2), ("eq", 31, 72, 1), ("ge", 40, 40, 3), ("dep", 33, 65, 1),
    ("neg", 1, 1, 1), ("ge", 1, 1, 1),
]
TWOPHASE_INFEASIBLE_AT = 6
TWOPHASE_DROPS_A_ROW = (4, 9, 14)       # the dep LPs
TWOPHASE_FOUR_WAVE = (11, 12, 13, 14)
TWOPHASE_CAP = 400


def twophase_list():
    return [gen.phase1_lp(*spec) for spec in TWOPHASE_SPECS]


def shape_of(T):
    """(m, n) of an engine-layout tableau"""
    return T.shape[0] - 1, T.shape[1] - 1
