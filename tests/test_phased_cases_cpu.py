"""The inputs of test_gpu_twophase_device.py still reach what they are there
for (tests/_phased_cases.py): each is above the two-phase LDS limit, and the
reporting oracle ends it where the case says.  No GPU."""
import pytest

import _phased_cases as pc
import _twophase_cases as tc
from lpsol_amd import _lib

LDS_, AUTO = _lib.PLACE_LDS, _lib.PLACE_AUTO
shape_of = pc.shape_of


def above_the_limit(T, shape, need):
    assert shape_of(T) == shape
    assert _lib.twophase_lds_bytes(*shape) == need > pc.LDS
    assert _lib.phased_on_device(AUTO, *shape) and not _lib.phased_too_large(AUTO, *shape)
    assert _lib.phased_too_large(LDS_, *shape)


def test_ge81_is_optimal_after_both_phases():
    stack = pc.ge81_stack()
    recs, cap = tc.oracle_batch(stack)
    for T, o in zip(stack, recs):
        above_the_limit(T, pc.GE_SHAPE, pc.GE_LDS)
        assert _lib.batch_lds_bytes(*pc.GE_SHAPE) <= pc.LDS         # LDS-placed for the plain call
        assert (o["status"], o["stage"], o["rows"]) == (tc.OPTIMAL, tc.PHASE2, 82)
        assert 86 <= len(o["init_seq"]) <= 94 and 193 <= len(o["seq"]) <= 249
        assert o["nart"] == len(o["init_seq"])                      # no drive-out pivot
    assert cap < 300


def test_drop_stack_drops_rows_and_drives_out():
    stack = pc.drop_stack()
    recs, cap = tc.oracle_batch(stack)
    for i, (T, o) in enumerate(zip(stack, recs)):
        above_the_limit(T, pc.DEP_SHAPE, pc.DEP_LDS)
        assert (o["status"], o["stage"], o["rows"]) == (tc.OPTIMAL, tc.PHASE2, pc.DROP_ROWS)
        assert len(o["init_seq"]) - o["nart"] == pc.DROP_DRIVE_OUT.get(i, 0)
        assert o["bfs"][pc.DROP_ROWS:] == [-1] * 56
        if i in pc.DROP_NART:
            assert o["nart"] == pc.DROP_NART[i]
    assert cap < tc.LOG_CAP * 2


@pytest.mark.parametrize("b", pc.large_batches(), ids=lambda b: b["name"])
def test_large_outcomes(b):
    recs, _ = tc.oracle_batch(b["stack"], b["tol"], b["cap"])
    for i, (T, o) in enumerate(zip(b["stack"], recs)):
        assert _lib.twophase_lds_bytes(*shape_of(T)) > pc.LDS
        if i in b["want"]:
            assert (o["status"], o["stage"]) == b["want"][i], i
        elif b["optimal_neighbours"]:
            assert (o["status"], o["stage"]) == (tc.OPTIMAL, tc.PHASE2), i


def test_cycling_lps_reach_any_cap():
    b = pc.large_batches()[0]
    for cap in (pc.CYCLE_CAP, 1500):
        for T in b["stack"][:2]:
            o = tc.report(T, None, cap)
            assert (o["status"], o["stage"], o["nart"]) == (tc.CAP_REACHED, tc.ARTIFICIAL, cap)


def test_ragged_list_mixes_the_placements():
    items = pc.ragged_list()
    toff, woff = pc.slot_offsets(items)
    dev = tuple(i for i, T in enumerate(items) if _lib.phased_on_device(AUTO, *shape_of(T)))
    assert dev == pc.RAGGED_DEVICE
    assert not any(_lib.phased_too_large(AUTO, *shape_of(T)) for T in items)
    plain_dev = [i for i, T in enumerate(items) if _lib.placed_on_device(AUTO, *shape_of(T))]
    assert plain_dev == [3]                                         # ge(100, 100): device for both calls
    assert shape_of(items[3]) == (101, 201)
    # a device LP at an odd offset into W and T (head = 1) and one at an even offset
    assert (toff[1] & 1, woff[1] & 1) == (1, 1)
    assert any(woff[i] & 1 == 0 for i in dev)
    assert {_lib.twophase_waves(*shape_of(items[i])) for i in (0, 2, 5, 7)} == {1, 4}
    recs, cap = tc.oracle_batch(items)
    assert cap <= pc.RAGGED_CAP
    assert all((o["status"], o["stage"]) == (tc.OPTIMAL, tc.PHASE2) for o in recs)
    assert recs[4]["rows"] < 116
