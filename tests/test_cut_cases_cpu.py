"""The inputs of the warm-cut tests on the host oracle alone (tests/_cut_cases.py):
the LPs the GPU tests extend, walked with the host dual rule and compared
with a cold solve of the LPs with the rows added.

Measured here on the oracle (le and lege, 8x10 seeds 1..64, 24x24 seeds 1..32,
40x40 seeds 1..16): every warm verdict equals the cold one; the optima agree
within 3.9e-15 relative (the bound asserted is 1e-12); the longest warm walk
takes 41 pivots against a cap of 10 * (m' + n') >= 300; set_rhs on D with the
joined slack table and right-hand sides gives D's column 0 back within 1.3e-15
of the largest entry of the column (the bound asserted is 1e-12)."""
import numpy as np
import pytest

import _cut_cases as cc
import _dual_cases as dc
from lpsol_amd import _lib
from lpsol_amd.problem import extend_tableau

REL = 1e-12
SHAPES = [cc.SMALL, cc.MID, cc.LARGE]


def cases(shape, workload):
    return [cc.case(*shape, seed, workload) for seed in cc.SEEDS[shape]]


@pytest.mark.parametrize("workload", cc.WORKLOADS)
@pytest.mark.parametrize("shape", SHAPES, ids=["8x10", "24x24", "40x40"])
def test_warm_verdicts_and_optima_equal_the_cold_ones(shape, workload):
    worst, most, verdicts = 0.0, 0, []
    for c in cases(shape, workload):
        st, npiv, _, z = cc.warm_answer(c)
        cst, cz, _ = cc.cold(c, workload)
        assert st == cst, (shape, workload, st, cst)
        assert st in (_lib.OPTIMAL, _lib.INFEASIBLE)
        assert npiv < c["cap"]
        most = max(most, npiv)
        verdicts.append(st)
        if st == _lib.OPTIMAL:
            worst = max(worst, abs(z - cz) / max(1.0, abs(cz)))
    print("%s %s: worst relative difference %.3g, most warm pivots %d, %d optimal, %d infeasible"
          % (shape, workload, worst, most, verdicts.count(_lib.OPTIMAL), verdicts.count(_lib.INFEASIBLE)))
    assert worst <= REL
    if workload == "le":
        assert verdicts == [_lib.OPTIMAL] * len(verdicts)
    else:
        assert _lib.OPTIMAL in verdicts and _lib.INFEASIBLE in verdicts


def test_warm_takes_fewer_pivots_than_cold_on_average():
    for shape in SHAPES:
        cs = cases(shape, "le")
        warm = np.mean([c["warm"]["npiv"] for c in cs])
        cold = np.mean([cc.cold(c, "le")[2] for c in cs])
        print("%s le: mean pivots warm %.1f, cold %.1f" % (shape, warm, cold))
        assert warm < cold


def test_the_inputs_are_no_no_ops():
    """a condition on the inputs: the cuts cut the optimum off, so the GPU tests are not about walks of no pivot"""
    idle = [c["warm"]["npiv"] == 0 for c in cases(cc.SMALL, "lege")]
    assert sum(idle) <= 2
    assert all(c["warm"]["npiv"] > 0 for c in cases(cc.SMALL, "le"))


@pytest.mark.parametrize("workload", cc.WORKLOADS)
def test_the_new_columns_hold_the_basis_inverse(workload):
    """the M-reading of DESIGN.md 4q holds on D: set_rhs with the joined slack table and right-hand sides
    reproduces D's column 0 up to the order of summation"""
    worst = 0.0
    for shape in SHAPES:
        m, ns = shape
        for c in cases(shape, workload):
            slack = dc.slack_table(c["joined"], ns)
            rhs = np.concatenate([[c["T0"][0, 0]], c["T0"][1:, 0], c["beta"]])
            back = dc.set_rhs(c["D"], slack, rhs)
            scale = max(1.0, np.abs(c["D"][:, 0]).max())
            worst = max(worst, np.abs(back[:, 0] - c["D"][:, 0]).max() / scale)
            assert dc.same_bits(back[:, 1:], c["D"][:, 1:])
    print("%s: column 0 comes back within %.3g" % (workload, worst))
    assert worst <= REL


def test_extend_is_the_package_statement():
    """lpsol_amd.problem.extend_tableau (columns side by side) gives the scalar loop's bits"""
    for shape, seed, workload, q in ((cc.SMALL, 3, "lege", 2), (cc.MID, 4, "le", 3), ((1, 1), 5, "lege", 1),
                                     (cc.SMALL, 6, "le", 0), (cc.SMALL, 7, "lege", 5)):
        c = cc.case(*shape, seed, workload, q)
        D, basis = extend_tableau(c["opt"], c["basis"], c["rows"], c["sense"])
        assert dc.same_bits(D, c["D"]) and np.array_equal(basis, c["basis2"]) and basis.dtype == np.int32
    T, basis, rows, sense = cc.odd_case()
    D, _ = extend_tableau(T, basis, rows, sense)
    want, _ = cc.extend(T, basis, rows, sense)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(D), nan) and dc.same_bits(D[~nan], want[~nan])
    assert dc.same_bits(D[:4, :5], T)                           # the NaN and the -0.0 of T are copied as bits
    assert np.signbit(D[5, 0]) and D[5, 0] == 0.0              # a >= cut whose priced cell is +0.0 stores -0.0
    assert nan[4:, :5].any() and np.isinf(D[4, :5]).any()
    with pytest.raises(ValueError, match='"=="'):
        extend_tableau(T, basis, rows[:1], ["=="])
    with pytest.raises(ValueError, match="rows must be"):
        extend_tableau(T, basis, rows[:, :4], sense)
    with pytest.raises(ValueError, match="sense must hold"):
        extend_tableau(T, basis, rows, sense[:2])


# ---------------------------------------------------------------------------
# the inputs of test_gpu_batch_cut_edges.py: where the lanes of the flat kernels fall
# ---------------------------------------------------------------------------

def assert_lane_edges(batch, which, windows, edges, big, inside):
    """the conditions on a ragged batch and its windows, from the shapes alone"""
    B, F = len(batch), cc.FLAT
    assert all(0 <= first and count >= 1 and first + count <= B for first, count in windows), which
    assert any(first > 0 and cc.lane_starts(batch, which, first, count)[-1] > 2 * F for first, count in windows), which
    seen = set()
    for first, at in edges.items():
        count = next(c for f, c in windows if f == first)
        s = cc.lane_starts(batch, which, first, count)
        lanes = np.diff(s)
        assert all(a in s[:-1] and lanes[s.index(a):].any() for a in at), (which, first)    # an LP with lanes begins there
        seen |= set(at)
    assert {F - 1, F, F + 1} <= seen and seen & {2 * F - 1, 2 * F, 2 * F + 1}, (which, seen)
    whole = cc.lane_starts(batch, which, 0, B)
    assert cc.LANE_MAPS[which](*batch[big]) > F and (big, 1) in windows, which          # alone, more than a workgroup
    assert whole[big] // F != (whole[big + 1] - 1) // F, which                          # and in two of the whole batch
    assert F <= whole[inside] < whole[inside + 1] <= 2 * F and (inside, 1) in windows, which


def test_the_cut_blocks_cross_workgroups_where_they_say():
    assert cc.GROUP >= 1 and len(cc.BLOCK) == cc.BLOCK_WINDOWS[0][1] and cc.BLOCK[cc.BLOCK_BIG] == (260, 3, 1)
    for which in ("rows", "basis"):
        assert_lane_edges(cc.BLOCK, which, cc.BLOCK_WINDOWS, cc.BLOCK_EDGES[which], cc.BLOCK_BIG, cc.BLOCK_INSIDE)
    assert len(cc.COPY_BLOCK) == cc.COPY_WINDOWS[0][1]
    assert_lane_edges(cc.COPY_BLOCK, "copy", cc.COPY_WINDOWS, cc.COPY_EDGES, cc.COPY_BIG, cc.COPY_INSIDE)
    # the uniform source: windows of both maps in three workgroups, one with first > 0
    first, count = cc.UNIFORM_WINDOWS[1]
    assert len({s[:2] for s in cc.UNIFORM_BLOCK}) == 1 and first > 0
    for which in ("rows", "basis"):
        assert cc.lane_starts(cc.UNIFORM_BLOCK, which, first, count)[-1] > 2 * cc.FLAT
        assert cc.FLAT % cc.LANE_MAPS[which](*cc.UNIFORM_BLOCK[5]) != 0


def test_the_cut_blocks_have_runs_of_lps_without_a_row_where_they_say():
    for batch, windows, zeros, walked in ((cc.BLOCK, cc.BLOCK_WINDOWS, cc.BLOCK_ZEROS, cc.BLOCK_WALKED),
                                          (cc.UNIFORM_BLOCK, cc.UNIFORM_WINDOWS, cc.UNIFORM_ZEROS, cc.UNIFORM_WINDOWS[1])):
        assert zeros in windows and walked in windows
        assert all(q == 0 for _, _, q in batch[zeros[0]:zeros[0] + zeros[1]]) and zeros[1] >= 2
        starts_with = ends_with = middle = False
        for first, count in windows:
            if (first, count) == zeros:
                continue
            runs = cc.zero_runs(batch, first, count)
            rows = np.diff(cc.lane_starts(batch, "rows", first, count))
            starts_with |= any(at == 0 for at, n in runs)
            ends_with |= any(at + n == count for at, n in runs)
            middle |= any(rows[:at].any() and rows[at + n:].any() for at, n in runs)
        assert starts_with and ends_with and middle
    # the walked window of BLOCK has all three
    runs = cc.zero_runs(cc.BLOCK, *cc.BLOCK_WALKED)
    assert runs[0][0] == 0 and sum(runs[-1]) == cc.BLOCK_WALKED[1] and len(runs) >= 3


@pytest.mark.parametrize("name", ["block", "copy", "uniform"])
def test_the_cut_blocks_walk_to_both_verdicts_and_every_window_changes_something(name):
    batch, windows = dict(block=(cc.BLOCK, cc.BLOCK_WINDOWS), copy=(cc.COPY_BLOCK, cc.COPY_WINDOWS),
                          uniform=(cc.UNIFORM_BLOCK, cc.UNIFORM_WINDOWS))[name]
    cs = cc.block_cases(batch)          # (every source LP ends optimal on the oracle: case() asserts it)
    verdicts = [c["warm"]["status"] for c in cs]
    assert set(verdicts) == {_lib.OPTIMAL, _lib.INFEASIBLE}
    assert all(2 * c["warm"]["npiv"] < c["cap"] and c["warm"]["npiv"] <= dc.LOG_CAP for c in cs)
    assert all(2 * dc.walk(c["D"], dc.CAP)["npiv"] < dc.CAP for c in cs)       # the GPU tests' own cap
    for first, count in windows:
        w = cs[first:first + count]
        if all(c["rows"].shape[0] == 0 for c in w):
            continue                    # a window without a row: the destination is the source, which is the point
        assert any(c["rows"][0].any() for c in w if c["rows"].shape[0]), (first, count)     # row 0 of some LP's cuts
        assert any(c["warm"]["npiv"] > 0 for c in w) or count == 1, (first, count)
    # the window the GPU test walks: both verdicts, and LPs that pivot
    walked = dict(block=cc.BLOCK_WALKED, copy=cc.COPY_WINDOWS[1], uniform=cc.UNIFORM_WINDOWS[1])[name]
    w = cs[walked[0]:sum(walked)]
    assert {c["warm"]["status"] for c in w} == {_lib.OPTIMAL, _lib.INFEASIBLE}
    assert sum(c["warm"]["npiv"] > 0 for c in w) >= 10


def test_the_small_batches_a_gpu_test_walks_end_both_ways():
    both = {_lib.OPTIMAL, _lib.INFEASIBLE}
    zero = cc.block_cases(cc.ZERO_BATCH)
    assert cc.zero_runs(cc.ZERO_BATCH, 1, 8) == [(0, 2), (3, 2), (6, 2)] and cc.zero_runs(cc.ZERO_BATCH, 0, 2) == [(0, 2)]
    for cs in (zero[1:], cc.ragged_cases(), [cc.case(*cc.SMALL, s, "lege") for s in range(1, 17)],
               [cc.case(*cc.LARGE, s, "lege") for s in range(1, 5)]):
        assert {c["warm"]["status"] for c in cs} == both
        assert all(2 * dc.walk(c["D"], dc.CAP)["npiv"] < dc.CAP for c in cs)
        assert any(c["warm"]["npiv"] > 0 for c in cs)
    assert all(c["warm"]["npiv"] == 0 for c in zero if c["rows"].shape[0] == 0)


def test_the_threshold_shapes_are_on_both_sides():
    from lpsol_amd._lib import batch_lds_bytes
    m, ns = cc.THRESHOLD
    assert (m + 1) * (ns + m + 1) == 1891 <= cc.ONE_WAVE_ELEMS < (m + 3) * (ns + m + 3) == 2079
    m, ns = cc.LDS_EDGE
    assert batch_lds_bytes(m, ns + m) == 161720 <= 163840 < batch_lds_bytes(m + 2, ns + m + 2) == 166568
    for shape, workload, seeds in ((cc.THRESHOLD, "lege", range(1, 9)), (cc.LDS_EDGE, "le", (1, 2))):
        cs = [cc.case(*shape, s, workload) for s in seeds]
        assert all(c["warm"]["status"] in (_lib.OPTIMAL, _lib.INFEASIBLE) and 2 * c["warm"]["npiv"] < c["cap"] for c in cs)
        assert any(c["warm"]["npiv"] > 0 for c in cs)
        if workload == "lege":
            assert {c["warm"]["status"] for c in cs} == {_lib.OPTIMAL, _lib.INFEASIBLE}


def test_three_groups_of_rows_walk_to_both_verdicts():
    assert cc.GROUP_QS == (2 * cc.GROUP + 1, 3 * cc.GROUP)
    for shape in (cc.SMALL, cc.LARGE):
        for q in cc.GROUP_QS:
            cs = cc.group_cases(shape, q)
            assert cc.rows_lanes(*shape, q) == 3 * (sum(shape) + 1)
            assert {c["warm"]["status"] for c in cs} == {_lib.OPTIMAL, _lib.INFEASIBLE}
            assert all(2 * c["warm"]["npiv"] < c["cap"] and 2 * dc.walk(c["D"], dc.CAP)["npiv"] < dc.CAP for c in cs)
    assert sum(cc.LARGE) + 1 > 64                   # a group's lanes exceed one wave


def test_the_extreme_rows_make_infinities_nans_and_subnormals():
    T, basis, rows, sense = cc.odd_case()
    small = cc.case(*cc.SMALL, 3, "lege", 3)
    seen = []
    for how in cc.EXTREME_ROWS:
        for src, b, r, s in ((T, basis, rows, sense), (small["opt"], small["basis"], small["rows"], small["sense"])):
            D, _ = cc.extend(src, b, cc.extreme_rows(r, how), s)
            seen.append(D[src.shape[0]:, :src.shape[1]].ravel())
    got = np.concatenate(seen)
    assert np.isinf(got).any() and np.isnan(got).any() and ((got != 0) & (np.abs(got) < 2.2250738585072014e-308)).any()
