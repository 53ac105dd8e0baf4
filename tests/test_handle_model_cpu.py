"""The call sequences of tests/_handle_model.py on the model alone (no GPU):
conditions on the inputs of test_gpu_handle_state.py, checked for exactly the
sequences it replays (_handle_model.SEQUENCES).  A sequence that misses one of
them would let the GPU test pass without running what it is there for."""
import numpy as np
import pytest

import _handle_model as hm
from oracle.f64 import F64Tableau


@pytest.mark.parametrize("spec", hm.SEQUENCES, ids=hm.seq_id)
def test_sequence_covers_the_abi(spec):
    ops = hm.sequence(*spec)
    kinds = [o["kind"] for o in ops]
    assert not [i for i, o in enumerate(ops) if o.get("skipped")]
    for k in hm.KINDS:
        assert kinds.count(k) >= 2, k
    rets = [(o["kind"], o["ret"]) for o in ops]
    assert ("checked_bad", hm.BAD_PIVOT) in rets
    assert ("pivot_zero", hm.ZERO_PIVOT) in rets
    assert ("checked_ok", hm.PIVOTED) in rets
    status = [o["ret"][0] for o in ops if o["kind"] in ("run", "solve")]
    assert hm.CAP_REACHED in status and hm.OPTIMAL in status
    # every k of run, cap of solve, depth of set_block; both rules and do_pivot of find
    assert {o["args"][1] for o in ops if o["kind"] == "run"} == set(hm.RUN_K)
    assert {o["args"][0] for o in ops if o["kind"] == "solve"} == set(hm.SOLVE_CAPS)
    assert {o["args"][0] for o in ops if o["kind"] == "set_block"} == set(hm.BLOCKS)
    assert {o["args"] for o in ops if o["kind"] == "find"} >= {(r, d) for r in (0, 1) for d in (False, True)}
    # runs that enqueue pivots at deep sweeps (64, 48, auto) and at shallow ones (1, 7):
    # a tall tableau takes another selection kernel at 32 and below (select.hip sel_geom)
    depth, deep, shallow = 0, 0, 0
    for o in ops:
        if o["kind"] == "set_block":
            depth = o["args"][0]
        elif o["kind"] in ("run", "solve") and o["ret"][1] > 0:
            deep += depth in (0, 48, 64)
            shallow += depth in (1, 7)
    assert deep >= 3 and shallow >= 1
    pairs = list(zip(ops, ops[1:]))
    # lp_run(h, rule, 0) directly after a window, after a whole upload, and a
    # whole upload after a solve that ended optimal (the old Ctl is LP_OPTIMAL)
    run0 = [a["kind"] for a, b in pairs if b["kind"] == "run" and b["args"][1] == 0]
    assert set(run0) & set(hm.PUTS) and "upload" in run0
    assert all(o["ret"] == (hm.PIVOTED, 0) for o in ops if o["kind"] == "run" and o["args"][1] == 0)
    assert any(a["kind"] == "solve" and a["ret"][0] == hm.OPTIMAL and b["kind"] == "upload" for a, b in pairs)
    assert any(a["kind"] == "put_row0" and b["kind"] in hm.SCANS for a, b in pairs)
    # the windows change what the mirrors hold: a cost, and a b_i
    prev = ops[0]["T"]
    row0_changed = col0_changed = False
    for o in ops[1:]:
        if o["kind"] in hm.PUTS:
            r0, rows = o["args"]
            row0_changed |= r0 == 0 and not hm.bits(prev[0], o["T"][0])
            col0_changed |= not hm.bits(prev[:, 0], o["T"][:, 0])
        if o["T"] is not None:
            prev = o["T"]
            assert np.isfinite(prev).all()             # the engine's domain (include/lpgpu.h)
    assert row0_changed and col0_changed


def test_k_group_prefix_runs_pivots():
    """the k_group leg replays a prefix of the tall sequence: it still holds a
    window, a scan, a run and an explicit pivot"""
    ops = hm.k_group_ops()
    assert len(ops) >= 20 and "set_block" not in {o["kind"] for o in ops}
    kinds = {o["kind"] for o in ops}
    assert kinds & set(hm.PUTS) and kinds & set(hm.SCANS) and "run" in kinds
    assert kinds & {"pivot", "checked_ok", "find"}
    assert any(o["kind"] in ("run", "solve") and o["ret"][1] > 0 for o in ops)


def test_model_against_oracle_calls():
    """the model's own plumbing: each method is the oracle call it names"""
    spec = hm.SEQUENCES[0]
    T = hm.sequence(*spec)[0]["T"]
    M, o = hm.HandleModel(T), F64Tableau(T)
    assert M.find_all() == o.find_all()
    r, c = o.find(0)
    assert M.find(0, True) == (r, c)
    o.pivot(r, c)
    assert hm.bits(M.T, o.T)
    S = M.find_all()
    bad = next((i, S[0][1]) for i in range(M.m) if (i, S[0][1]) not in S and M.T[1 + i, 1 + S[0][1]] != 0.0)
    before = M.T.copy()
    assert M.pivot_checked(*bad) == hm.BAD_PIVOT and hm.bits(M.T, before)
    assert M.pivot_checked(*S[0]) == hm.PIVOTED
    o.pivot(*S[0])
    assert hm.bits(M.T, o.T)
    assert M.run(0, 0) == (hm.PIVOTED, 0, [])
    assert M.solve(0)[:3] == (hm.CAP_REACHED, 0, 0)


@pytest.mark.parametrize("row0,nrows,ldh,rb,rc,want", [
    (0, 0, 31, 0, None, hm.PIVOTED), (0, 1, 31, 0, None, hm.PIVOTED), (20, 1, 31, 0, None, hm.PIVOTED),
    (1, 20, 36, 0, None, hm.PIVOTED), (-1, 1, 31, 0, None, hm.BAD_ARG), (20, 2, 31, 0, None, hm.BAD_ARG),
    (0, 1, 30, 0, None, hm.BAD_ARG), (0, 2, 31, 6, 7, hm.BAD_ARG), (6, 2, 31, 6, 7, hm.BAD_ARG),
    (7, 7, 31, 6, 7, hm.PIVOTED), (0, 1, 31, 6, 7, hm.PIVOTED), (13, 2, 31, 6, 7, hm.BAD_ARG)])
def test_window_status(row0, nrows, ldh, rb, rc, want):
    assert hm.window_status(20, 30, row0, nrows, ldh, rb, rc) == want
    M = hm.HandleModel(np.zeros((21, 31)))
    rows = np.ones((max(nrows, 0), ldh))
    if nrows >= 0:
        assert M.put_rows(row0, rows, rb, rc) == want
        assert (M.T != 0.0).any() == (want == hm.PIVOTED and nrows > 0)
