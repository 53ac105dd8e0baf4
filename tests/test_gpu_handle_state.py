"""What one lp_handle carries from call to call (include/lpgpu.h), on every
pivot path of the engine, bit for bit against tests/_handle_model.py (that is
oracle/lp_f64.c and, for the form checks, the host predicates of
lpsol_amd.Tableau).  No tolerance anywhere.

* Interleaved calls: a seeded sequence over the whole C-ABI -- runs (k = 0
  included), capped and whole solves, both findPivot rules, explicit, checked
  and refused pivots, the column scans, row windows, lp_set_tol, lp_set_block --
  replayed on the per-pivot kernels, k_sel on one XCD, k_sel as XCD shards,
  k_group, an in-process shard group and, in a child process, out-of-place
  sweeps.  test_handle_model_cpu.py asserts what the sequences contain.
* Row windows through raw lp_upload_rows / lp_download_rows: a host leading
  dimension above n + 1, empty and edge windows, refused windows (which must
  leave the device untouched, on a shard too), and a window that changes a
  cost, a b_i or an a_ij between two calls: the row-0 / column-0 mirrors
  (lp_handle::eager_ok, k_load_eager) must follow.

Reference: lpsol/tableau.py:82-108,128-158 (getters / setters the windows
replace), :295-308 (pivot); lpsol/simplex.py:199-360 (pivot, findPivot*)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _handle_model as hm
from lpsol_amd import _lib
from lpsol_amd import generators as gen

pytestmark = pytest.mark.gpu

STD, MIN = _lib.RULE_STANDARD, _lib.RULE_MIN_INDEX


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"


def _engine(spec):
    m, n = gen.shape(*spec[:3])
    return _lib.Engine(m, n)


# ------------------------------------------------------------ interleaved calls
# The selection kernel a run takes depends on the pivots per sweep in force
# (lp_set_block is part of the sequences): replay() reports every run's, and
# each leg asserts that the path it is named after was taken -- by every run
# where the engine offers no other, else by those at the depths that take it.
@pytest.mark.parametrize("spec", [hm.SMALL, hm.MID], ids=hm.seq_id)
@pytest.mark.parametrize("path", ["kernels", "k_sel"])
def test_interleaved_calls_one_device(spec, path, monkeypatch):
    if path == "kernels":
        monkeypatch.setenv("LPGPU_SELECT", "kernels")
    e = _engine(spec)
    try:
        took = hm.replay(hm.sequence(*spec), [e])
    finally:
        e.close()
    assert len(took) >= 5
    for t in took:
        if path == "kernels":
            assert t["path"] == _lib.PATH_KERNELS and t["kernel"] == "none", t
        else:
            assert t["path"] == _lib.PATH_PERSISTENT and t["kernel"] == "k_sel" and t["xcd_shards"] == 0, t


def test_interleaved_calls_xcd_shards():
    """6000 rows: k_sel as one row shard per XCD at more than 32 pivots per
    sweep (select.hip sel_geom), k_group below"""
    e = _engine(hm.TALL)
    try:
        took = hm.replay(hm.sequence(*hm.TALL), [e])
    finally:
        e.close()
    deep = [t for t in took if t["block"] > 32]
    assert len(deep) >= 3 and len(deep) < len(took), took
    for t in took:
        assert t["path"] == _lib.PATH_PERSISTENT, t
        if t["block"] > 32:
            assert t["kernel"] == "k_sel" and t["xcd_shards"] == 8 and t["xcd_shards_engaged"], t
        else:
            assert t["kernel"] == "k_group", t


def test_interleaved_calls_k_group(monkeypatch):
    """the same tall tableau with the XCD shards off: k_group at the depth
    that takes the shards otherwise.  A prefix of the sequence, the tableau
    compared after every fifth call that can change it"""
    monkeypatch.setenv("LPGPU_SEL_XS", "0")
    e = _engine(hm.TALL)
    try:
        took = hm.replay(hm.k_group_ops(), [e], every=5)
    finally:
        e.close()
    assert took
    for t in took:
        assert t["block"] > 32 and t["path"] == _lib.PATH_PERSISTENT and t["kernel"] == "k_group", t


@pytest.mark.parametrize("peer", ["1", "0"], ids=["peer", "collective"])
def test_interleaved_calls_shard_group(peer, monkeypatch):
    """three in-process row shards: each window goes to the members that hold
    its rows (row 0 to all of them), every other call to member 0"""
    monkeypatch.setenv("LPGPU_PEER", peer)
    m, n = gen.shape(*hm.GROUP[:3])
    grp = _lib.create_group(m, n, 3)
    try:
        took = hm.replay(hm.sequence(*hm.GROUP), grp)
    finally:
        for g in reversed(grp):
            g.close()
    assert len(took) >= 5
    for t in took:
        assert t["path"] == (_lib.PATH_PEER if peer == "1" else _lib.PATH_COLLECTIVE), t


def test_interleaved_calls_out_of_place_worker():
    """LPGPU_SWEEP_OOP is read once per process: a child process"""
    worker = os.path.join(os.path.dirname(__file__), "_handle_state_worker.py")
    env = dict(os.environ, LPGPU_SWEEP_OOP="1")
    run = subprocess.run([sys.executable, "-u", worker], env=env, capture_output=True, text=True, timeout=110)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr


# ------------------------------------------------------------------ row windows
SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
WINDOW_SHAPES = [("mixed", 40, 30, 5), ("tall", 600, 40, 6)]
_shape_id = "{0}_{1}x{2}".format


def _up(e, row0, nrows, buf, ldh):
    return e.lib.lp_upload_rows(e.h, row0, nrows, _lib._ptr(buf), ldh)


def _down(e, row0, nrows, buf, ldh):
    return e.lib.lp_download_rows(e.h, row0, nrows, _lib._ptr(buf), ldh)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _windows(m):
    return [(0, 0), (3, 0), (0, 1), (m, 1), (1, m)]       # empty, row 0, the last row, [1, m + 1)


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: _shape_id(*s))
def test_host_leading_dimension_above_n_plus_1(shape):
    """ldh = n + 1 + 5: a download leaves the 5 pad cells of every host row
    alone, an upload does not read them"""
    T = gen.tableau(*shape)
    F = gen.tableau(*shape[:3], shape[3] + 100)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    ldh = n + 1 + 5
    e = _lib.Engine(m, n)
    try:
        e.upload(T)
        e.run(STD, 3)
        M = hm.HandleModel(T)
        M.run(STD, 3)
        for row0, nrows in _windows(m):
            buf = np.full((max(nrows, 1), ldh), SENTINEL)
            assert _down(e, row0, nrows, buf, ldh) == _lib.PIVOTED
            want = np.full((max(nrows, 1), ldh), SENTINEL)
            want[:nrows, :n + 1] = M.rows(row0, nrows)
            assert np.array_equal(_u64(buf), _u64(want)), (row0, nrows)
        for row0, nrows in _windows(m):
            buf = np.full((max(nrows, 1), ldh), np.nan)
            buf[:nrows, :n + 1] = F[row0:row0 + nrows]
            assert _up(e, row0, nrows, buf, ldh) == _lib.PIVOTED
            assert M.put_rows(row0, buf[:nrows]) == hm.PIVOTED
            assert hm.bits(e.download(), M.T), (row0, nrows)
            # and the calls after it see the patched rows
            assert e.find_all() == M.find_all(), (row0, nrows)
            assert hm._norm(e.find(MIN, False)) == hm._norm(M.find(MIN, False)), (row0, nrows)
        assert e.exchange_path()[1] == 0
    finally:
        e.close()


def _refused(e, row0, nrows, ldh):
    """both transfers answer LP_BAD_ARG and the host buffer is not written"""
    n = e.n
    src = np.full((max(nrows, 1) + 2, max(ldh, n + 1)), 7.0)
    assert _up(e, row0, nrows, src, ldh) == _lib.BAD_ARG, (row0, nrows, ldh)
    dst = np.full((max(nrows, 1) + 2, max(ldh, n + 1)), SENTINEL)
    assert _down(e, row0, nrows, dst, ldh) == _lib.BAD_ARG, (row0, nrows, ldh)
    assert (_u64(dst) == _u64(SENTINEL)).all(), (row0, nrows, ldh)


def _member_state(grp):
    return [np.concatenate([g.rows(0, 1), g.rows(1 + g.row_begin, g.row_count)]) for g in grp]


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: _shape_id(*s))
def test_refused_window_leaves_the_device_untouched(shape):
    T = gen.tableau(*shape)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    e = _lib.Engine(m, n)
    try:
        e.upload(T)
        e.run(STD, 2)
        before = e.download()
        for row0, nrows, ldh in [(-1, 1, n + 1), (-1, 0, n + 1), (m, 2, n + 1), (0, m + 2, n + 1), (m + 1, 1, n + 1),
                                 (0, 1, n), (1, 2, n), (0, -1, n + 1)]:
            assert hm.window_status(m, n, row0, nrows, ldh) == hm.BAD_ARG
            _refused(e, row0, nrows, ldh)
            assert hm.bits(e.download(), before), (row0, nrows, ldh)
        # the handle still answers as the model
        M = hm.HandleModel(T)
        M.run(STD, 2)
        assert hm.bits(before, M.T)
        assert hm._norm(e.find(STD, True)) == hm._norm(M.find(STD, True)) and hm.bits(e.download(), M.T)
    finally:
        e.close()


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: _shape_id(*s))
def test_refused_window_on_a_shard(shape):
    """members 1 and 2 of three shards: a window that starts in rows the rank
    holds (row 0) or does not hold and runs into the other kind is refused as
    a whole -- no row of it is copied, in either direction"""
    T = gen.tableau(*shape)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    grp = _lib.create_group(m, n, 3)
    try:
        for g in grp:
            g.upload(T)
        grp[0].run(STD, 2)
        before = _member_state(grp)
        for g in grp[1:]:
            rb, rc = g.row_begin, g.row_count
            for row0, nrows in [(0, 2), (1 + rb - 1, 2), (1 + rb + rc - 1, 2) if g is grp[1] else (0, 3)]:
                assert hm.window_status(m, n, row0, nrows, n + 1, rb, rc) == hm.BAD_ARG
                _refused(g, row0, nrows, n + 1)
                for a, b in zip(_member_state(grp), before):
                    assert hm.bits(a, b), (g.row_begin, row0, nrows)
        M = hm.HandleModel(T)
        M.run(STD, 2)
        assert hm.bits(hm.group_state(grp), M.T)
        assert hm._norm(grp[0].find(STD, True)) == hm._norm(M.find(STD, True))
        assert hm.bits(hm.group_state(grp), M.T)
    finally:
        for g in reversed(grp):
            g.close()


def _changes(M):
    """-> [(name, row0, rows)]: windows of the model's current tableau with
    (a) one cost changed so that the entering column changes, (b) b of the
    leaving row so that the leaving row changes, (c) one a_ij (the pivot cell,
    negated: the row leaves the ratio test).  Asserted on the model here."""
    r, c = M.o.find(STD)
    out = []
    row = M.T[:1].copy()
    j = next(j for j in range(M.n) if j != c)
    row[0, 1 + j] = row[0, 1:].min() - 1.0
    out.append(("cost", 0, row))
    row = M.T[1 + r:2 + r].copy()
    row[0, 0] = row[0, 0] * 1024.0 + 64.0
    out.append(("b", 1 + r, row))
    row = M.T[1 + r:2 + r].copy()
    row[0, 1 + c] = -row[0, 1 + c]
    out.append(("a", 1 + r, row))
    for name, row0, rows in out:
        P = hm.HandleModel(M.T, M.tol)
        P.put_rows(row0, rows)
        w = P.o.find(STD)
        assert isinstance(w, tuple) and (w[1] != c if name == "cost" else w[0] != r), name
    return out


def _bad_pair(M):
    S = M.find_all()
    c = S[0][1]
    r = next(i for i in range(M.m) if M.T[1 + i, 1 + c] > 1e-9 and (i, c) not in S)
    return (r, c), S[0]


PROBES = ["find_std", "find_min", "find_all", "max_increase", "form_checks", "checked", "run0_find", "run1"]


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: _shape_id(*s))
@pytest.mark.parametrize("path", ["kernels", "persistent"])
def test_window_between_calls_reaches_the_next_call(shape, path, monkeypatch):
    """state S (three pivots in, mirrors loaded by the calls before); a window
    upload that changes a cost / a b_i / an a_ij; then ONE call, which must
    answer as the model with the same rows patched -- for every kind of call
    that reads the mirrors or the tableau"""
    if path == "kernels":
        monkeypatch.setenv("LPGPU_SELECT", "kernels")
    T = gen.tableau(*shape)
    m, n = T.shape[0] - 1, T.shape[1] - 1
    S = hm.HandleModel(T)
    S.run(STD, 3)
    changes = _changes(S)
    e = _lib.Engine(m, n)
    try:
        e.upload(T)
        assert e.run(STD, 3)[1] == 3
        assert e.exchange_path()[0] == (_lib.PATH_KERNELS if path == "kernels" else _lib.PATH_PERSISTENT)
        for name, row0, rows in changes:
            for probe in PROBES:
                where = (name, probe)
                # back to S with its mirrors loaded
                e.upload(S.T)
                assert hm._norm(e.find(STD, False)) == hm._norm(S.o.find(STD)), where
                assert e.find_max_increase(False) == S.o.find_max_increase(), where
                M = hm.HandleModel(S.T, S.tol)
                assert _up(e, row0, 1, np.ascontiguousarray(rows), n + 1) == _lib.PIVOTED
                assert M.put_rows(row0, rows) == hm.PIVOTED
                if probe == "find_std":
                    assert hm._norm(e.find(STD, False)) == hm._norm(M.find(STD, False)), where
                elif probe == "find_min":
                    assert hm._norm(e.find(MIN, False)) == hm._norm(M.find(MIN, False)), where
                elif probe == "find_all":
                    assert e.find_all() == M.find_all(), where
                elif probe == "max_increase":
                    assert hm._norm(e.find_max_increase(False)) == hm._norm(M.find_max_increase(False)), where
                elif probe == "form_checks":
                    assert e.form_checks() == M.form_checks(), where
                elif probe == "checked":
                    bad, ok = _bad_pair(M)
                    assert e.pivot_checked(*bad) == M.pivot_checked(*bad) == _lib.BAD_PIVOT, where
                    assert hm.bits(e.download(), M.T), where
                    e.upload(S.T)                      # mirrors of S again, then the window, then the accepted pivot
                    e.find(STD, False)
                    _up(e, row0, 1, np.ascontiguousarray(rows), n + 1)
                    assert e.pivot_checked(*ok) == M.pivot_checked(*ok) == _lib.PIVOTED, where
                elif probe == "run0_find":
                    assert e.run(STD, 0) == (_lib.PIVOTED, 0), where
                    assert hm._norm(e.find(STD, False)) == hm._norm(M.find(STD, False)), where
                else:
                    st, done, log = M.run(STD, 1)
                    assert e.run(STD, 1) == (st, done) and e.log().tolist() == log, where
                assert hm.bits(e.download(), M.T), where
        assert e.exchange_path()[1] == 0
    finally:
        e.close()
