"""GPU: bench.py's restart of a finite LP on a real engine (run_steps,
restart): an engine that has reached its optimum gets the initial tableau
again through put_rows and must repeat itself -- the same pivots in the same
order and, pivot count for pivot count, the same tableau bit for bit.  Small
LPs that end within tens of pivots, on the per-pivot kernels (block 8) and at
the engine's automatic depth; event timing on, as in the timed steps, so the
launches that exit at once after the optimum are counted from the engine's
own launch counts."""
import numpy as np
import pytest

import bench
from lpsol_amd import _lib
from lpsol_amd import generators as gen

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,m,ns,seed,block", [("mixed", 24, 32, 11, 8), ("pos", 96, 64, 2, 0),
                                                  ("mixed", 200, 150, 5, 16)])
def test_restart_repeats_the_lp(kind, m, ns, seed, block):
    T = gen.tableau(kind, m, ns, seed)
    kept = [(0, T[:1]), (1, T[1:])]

    # the LP once, to its optimum: its length, pivot log and final tableau
    ref = _lib.Engine(m, T.shape[1] - 1)
    ref.set_block(block)
    B = ref.get_block()
    ref.upload(T)
    st, length = ref.run(_lib.RULE_STANDARD, 1 << 20)
    assert st == _lib.OPTIMAL and length >= 2
    ref_log, ref_end = ref.log()[:length].copy(), ref.download()

    # two passes and a part of a third through run_steps, in two calls
    e = _lib.Engine(m, T.shape[1] - 1)
    e.set_block(block)
    e.upload(T)
    part = max(1, length // 3)
    steps = -(-(2 * length + part) // B)
    state = {}
    e.profile(True, every=1)
    state["every"] = 1
    bench.run_steps(e, 1, B, kept, state=state)
    bench.run_steps(e, steps - 1, B, kept, state=state)
    sweeps, selections = e.update_time()[1], e.select_time()[1]
    e.profile(False)
    total = steps * B
    assert state["length"] == length
    assert state["restarts"] == total // length - (1 if total % length == 0 else 0)
    tail = total - state["restarts"] * length
    assert state["in_pass"] == tail
    # the last call's pivots are the LP's own first pivots again
    log = e.log()
    assert 1 <= len(log) <= tail and np.array_equal(log, ref_log[tail - len(log):tail])
    # and the tableau after them is the one a fresh engine has after as many
    f = _lib.Engine(m, T.shape[1] - 1)
    f.set_block(block)
    f.upload(T)
    assert f.run(_lib.RULE_STANDARD, tail)[1] == tail
    assert np.array_equal(e.download(), f.download())
    if tail == length:
        assert np.array_equal(e.download(), ref_end)
    # the launches beyond those that worked are the ones counted as idle
    assert 0 <= state["idle_sweeps"] < sweeps and 0 <= state["idle_selections"] < selections
    for x in (ref, e, f):
        x.close()
