"""Child process of test_gpu_handle_state.py::test_interleaved_calls_out_of_place_worker:
the engine with LPGPU_SWEEP_OOP=1 (read once per process).  Every sweep of a
run reads one tableau buffer and writes the other, so the handle's current
tableau alternates between two allocations; row windows, scans and explicit
pivots must land on whichever holds it.

* First, runs of 3, 17, 70 and 1 pivots at depth 64 -- one sweep each, two for
  the 70: the current buffer is the second, the first, the first and the second
  one after them (1, 2, 4, 5 flips).  After each: a window upload, every scan,
  both findPivot rules, a window download, lp_run(rule, 0), a checked pivot.
* Then the whole interleaved sequence of mixed 300x191 (tests/_handle_model.py).
Everything against the model, bit for bit.  Prints one line per step and
"ALL OK" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "linear-program-solver_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _handle_model as hm  # noqa: E402
from lpsol_amd import _lib, generators as gen  # noqa: E402

STD, MIN = _lib.RULE_STANDARD, _lib.RULE_MIN_INDEX


def check(name, ok):
    print(name, "ok" if ok else "MISMATCH", flush=True)
    if not ok:
        sys.exit(1)


def after_flips(e, M, F, flips, row0):
    w = f"after {flips} flips:"
    rows = F[row0:row0 + 3]
    e.put_rows(row0, rows)
    M.put_rows(row0, rows)
    check(f"{w} find_all", e.find_all() == M.find_all())
    check(f"{w} form_checks", e.form_checks() == M.form_checks())
    check(f"{w} max increase", hm._norm(e.find_max_increase(False)) == hm._norm(M.find_max_increase(False)))
    check(f"{w} findPivot", all(hm._norm(e.find(r, False)) == hm._norm(M.find(r, False)) for r in (STD, MIN)))
    check(f"{w} window download", hm.bits(e.rows(row0, 3), M.rows(row0, 3)))
    check(f"{w} run 0", e.run(MIN, 0) == (hm.PIVOTED, 0))
    S = M.find_all()
    check(f"{w} checked pivot", e.pivot_checked(*S[-1]) == M.pivot_checked(*S[-1]) == hm.PIVOTED)
    check(f"{w} tableau", hm.bits(e.download(), M.T))


def main():
    kind, m, ns, seed, _ = hm.MID
    T = gen.tableau(kind, m, ns, seed)
    F = gen.tableau(kind, m, ns, seed + 500)
    e = _lib.Engine(T.shape[0] - 1, T.shape[1] - 1)
    check("two sweep buffers", e.sweep_buffers() == 2)
    e.upload(T)
    e.set_block(64)
    M = hm.HandleModel(T)
    flips = 0
    for k, row0 in ((3, 0), (17, m - 2), (70, 5), (1, 0)):
        st, done, log = M.run(STD, k)
        check(f"run {k}", e.run(STD, k) == (st, done) and e.log().tolist() == log and done == k)
        if flips == 0:
            check("persistent path", e.exchange_path()[0] == _lib.PATH_PERSISTENT)
        flips += (k + 63) // 64
        after_flips(e, M, F, flips, row0)
    hm.replay(hm.sequence(*hm.MID), [e])
    check("interleaved sequence", True)
    check("two sweep buffers", e.sweep_buffers() == 2)
    check("no fallback", e.exchange_path()[1] == 0)
    e.close()


if __name__ == "__main__":
    assert os.environ.get("LPGPU_SWEEP_OOP") == "1"
    main()
    print("ALL OK")
