#!/usr/bin/env python3
"""Problem-form upload against the upload of host-assembled tableaux: the
tableaux' slack blocks laid out on the device (lp_problem_upload, k_assemble)
against shipping them over PCIe, and duals() against download() + the host
formula.

Five seeded workloads: mixed 8x10 x 16384, 40x40 x 4096 and 64x64 x 1024
(generators.mixed_stack, seeds 1..B) under place="lds", mixed 100x100 x 2048
under place="auto" (device-placed), and phase1_lp("ge", 24, 24) x 4096 for the
two-phase path.  For each, in one process, 5 timed repetitions after a warm-up
(host clock, every call synchronous), the legs alternating and taking turns at
going first:

  (a)  on one reused engine: upload_problems + derive_basis (nothing, on the
       two-phase path) + solve + solution()
  (b)  on the same engine: upload of tableaux the host assembled beforehand +
       the same remaining calls -- what the library offered before
  (b') (b) with assemble_tableaux on the host inside the timed region
  (c)  the whole call solve_problems(c, A, b, sense) against assemble_tableaux
       + solve_batch / solve_lp_batch(result="solution")
  the upload step of (a) and of (b) alone, and duals() against download() +
  problem_duals on the host

Before anything is timed the new path is checked against the old one: equal
status and pivot counts, and the bits of objective and x.  The condition: at
every shape the slowest of (a)'s five is not above the fastest of (b)'s five.

Prints one JSON line (profiles/r15/problem_bench.json).  Run it once, under a
time limit:  timeout 900 python scripts/problem_bench.py
With --trace it only runs each workload's (a) leg three times, for a kernel
trace of k_assemble taken in a run of its own.
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

from lpsol_amd import _lib, assemble_tableaux, problem_duals, solve_batch, solve_lp_batch, solve_problems  # noqa: E402
from lpsol_amd import generators as gen          # noqa: E402

# kind, m, ns, LPs, place
WORKLOADS = [("mixed", 8, 10, 16384, "lds"), ("mixed", 40, 40, 4096, "lds"), ("mixed", 64, 64, 1024, "lds"),
             ("mixed", 100, 100, 2048, "auto"), ("ge", 24, 24, 4096, "lds")]
CAP = 1 << 16
REPS = 5


def med(xs):
    return statistics.median(xs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def inputs(kind, m, ns, B):
    """-> (tableaux, senses, ns)"""
    if kind == "mixed":
        return gen.mixed_stack(m, ns, range(1, B + 1)), np.zeros(m, dtype=np.int8), ns
    T = np.stack([gen.phase1_lp("ge", m, ns, s) for s in range(1, B + 1)])
    return T, np.array([_lib.SENSE_GE] * m + [_lib.SENSE_LE], dtype=np.int8), ns


def bench(kind, m, ns, B, place, trace=False):
    T, sense, ns = inputs(kind, m, ns, B)
    P = np.ascontiguousarray(T[:, :, :ns + 1])
    c, A, b = T[:, 0, 1:ns + 1], T[:, 1:, 1:ns + 1], T[:, 1:, 0]
    Th = assemble_tableaux(P, sense)
    assert np.array_equal(Th, T)
    rows, n = T.shape[1] - 1, T.shape[2] - 1
    plain = kind == "mixed"
    placed = place != "lds"
    old_call = solve_batch if plain else solve_lp_batch

    eng = _lib.BatchEngine(B, rows, n, place=place)
    eng.set_senses(sense)

    def rest():
        if plain:
            eng.derive_basis()
            out = eng.solve(CAP)
        else:
            out = (eng.solve_lp_placed if placed else eng.solve_lp)(CAP)
        return out, eng.solution()

    def leg_a():
        eng.upload_problems(P)
        return rest()

    def leg_b():
        eng.upload(Th)
        return rest()

    def leg_b2():
        eng.upload(assemble_tableaux(P, sense))
        return rest()

    if trace:
        for _ in range(3):
            leg_a()
        eng.close()
        return {"shape": f"{kind} {m}x{ns}", "lps": B}

    # the check, before anything is timed
    (sa, xa), (sb, xb) = leg_a(), leg_b()
    assert all(same_bits(p, q) for p, q in zip(sa, sb)), "status or pivot counts differ"
    assert same_bits(xa[0], xb[0]) and same_bits(xa[1], xb[1]), "x or objective bits differ"
    optimal = int(np.count_nonzero(sa[0] == _lib.OPTIMAL))
    new = solve_problems(c, A, b, sense, max_pivots=CAP, place=place)
    old = old_call(Th, max_pivots=CAP, place=place, result="solution")
    assert new.path == ("plain" if plain else "twophase")
    assert same_bits(new.status_code, old.status_code) and same_bits(new.npiv, old.npiv)
    assert same_bits(new.objective, old.objective) and same_bits(new.x, old.x[:, :ns])
    new._engine.close()
    old._engine.close()
    del new, old

    def whole_new():
        dt, res = clock(lambda: solve_problems(c, A, b, sense, max_pivots=CAP, place=place))
        res._engine.close()
        return dt

    def whole_old():
        dt, res = clock(lambda: old_call(assemble_tableaux(P, sense), max_pivots=CAP, place=place, result="solution"))
        res._engine.close()
        return dt

    def host_duals():
        out = eng.download()
        return np.stack([problem_duals(t, sense, ns) for t in out])

    keys = ("a", "b", "b2", "c_new", "c_old", "up_a", "up_b", "duals", "host_duals")
    t = {k: [] for k in keys}
    for rep in range(REPS + 1):                 # rep 0 is the warm-up
        legs = [("a", leg_a), ("b", leg_b), ("b2", leg_b2)]
        legs = legs[rep % 3:] + legs[:rep % 3]  # they take turns at going first
        got = {k: clock(fn)[0] for k, fn in legs}
        pair = [("c_new", whole_new), ("c_old", whole_old)]
        for k, fn in (pair if rep % 2 else pair[::-1]):
            got[k] = fn()
        ups = [("up_a", lambda: eng.upload_problems(P)), ("up_b", lambda: eng.upload(Th))]
        for k, fn in (ups if rep % 2 else ups[::-1]):
            got[k] = clock(fn)[0]
        rest()
        dd = [("duals", eng.duals), ("host_duals", host_duals)]
        for k, fn in (dd if rep % 2 else dd[::-1]):
            got[k] = clock(fn)[0]
        if rep:
            for k in keys:
                t[k].append(got[k])
    assert same_bits(eng.duals(), host_duals())
    eng.close()
    return {
        "shape": f"{kind} {m}x{ns}", "m": rows, "n": n, "ns": ns, "lps": B, "place": place,
        "path": "plain" if plain else "twophase", "optimal_lps": optimal,
        "problem_s": med(t["a"]), "problem_s_runs": t["a"],
        "tableau_s": med(t["b"]), "tableau_s_runs": t["b"],
        "tableau_with_host_assembly_s": med(t["b2"]), "tableau_with_host_assembly_s_runs": t["b2"],
        "tableau_over_problem": med(t["b"]) / med(t["a"]),
        "slowest_problem_over_fastest_tableau": max(t["a"]) / min(t["b"]),
        "condition_met": max(t["a"]) <= min(t["b"]),
        "solve_problems_call_s": med(t["c_new"]), "solve_problems_call_s_runs": t["c_new"],
        "old_call_s": med(t["c_old"]), "old_call_s_runs": t["c_old"],
        "upload_problems_s": med(t["up_a"]), "upload_problems_s_runs": t["up_a"],
        "upload_tableaux_s": med(t["up_b"]), "upload_tableaux_s_runs": t["up_b"],
        "duals_s": med(t["duals"]), "duals_s_runs": t["duals"],
        "download_and_host_duals_s": med(t["host_duals"]), "download_and_host_duals_s_runs": t["host_duals"],
        "bytes_in_problem": int(P.nbytes), "bytes_in_tableaux": int(Th.nbytes),
        "bytes_ratio": P.nbytes / Th.nbytes,
        "bit_identical_to_tableau_path": True,
    }


def main():
    if _lib.device_count() < 1:
        raise SystemExit("problem_bench.py needs a GPU")
    trace = "--trace" in sys.argv[1:]
    out = [bench(*w, trace=trace) for w in WORKLOADS]
    if trace:
        print(json.dumps({"bench": "problem_bench", "trace_only": True, "workloads": out}))
        return 0
    ok = all(r["condition_met"] for r in out)
    print(json.dumps({"bench": "problem_bench", "reps": REPS, "workloads": out,
                      "problem_leg_never_slower_than_tableau_leg": ok}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
