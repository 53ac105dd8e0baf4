"""bench.py's accounting, checked without a GPU: the algorithmic byte counts
behind `roofline.achieved`, the strong-scaling row split,
the per-launch figures of a timed run, the traffic file's stamp and the
dense CPU baseline's pivot."""
import json
import os

import numpy as np
import pytest

import bench
from lpsol_amd import generators as gen
from oracle import exact


def test_pivot_bytes_matches_survey():
    # B = 8 * [2 (m+1)(n+1) + (n+1) + 2 (m+1)]; cfg3: 537,198,632 B
    assert bench.pivot_bytes(4096, 8192) == 537_198_632
    assert bench.pivot_bytes(512, 1024) == 8_429_608
    assert bench.pivot_bytes(32768, 8192) == 4_296_212_520


def test_sweep_bytes_cfg3():
    # one 32-pivot sweep of cfg3: rows read + written, P and M read once
    rows, n = 4097, 8192
    assert bench.sweep_bytes(rows, n, 32) == 8 * (2 * rows * (n + 1) + 32 * (n + 1) + 32 * rows)
    assert bench.sweep_bytes(rows, n, 32) == 540_213_776


@pytest.mark.parametrize("name", ["cfg4", "cfg3"])
@pytest.mark.parametrize("nranks", [1, 2, 4, 8])
def test_strong_scaling_rows_partition(name, nranks):
    """the same tableau at every N, rows split like lp_create_sharded"""
    spans = [bench.workload(name, nranks, r) for r in range(nranks)]
    kind, m, ns, n, _, _ = spans[0]
    assert (m, n) == ((32768, 8192) if name == "cfg4" else (4096, 8192))
    assert [s[4] for s in spans] == [m * r // nranks for r in range(nranks)]
    assert spans[0][4] == 0 and spans[-1][5] == m
    for a, b in zip(spans, spans[1:]):
        assert a[5] == b[4]                                  # contiguous, no overlap


@pytest.mark.parametrize("steps,block", [(20, 32), (1, 32), (128, 16)])
def test_accounting_per_launch(steps, block):
    """every launch of a timed run carries exactly `block` pivots (one step =
    one group), so per-launch bytes and per-pivot selection time follow"""
    a = bench.accounting(steps, block, elapsed=0.5, sweep_avg_ms=0.1, sel_avg_ms=0.2,
                         local_rows=4097, n=8192)
    assert a["pivots"] == steps * block
    assert a["pivots_per_s"] == pytest.approx(steps * block / 0.5)
    assert a["ms_per_step"] == pytest.approx(500.0 / steps)
    assert a["sweep_bytes_per_launch"] == bench.sweep_bytes(4097, 8192, block)
    assert a["achieved_GBps"] == pytest.approx(bench.sweep_bytes(4097, 8192, block) / 1e-4 / 1e9)
    assert a["selection_us_per_pivot"] == pytest.approx(200.0 / block)
    assert a["sweep_time_share"] == pytest.approx(0.1 * steps / 500.0)


def test_traffic_needs_this_build(tmp_path):
    """roofline.traffic is reported only for builds of the sources, workload and
    block the PMC passes measured (scripts/hbm_traffic.py stamps them)"""
    p = tmp_path / "t.json"
    d = {"kernel": "k_sweep_dp<8, 32, 16, 1>", "block": 32, "workload": "cfg4", "src_sha256": "abc",
         "hbm_bytes_per_launch": 123.0}
    p.write_text(json.dumps(d))
    assert bench.load_traffic(str(p), 32, "cfg4", "abc") == 123.0
    assert bench.load_traffic(str(p), 32, "cfg4", "abd") is None
    assert bench.load_traffic(str(p), 32, "cfg3", "abc") is None
    assert bench.load_traffic(str(p), 16, "cfg4", "abc") is None
    p.write_text(json.dumps({"entries": [dict(d, workload="cfg3", hbm_bytes_per_launch=7.0), d]}))
    assert bench.load_traffic(str(p), 32, "cfg4", "abc") == 123.0
    assert bench.load_traffic(str(p), 32, "cfg3", "abc") == 7.0


def test_dense_pivot_is_the_reference_pivot():
    """pivot_dense (the CPU baseline's cost model: every column, as
    tableau.py:269-276) gives the same exact tableau as the oracle's pivot"""
    T = gen.tableau("mixed", 12, 10, 4)
    a, b = exact.from_array(T), exact.from_array(T)
    for _ in range(6):
        p = exact.find_standard(a)
        if isinstance(p, str):
            break
        exact.pivot(a, *p)
        exact.pivot_dense(b, *p)
        assert a == b


def test_cpu_baseline_sample_runs():
    """the bounded cpu_baseline leg on the cfg3 workload, a short sample"""
    r = bench.cpu_baseline("cfg3", seconds_target=0.5)
    assert r["cores"] == 1 and r["kind"] == "port" and r["value"] > 0
    assert "pivot_dense" in r["sample"]


def test_cpu_baseline_mid_run_sample():
    """the cpu_baseline's later-pivot point: the first pivots (here the
    reference's own cfg3 prefix, tests/golden/r3.json) replayed exactly on row
    0, the pivot rows and a sample, then pivot #(k+1) timed on the sample"""
    from conftest import load_golden
    seq = [tuple(p) for p in load_golden("r3.json")["standard_k"][0]["seq"]]
    r = bench.cpu_baseline("cfg3", seconds_target=0.5, seq=seq, k_mid=3)
    assert r["kind"] == "port" and r["cores"] == 1 and r["value"] > 0
    assert "seconds_per_pivot_at_1" in r and "seconds_per_pivot_at_4" in r
    assert r["seconds_per_pivot"] == r["seconds_per_pivot_at_4"]


class _FakeEngine:
    """records put_rows / run calls (bench's device warm-up and upload)"""

    def __init__(self, pivots_left=10 ** 9):
        self.puts, self.runs, self.left = [], [], pivots_left

    def put_rows(self, row0, rows):
        self.puts.append((row0, rows.shape[0], float(rows[0, 0])))

    def run(self, rule, k):
        done = min(k, self.left)
        self.left -= done
        self.runs.append(k)
        return (1 if done < k else 0), done          # 1: optimal (the LP ended inside the call)


def test_device_warmup_runs_whole_groups_and_stops_when_the_lp_ends():
    assert bench.device_warmup(None, 64, 150.0) == {"ms": 0.0, "groups": 0}
    h = _FakeEngine(pivots_left=64 * 20)
    r = bench.device_warmup(h, 64, 1e6)
    assert r["groups"] == 20 and h.runs == [512, 512, 512]
    h = _FakeEngine()
    r = bench.device_warmup(h, 64, 0.0)
    assert r["groups"] == 0 and h.runs == []


def test_upload_feeds_the_heater_the_same_rows_locally_numbered():
    kind, m, ns, n, a0, a1 = bench.workload("cfg3", 2, 1)
    e, h = _FakeEngine(), _FakeEngine()
    bench.upload([e], kind, m, ns, [(a0, a1)], blk=1024, heaters=[h])
    assert [p[0] for p in e.puts] == [0] + [1 + a for a in range(a0, a1, 1024)]
    assert [p[0] for p in h.puts] == [0] + [1 + a - a0 for a in range(a0, a1, 1024)]
    assert [p[1:] for p in e.puts] == [p[1:] for p in h.puts]


def test_profile_every_for_times_every_long_sweep():
    """cfg4 on one GPU (a 2.1 GB local tableau): every sweep launch timed
    (VERDICT r5); cfg3 and the 8-GPU rank: every 4th / 8th; an explicit
    --profile-every wins"""
    assert bench.profile_every_for(32769, 8192, 20, 0) == 1
    assert bench.profile_every_for(4097, 8192, 20, 0) == 4
    assert bench.profile_every_for(4097, 8192, 64, 0) == 8
    assert bench.profile_every_for(32769, 8192, 20, 3) == 3


class _ClockEngine:
    """sweep_clocks() as lpdiag_sweep_clocks returns it: (launch, cycles,
    100 MHz ticks, start tick), oldest first"""

    def __init__(self, rows):
        self.rows = np.array(rows, dtype=np.int64)

    def sweep_clocks(self, cap):
        return self.rows[-cap:]


def test_sweep_clock_summary_reads_the_clock():
    # 1.6 M cycles over 80,000 ticks (800 us) = 2.0 GHz; 1.6 M over 72,727 = 2.2 GHz
    rows = [[0, 1_600_000, 80_000, 0], [1, 1_600_000, 72_727, 90_000], [2, 1_700_000, 85_000, 170_000]]
    s = bench.sweep_clock_summary(_ClockEngine(rows), 2)
    assert s["launches"] == 2
    assert s["ghz_per_launch"] == [2.2, 2.0]
    assert abs(s["kcycles_mean"] - 1650.0) < 1e-9
    assert abs(s["block0_us_mean"] - (727.27 + 850.0) / 2) < 1e-9
    assert abs(s["ghz_min"] - 2.0) < 1e-9 and abs(s["ghz_max"] - 2.2) < 1e-4
    assert bench.sweep_clock_summary(_ClockEngine(np.zeros((0, 4))), 4) == {"launches": 0}


def test_sweep_clock_summary_survives_a_failing_engine():
    class Bad:
        def sweep_clocks(self, cap):
            raise RuntimeError("no clocks")
    assert bench.sweep_clock_summary(Bad(), 4) == {"error": "no clocks"}


def test_plain_run_measures_the_main_workload_only():
    """--full (off by default) is what adds the cfg3 leg and the CPU baseline;
    --dump-outputs names the directory of the last step's outputs"""
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 20, 5)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out" and not a.no_cfg3 and not a.no_cpu_baseline


def test_dump_rows_is_a_fixed_sample_within_the_size_limit():
    for name in ("cfg4", "cfg3"):
        _, m, _, n, _, _ = bench.workload(name, 1, 0)
        r = bench.dump_rows(m, n)
        assert r[0] == 0 and np.all(np.diff(r) > 0) and r[-1] <= m
        assert len(r) > 256 and len(r) * (n + 1) * 8 <= bench.DUMP_SAMPLE_BYTES
        assert np.array_equal(r, bench.dump_rows(m, n))
    assert bench.dump_rows(5, 7).tolist() == [0, 1, 2, 3, 4, 5]      # a small tableau: every row


class _DumpEngine:
    """a tableau whose cell (r, c) holds 1000 r + c, as one rank's engine"""

    def __init__(self, m, n, row_begin, row_count):
        self.m, self.n, self.row_begin, self.row_count = m, n, row_begin, row_count

    def rows(self, row0, nrows):
        assert row0 == 0 or self.row_begin < row0 <= self.row_begin + self.row_count
        return 1000.0 * np.arange(row0, row0 + nrows)[:, None] + np.arange(self.n + 1)[None, :]

    def log(self):
        return np.arange(12, dtype=np.int64).reshape(6, 2)

    def objective(self):
        return -2.5


def test_dump_outputs_writes_float64_arrays(tmp_path):
    d = str(tmp_path / "out")
    bench.dump_outputs(_DumpEngine(40, 7, 0, 40), d)
    files = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(files) == ["objective.npy", "pivot_log.npy", "tableau_row_index.npy", "tableau_rows.npy"]
    assert all(a.dtype == np.float64 for a in files.values())
    assert files["tableau_row_index.npy"].tolist() == list(range(41))
    assert np.array_equal(files["tableau_rows.npy"][:, 0], 1000.0 * np.arange(41))
    assert files["pivot_log.npy"].tolist() == np.arange(12.0).reshape(6, 2).tolist()
    assert files["objective.npy"].tolist() == [-2.5]


def test_dump_outputs_of_a_rank_keeps_its_own_rows(tmp_path):
    d = str(tmp_path)
    bench.dump_outputs(_DumpEngine(40, 7, 20, 20), d, rank=1)
    assert sorted(os.listdir(d)) == ["tableau_row_index.rank1.npy", "tableau_rows.rank1.npy"]
    assert np.load(os.path.join(d, "tableau_row_index.rank1.npy")).tolist() == list(range(21, 41))
    bench.dump_outputs(_DumpEngine(40, 7, 0, 20), d, rank=0)
    assert np.load(os.path.join(d, "tableau_row_index.rank0.npy")).tolist() == list(range(0, 21))


class _FiniteEngine(_FakeEngine):
    """an LP of `length` pivots that an upload starts over, behind lp_run's
    launch pattern: a call's groups go out in batches of `batch` pivots, with
    a check after each batch, so the groups of the batch in which the optimum
    is found still launch (and exit at once); every launch is event-timed"""

    def __init__(self, length, block, batch):
        super().__init__(pivots_left=length)
        self.length, self.block, self.batch = length, block, batch
        self.launches = 0

    def put_rows(self, row0, rows):
        super().put_rows(row0, rows)
        self.left = self.length

    def run(self, rule, k):
        self.runs.append(k)
        done = 0
        while done < k:
            b = min(self.batch, k - done)
            self.launches += -(-b // self.block)
            d = min(b, self.left)
            done, self.left = done + d, self.left - d
            if d < b:
                return 1, done                               # optimal inside this batch
        return 0, done

    def update_time(self):
        return 0.0, self.launches

    select_time = update_time

    def exchange_path(self):
        return bench._lib.PATH_PERSISTENT, 0


def test_run_steps_starts_the_lp_over_when_it_ends_inside_the_run():
    """a finite LP (150 pivots) timed for 10 steps of 64: five passes, the
    initial rows put back before each new one, 640 pivots in all; once the
    first pass has shown the LP's length no call asks for more than is left
    of it"""
    e = _FiniteEngine(150, 64, 1 << 15)
    kept = [(0, np.zeros((1, 3))), (1, np.ones((4, 3)))]
    state = {}
    assert bench.run_steps(e, 10, 64, kept, state=state) >= 0
    assert e.runs == [640, 150, 150, 150, 40]
    assert (state["in_pass"], state["restarts"], state["length"]) == (40, 4, 150)
    assert (state["idle_sweeps"], state["idle_selections"]) == (0, 0)       # event timing off: nothing read
    assert [p[:2] for p in e.puts] == [(0, 1), (1, 4)] * 4
    # the next call on the same engine goes on inside the pass
    bench.run_steps(e, 2, 64, kept, state=state)
    assert e.runs[5:] == [110, 18] and state["restarts"] == 5
    # within the LP's length: one call, as before; no steps: no call at all
    e, state = _FiniteEngine(150, 64, 1 << 15), {}
    bench.run_steps(e, 2, 64, kept, state=state)
    bench.run_steps(e, 0, 64, kept, state=state)
    assert e.runs == [128] and e.puts == [] and state["restarts"] == 0


@pytest.mark.parametrize("length,steps,batch", [(150, 10, 1 << 15), (1000, 40, 512), (1024, 40, 512), (1000, 40, 64)])
def test_run_steps_counts_the_launches_that_exited_at_once(length, steps, batch):
    """the idle launches are what the engine's launch counts show beyond the
    launches that worked -- whatever part of the call the engine had enqueued
    when it saw the optimum (here: batches of `batch` pivots), not the whole
    rest of the call"""
    block = 64
    e = _FiniteEngine(length, block, batch)
    state = {"every": 1}
    bench.run_steps(e, steps, block, [(0, np.zeros((1, 3)))], state=state)
    passes, rest = divmod(steps * block, length)
    worked = passes * -(-length // block) + -(-rest // block)
    assert state["idle_sweeps"] == e.launches - worked
    assert state["idle_sweeps"] <= -(-batch // block)
    # the selection of the group that found the optimum at its very start worked
    assert state["idle_selections"] == state["idle_sweeps"] - (1 if length % block == 0 else 0)


def test_run_steps_still_fails_on_any_other_early_end():
    with pytest.raises(SystemExit):                      # nothing kept to start over from
        bench.run_steps(_FakeEngine(pivots_left=100), 2, 64, None)

    class Unbounded(_FakeEngine):
        def run(self, rule, k):
            return 2, 10
    with pytest.raises(SystemExit):
        bench.run_steps(Unbounded(), 2, 64, [(0, np.zeros((1, 3)))])
    with pytest.raises(SystemExit):                      # an LP with no pivot at all
        bench.run_steps(_FakeEngine(pivots_left=0), 2, 64, [(0, np.zeros((1, 3)))])
