"""bench.py's roofline bookkeeping on the CPU: the traffic field comes only from
a PMC summary of this exact library AND of this bench's workload (the det /
storm summaries of scripts/gpu_evidence.sh carry the same library hash).
And --dump-outputs: the arrays it writes (CPU, a stand-in engine), and on the
GPU a plain run's line and two identical dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _write(path, **kw):
    with open(path, "w") as f:
        json.dump(kw, f)


def test_pmc_workload_from_field_and_suffix(tmp_path):
    assert bench.pmc_workload(str(tmp_path / "pmc_k_step_r09.json"), {}) == bench.BENCH_WORKLOAD
    assert bench.pmc_workload(str(tmp_path / "pmc_k_step_r09_det.json"), {}) == "det"
    assert bench.pmc_workload(str(tmp_path / "pmc_k_step_r09_storm.json"), {}) == "storm"
    assert bench.pmc_workload(str(tmp_path / "pmc_k_step_x.json"), {"workload": "storm"}) == "storm"


def test_pmc_traffic_skips_other_workloads(tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    # same library hash: the general-path summaries sort after the bench's
    _write(prof / "pmc_k_step_r09.json", lib_sha16="abc", hbm_bytes_per_launch=1.0e8,
           workload=bench.BENCH_WORKLOAD)
    _write(prof / "pmc_k_step_r09_det.json", lib_sha16="abc", hbm_bytes_per_launch=8.0e8)
    _write(prof / "pmc_k_step_r09_storm.json", lib_sha16="abc", hbm_bytes_per_launch=7.0e9,
           workload="storm")
    _write(prof / "pmc_k_step_r08.json", lib_sha16="old", hbm_bytes_per_launch=2.0e8)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    v, src = bench.pmc_traffic("abc")
    assert v == 1.0e8 and src.endswith("pmc_k_step_r09.json")
    assert bench.pmc_traffic("nope") == (None, None)
    assert bench.pmc_traffic(None) == (None, None)


def test_committed_summaries_name_their_workload():
    """Every committed PMC summary resolves to one workload, and at most one
    bench-workload summary exists per library hash."""
    seen = {}
    prof = os.path.join(ROOT, "profiles")
    for f in sorted(os.listdir(prof)):
        if not (f.startswith("pmc_k_step_") and f.endswith(".json")):
            continue
        d = json.load(open(os.path.join(prof, f)))
        w = bench.pmc_workload(f, d)
        assert w in (bench.BENCH_WORKLOAD, "det", "storm"), f
        if w == bench.BENCH_WORKLOAD and d.get("lib_sha16"):
            seen.setdefault(d["lib_sha16"], []).append(f)
    dup = {k: v for k, v in seen.items() if len(v) > 1}
    assert not dup, dup


class _FakeEngine:
    """state_read / counts of an engine, for dump_outputs"""

    def __init__(self, st):
        self.st = st

    def state_read(self, ty):
        return self.st

    def counts(self):
        return {k: i + 1 for i, k in enumerate(bench.COUNT_KEYS)}


def _state(n):
    st = np.random.default_rng(1).integers(0, 1 << 64, size=(3, n), dtype=np.uint64)
    st[0, 0], st[1, 0], st[2, 0] = (1 << 64) - 1, 0, (1 << 32)      # the halves' extremes
    return st


def _load(d, name):
    a = np.load(os.path.join(d, name + ".npy"))
    assert a.dtype == np.float64
    return a


def test_dump_outputs_halves_are_exact(tmp_path):
    """--dump-outputs: every u64 state word comes back bit for bit from its two
    float64 halves; the counters and the (complete) index are written beside."""
    st, d = _state(1000), str(tmp_path / "nested" / "dump")
    bench.dump_outputs(_FakeEngine(st), 0, d, 0, 1)
    assert sorted(os.listdir(d)) == ["counts.npy", "state_hi.npy", "state_index.npy", "state_lo.npy"]
    hi, lo = _load(d, "state_hi"), _load(d, "state_lo")
    back = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    np.testing.assert_array_equal(back, st)
    np.testing.assert_array_equal(_load(d, "state_index"), np.arange(1000))
    np.testing.assert_array_equal(_load(d, "counts"), np.arange(1, len(bench.COUNT_KEYS) + 1))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """Past the byte limit the pingers are the same seeded sample in every run,
    and a second rank writes files of its own within its share of the limit."""
    st = _state(1000)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 56 * 200)
    idx = []
    for run, (rank, world, sfx) in enumerate([(0, 1, ""), (0, 1, ""), (1, 2, "_rank1")]):
        d = str(tmp_path / f"d{run}")
        bench.dump_outputs(_FakeEngine(st), 0, d, rank, world)
        i = _load(d, "state_index" + sfx).astype(np.int64)
        assert i.size == 200 // world and np.all(np.diff(i) > 0)
        back = ((_load(d, "state_hi" + sfx).astype(np.uint64) << np.uint64(32))
                | _load(d, "state_lo" + sfx).astype(np.uint64))
        np.testing.assert_array_equal(back, st[:, i])
        payload = sum(np.load(os.path.join(d, f)).nbytes for f in os.listdir(d))
        assert payload <= bench.DUMP_MAX_BYTES // world + 8 * len(bench.COUNT_KEYS)
        idx.append(i)
    np.testing.assert_array_equal(idx[0], idx[1])


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """A plain run times exactly --steps steps, leaves the legs of --full out,
    and two runs with the same arguments dump the same arrays."""
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--actors", "5000"]
    lines = [_bench(*argv, "--dump-outputs", str(tmp_path / d)) for d in "ab"]
    for ln in lines:
        assert ln["metric"] == "actor msgs/sec (node), message-ubench & ring"
        assert ln["unit"] == "msgs/s" and ln["higher_is_better"] is True and ln["dtype"] == "u64"
        assert ln["steps"] == 3 and ln["warmup"] == 2 and ln["ms_per_step"] > 0
        assert ln["value"] > 0 and ln["dropped"] == 0
        assert ln["cpu_baseline"] is None and ln["ring"] is None
        # steady state: every ping is forwarded, 5 per pinger per step
        assert ln["msgs_per_step"] == 5 * 5000
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == 4
    for f in os.listdir(a):
        np.testing.assert_array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f)))
    counts = dict(zip(bench.COUNT_KEYS, _load(a, "counts")))
    assert counts["steps"] == 5 and counts["delivered"] == 5 * 5 * 5000
    # the pingers' third word counts the pings each has handled
    pings = _load(a, "state_hi")[2] * 2.0 ** 32 + _load(a, "state_lo")[2]
    assert pings.size == 5000 and pings.sum() == counts["delivered"]
