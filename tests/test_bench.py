"""bench.py's own contract: a plain run times its steps and prints the result line (nothing else), `--full` adds the untimed
extra measurements, `--dump-outputs DIR` writes what the last timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--size", "160", "--seeds", "150", "--steps", "3", "--warmup", "1"]
EXTRA = ("roofline_isolated", "roofline_full_occupancy", "full_trace_loop", "cpu_baseline")


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_float64_and_bounded(tmp_path, monkeypatch):
    """every array float64; past the limit the large arrays keep one fixed, seeded sample of rows (named in <name>_rows.npy),
    the small ones are written whole"""
    rng = np.random.default_rng(0)
    arrays = {"nodes": rng.random((20000, 9)).astype(np.float32), "links": np.arange(40000, dtype=np.int32).reshape(-1, 2),
              "jminmax": np.array([0.0, 0.5], np.float32), "traces_used": np.array([7])}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v), k
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1 << 20)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["jminmax.npy", "links.npy", "links_rows.npy", "nodes.npy", "nodes_rows.npy", "traces_used.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in files) <= 1 << 20  # payloads (128 B: a .npy header)
    for k in ("nodes", "links"):
        rows = np.load(tmp_path / "a" / (k + "_rows.npy")).astype(np.int64)
        assert 0 < len(rows) < len(arrays[k]) and np.all(np.diff(rows) > 0)
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), arrays[k][rows])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    assert np.array_equal(np.load(tmp_path / "a" / "jminmax.npy"), arrays["jminmax"])


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_what_the_step_computed(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        out = _bench(SMALL + ["--dump-outputs", str(d)])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
            assert k in out, k
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
        assert not set(out) & set(EXTRA), "a plain run measures nothing but its steps"
        arr = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert set(arr) == {"nodes", "links", "seeds", "jminmax", "traces_used"}
        assert all(a.dtype == np.float64 for a in arr.values())
        c = out["counts"]
        assert arr["nodes"].shape == (c["nodes"] + 1, 9) and arr["seeds"].shape == (c["n_seeds"], 8) and c["nodes"] > 50
        assert arr["links"].ndim == 2 and arr["links"].shape[1] == 2 and int(arr["traces_used"][0]) == c["traces_used"]
        assert 0 <= arr["jminmax"][0] < arr["jminmax"][1]
        runs.append(arr)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), k


@pytest.mark.gpu
def test_bench_full_adds_the_extra_measurements():
    out = _bench(SMALL + ["--full"])
    want = EXTRA if out["config"]["trace_groups"] > 1 else EXTRA[1:]  # (roofline_isolated: the one-group rerun of a several-group step)
    for k in want:
        assert out.get(k), k
    assert out["cpu_baseline"]["value"] > 0 and out["full_trace_loop"]["traces_used"] > 0 and out["roofline_full_occupancy"]["frac"] > 0
