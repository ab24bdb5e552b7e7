"""bench.py's contract with its callers: --dump-outputs writes what the last timed step returned (float64, bounded in
size, the same seeded sample every run), and a plain run is the headline alone -- the rest is behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_small_batch_is_written_whole(tmp_path):
    import bench
    uact = np.arange(12, dtype=np.float64).reshape(1, 12) / 7.0
    rc = np.array([1, -1, 2, -3] * 3, dtype=np.int32)
    bench.dump_outputs(str(tmp_path), {"uact": uact, "rc": rc})
    assert sorted(os.listdir(tmp_path)) == ["rc.npy", "uact.npy"]
    u, r = np.load(tmp_path / "uact.npy"), np.load(tmp_path / "rc.npy")
    assert u.dtype == np.float64 and np.array_equal(u, uact)
    assert r.dtype == np.float64 and np.array_equal(r, rc)


def test_dump_outputs_large_batch_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    B = 1000
    uact = np.random.default_rng(3).standard_normal((2, B))
    rc = np.arange(B, dtype=np.int32)
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        bench.dump_outputs(str(d), {"uact": uact, "rc": rc})
        assert sorted(os.listdir(d)) == ["rc.npy", "sample_columns.npy", "uact.npy"]
        runs.append({n: np.load(d / f"{n}.npy") for n in ("uact", "rc", "sample_columns")})
        assert sum(a.nbytes for a in runs[-1].values()) <= 4096
    cols = runs[0]["sample_columns"].astype(np.int64)
    assert len(cols) > 0 and np.all(np.diff(cols) > 0) and cols[-1] < B
    assert np.array_equal(runs[0]["uact"], uact[:, cols]) and np.array_equal(runs[0]["rc"], cols)
    for n in runs[0]:
        assert np.array_equal(runs[0][n], runs[1][n])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_outputs(hip, tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "QP solves/sec (batched filter())" and line["unit"] == "QP solves/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert "configs" not in line and "c1" not in line and "pcie_inclusive" not in line
    assert line["cpu_baseline"] is None and "value_graph_replay" not in line
    B = line["config"]["batch_per_gpu"]
    uact, relax, rc = (np.load(out / f"{n}.npy") for n in ("uact", "relax", "rc"))
    assert uact.dtype == relax.dtype == rc.dtype == np.float64
    assert uact.shape == (1, B) and relax.shape[1] == B and rc.shape == (B,)
    hist = {str(int(k)): int(v) for k, v in zip(*np.unique(rc, return_counts=True))}
    assert hist == line["config"]["rc_histogram"]
    assert np.all(np.isfinite(uact[:, rc == 1]))
