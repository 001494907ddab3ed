"""bench.py's host-side helpers behind ``--dump-outputs`` and the plain (no ``--full``) run."""
from __future__ import annotations

import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def _arrays(rows: int) -> dict:
    rng = np.random.default_rng(1)
    return {"u0": rng.standard_normal((rows, 2)), "X": rng.standard_normal((rows, 4, 21)),
            "status": np.ones(rows, np.int32), "active": rng.integers(0, 2, (rows, 101)).astype(np.uint8)}


def test_dump_outputs_writes_every_array_as_float64(tmp_path):
    import bench

    arr = _arrays(37)
    shapes = bench.dump_outputs(tmp_path / "d", arr)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == sorted(f"{k}.npy" for k in arr)
    for k, a in arr.items():
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == np.float64 and list(got.shape) == shapes[k] == list(a.shape)
        np.testing.assert_array_equal(got, a.astype(np.float64))


def test_dump_outputs_samples_the_same_rows_past_the_limit(tmp_path):
    import bench

    arr = _arrays(500)
    limit = 100_000
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, arr, limit=limit)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))
    idx = rows.astype(int)
    assert 0 < len(idx) < 500 and (np.diff(idx) > 0).all() and idx.max() < 500
    total = 0
    for k, a in arr.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        np.testing.assert_array_equal(got, a[idx].astype(np.float64))
        total += got.nbytes
    assert total + rows.nbytes <= limit
    assert bench.DUMP_LIMIT_BYTES <= 64 * 1000 * 1000


def test_clock_ramp_runs_untimed_steps_for_the_given_time():
    import bench

    calls = []
    spent = bench.clock_ramp(calls.append, lambda: None, seconds=0.01)
    assert spent >= 0.01 and len(calls) >= 16 and len(calls) % 16 == 0 and set(calls) == {-1}


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
