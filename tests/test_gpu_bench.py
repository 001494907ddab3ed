"""A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` end to end: the line carries
the headline fields and nothing that belongs to `--full`, the K steps are the ones asked for, and two
runs write the same arrays (seeded inputs, a deterministic kernel), every QP's results in float64."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
FULL_ONLY = ("rel_err", "osqp_settings", "pipelined", "strong_config4", "cpu_baseline", "config1", "config5")
SHAPES = {"u0": (4096, 2), "X": (4096, 4, 21), "U": (4096, 2, 20), "status": (4096,), "iters": (4096, 4),
          "active": (4096, 101)}


def _plain_run(out_dir: Path) -> dict:
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "QP/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["metric"].startswith("MPC QP solves/s (horizon=20, batch=4096)")
        assert d["ms_per_step"] > 0 and d["solved_fraction"] == 1.0
        # value = solved QPs per second over the timed steps, ms_per_step the time of one of them
        assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
        assert d["clock_ramp_ms"] >= 200.0 and d["leg_order"] == ["headline"]
        assert not [k for k in FULL_ONLY if k in d]
        assert {k: tuple(v) for k, v in d["dumped_outputs"].items()} == SHAPES
    total = 0
    for name, shape in SHAPES.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == shape
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{k}.npy" for k in SHAPES)
    assert total <= 64 * 1000 * 1000
    assert (np.load(tmp_path / "a" / "status.npy") == 1).all()
