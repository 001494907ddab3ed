"""The drop-in claim, executed: INTEGRATION.md §2's two shim files laid over a copy of the reference
tree, and the reference's UNMODIFIED ``PipelineOrchestrator`` run end to end.

Build container only: ``/root/reference`` does not exist on the GPU box, so the test skips there.
The shim text is read out of INTEGRATION.md itself, so the document and the test cannot drift apart.
Without a GPU here, the B=1 device call behind ``MPCController.solve`` is the C restatement
(``tests/_dropin_driver.py``); the closed loop must reproduce ``closed_loop.npz``, the reference's
own loop (``/root/reference/src/pipeline/orchestrator.py:73-86``, ``control_stage.py:100-150``).
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
REFERENCE = Path(os.environ.get("RRT_MPC_REFERENCE", "/root/reference"))

needs_reference = pytest.mark.skipif(not (REFERENCE / "src" / "pipeline" / "orchestrator.py").exists(),
                                     reason="reference tree absent: its unmodified orchestrator cannot be run")


def integration_shims() -> dict:
    """{reference-relative path: file text} from the code blocks of INTEGRATION.md §2."""
    text = (ROOT / "INTEGRATION.md").read_text()
    sec = text.split("## 2.", 1)[1].split("\n## ", 1)[0]
    blocks = re.findall(r"```python\n(.*?)```", sec, flags=re.S)
    targets = re.findall(r"^`(src/[\w/]+\.py)`", sec, flags=re.M)
    assert len(blocks) == 2 and targets == ["src/control/mpc_controller.py", "src/pipeline/control_stage.py"], \
        (targets, len(blocks))
    return dict(zip(targets, blocks))


def _lay_shims(tmp_path: Path) -> Path:
    ref = tmp_path / "reference"
    shutil.copytree(REFERENCE / "src", ref / "src", ignore=shutil.ignore_patterns("__pycache__"))
    for rel, body in integration_shims().items():
        (ref / rel).write_text(body)
    return ref


def test_integration_shims_are_the_documented_ones():
    shims = integration_shims()
    assert "from mpcqp.control.mpc_controller import" in shims["src/control/mpc_controller.py"]
    assert "from mpcqp.pipeline.control_stage import TrajectoryTracker" in shims["src/pipeline/control_stage.py"]


@needs_reference
@pytest.mark.parametrize("N,sim_steps", [(10, 100), (15, 300)])
def test_unmodified_orchestrator_runs_on_the_shims(tmp_path, golden, N, sim_steps):
    import cpu_solver

    cpu_solver.build_library()
    ref = _lay_shims(tmp_path)
    # every other reference file is byte-for-byte the original
    for f in (REFERENCE / "src").rglob("*.py"):
        rel = f.relative_to(REFERENCE)
        if str(rel) not in integration_shims():
            assert (ref / rel).read_bytes() == f.read_bytes(), rel
    out = tmp_path / "run.npz"
    env = dict(os.environ, MPLBACKEND="Agg", PYTHONDONTWRITEBYTECODE="1")
    proc = subprocess.run([sys.executable, str(ROOT / "tests" / "_dropin_driver.py"), str(ref), str(out), str(N),
                           str(sim_steps)], capture_output=True, text=True, env=env, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    run = np.load(out)
    loop = golden("closed_loop.npz")
    plan = golden("default_plan.npz")
    np.testing.assert_array_equal(run["path"], plan["path"])  # the reference's planner, unchanged
    states = run["states"]
    assert states.shape == loop[f"N{N}_states"].shape == (65, 4)
    assert int(run["solves"]) == 65  # one QP per step, no relaxed retry
    np.testing.assert_allclose(states, loop[f"N{N}_states"], rtol=0, atol=1e-7)
    # the reference's orchestrator logged through the product tracker
    assert "MPC tracking finished after 65 steps (goal_reached=True)" in proc.stderr
