#!/usr/bin/env python3
"""Config 1 (the reference's single-vehicle loop, N = 10, 65 solves) through the drop-in
TrajectoryTracker under several B=1 solver schedules: ms per step (best of 5) and the kernel's own
per-QP time (HIP events over the 65 windows from device memory).  Every schedule ends at the exact
optimum; the states must agree with the reference loop (closed_loop.npz) to 1e-7 px.

    python tools/b1_schedules.py > profiles/<round>_b1_schedules.json
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np
from bench_common import default_track_args

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "rrt-mpc_amd"), str(ROOT)]

SCHEDULES = [
    {"polish_from": 25},
    {"polish_from": 10, "check_termination": 10, "adaptive_rho_interval": 10},
    {"polish_from": 15, "check_termination": 15, "adaptive_rho_interval": 15},
    {"polish_from": 5, "check_termination": 5, "adaptive_rho_interval": 25},
    {"polish_from": 10, "check_termination": 10, "adaptive_rho_interval": 20},
]


def main() -> None:
    import torch

    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.control.mpc_controller import BatchedMPCController
    from mpcqp.pipeline.control_stage import TrajectoryTracker

    g = np.load(ROOT / "tests" / "golden" / "closed_loop.npz")
    ref_states = g["N10_states"]
    wins, x0s, ups = g["N10_window"], g["N10_x0"], g["N10_u_prev"]
    planning, maps = default_track_args()
    params = MPCConfig(horizon=10).to_parameters(0.8)
    dev = torch.device("cuda:0")
    x0_t, w_t, up_t = (torch.from_numpy(a).to(dev) for a in (x0s, wins, ups))
    out = []
    for sched in SCHEDULES:
        tr = TrajectoryTracker(MPCConfig(horizon=10, sim_steps=100), VizConfig(), solver_settings=dict(sched),
                               relaxed_solver_settings=dict(sched))
        st = tr.track(planning, maps, map_resolution=0.8, visualize=False).states
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            st = tr.track(planning, maps, map_resolution=0.8, visualize=False).states
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        dev_px = float(np.abs(np.asarray(st) - ref_states).max()) if len(st) == len(ref_states) else None
        ctrl = BatchedMPCController(params, 1, device=dev, **sched)
        stream = torch.cuda.current_stream(dev)
        ks, its = [], []
        for rep in range(2):
            for q in range(len(wins)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctrl.solve_raw(1, x0_t[q], w_t[q], up_t[q], stream)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if rep:
                    ks.append(e0.elapsed_time(e1) * 1e3)
                    its.append(ctrl._iters[0].cpu().numpy().tolist())
        ctrl.close()
        its = np.asarray(its, float)
        out.append({"settings": sched, "track_ms_per_step": 1e3 * best / len(st), "steps": len(st),
                    "max_state_diff_vs_reference_px": dev_px, "kernel_us_mean": float(np.mean(ks)),
                    "kernel_us_max": float(np.max(ks)), "iters_mean": its.mean(axis=0).round(2).tolist()})
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
