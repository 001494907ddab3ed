#!/usr/bin/env python3
"""Where a B=1 drop-in step's time goes (config 1: one QP per closed-loop step, N = 10).

    python tools/b1_latency.py [--horizon 10] [--calls 400] > profiles/<round>_b1_latency.json

Each figure is the best of 5 repeats of `calls` calls on the config-1 windows (the reference loop's
own 65 windows of closed_loop.npz, cycled):
  * staged_c          mpcqp_solve_staged alone (inputs already in the mapped block): launch + kernel +
                      stream sync, the library's floor for one QP from the host;
  * solve_one         BatchedMPCController.solve_one (write the inputs, the staged call, copy outputs);
  * mpc_controller    MPCController(params).solve as the tracker calls it (+ argument handling and
                      the controller cache lookup);
  * device_inputs     the same QP from device memory with the caller's torch stream: mpcqp_build +
                      mpcqp_solve + torch.cuda.synchronize (no mapped memory);
  * kernel_event_us   HIP events around the device-input solve (the kernel alone, on its stream);
  * track_ms_per_step the whole drop-in TrajectoryTracker.track loop (bench.py's config1 figure).

    python tools/b1_latency.py --warm [--horizons 10 15 20] [--reps 5] > profiles/served_warm/<name>.json

The warm start of the B = 1 path against the cold path of the same process, interleaved (cold block,
warm block, cold block, ...), each figure the median of `reps` repeats, per horizon on the config-1 plan's
own closed loop (its windows, and as the guess of window k the U of window k - 1 shifted one step):
  * solve_one_us       BatchedMPCController.solve_one per window: the served call with its input writes,
                       cold and with U_guess (which adds the guess write and the warm served call);
  * kernel_event_us    HIP events around mpcqp_build + mpcqp_solve / mpcqp_solve_warm of the same QPs from
                       device memory (k_solve<N> / k_solve_warm<N> at B = 1: the solve alone);
  * track_ms_per_step  TrajectoryTracker.track, cold and with warm_start=True;
  * hit_rate           solves from a guess that ended without an ADMM iteration (iters[0] == 0);
  * guess_write_us     the host's share: shifting the previous U and writing it into the guess block.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
from bench_common import default_track_args, interleaved

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "rrt-mpc_amd"), str(ROOT)]


def best_of(fn, calls: int, reps: int = 5) -> float:
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        for k in range(calls):
            fn(k)
        dt = (time.perf_counter() - t0) / calls * 1e6
        best = dt if best is None else min(best, dt)
    return best


def _median_blocks(fns: dict, reps: int) -> tuple:
    """(name -> median over `reps` of fn() (a time), name -> every repeat), the functions taking turns
    within each repeat: always in the order given, and every block warms itself up, so no repeat 0"""
    got, _ = interleaved(fns, reps, rotate=False, warmup=False)
    return {name: float(np.median(v)) for name, v in got.items()}, got


def warm_horizon(N: int, reps: int) -> dict:
    """The cold and the warm B = 1 path at horizon N on the config-1 plan (see the module docstring)."""
    import torch

    from mpcqp import _lib
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.control.mpc_controller import _single_controller
    from mpcqp.control.vehicle_model import f_discrete
    from mpcqp.control.ref_builder import build_reference
    from mpcqp.pipeline.control_stage import TrajectoryTracker, window_at

    planning, maps = default_track_args()
    path = planning.plan.path
    mpc = MPCConfig(horizon=N, sim_steps=300)
    params = mpc.to_parameters(0.8)
    ctrl = _single_controller(params)

    # the loop's own windows and optima (TrajectoryTracker.track's loop, cold)
    state = np.array([maps.start[0], maps.start[1], np.arctan2(path[1][1] - path[0][1], path[1][0] - path[0][0]), 5.0])
    u_prev, path_idx = np.zeros(2), 0
    ref_global = build_reference(path, mpc.v_px_s, N, mpc.dt)
    x0s, wins, ups, Us = [], [], [], []
    for _ in range(mpc.sim_steps):
        w = window_at(ref_global, path_idx, N)
        st, u0, X, U = ctrl.solve_one(state, w, u_prev)
        if st != _lib.SOLVED:
            raise SystemExit(f"N={N}: status {st} on the plan's own loop")
        x0s.append(state.copy()), wins.append(w.copy()), ups.append(u_prev.copy()), Us.append(U)
        state = f_discrete(state, u0, params.dt, params.wheelbase_px)
        u_prev = u0.copy()
        if path_idx < len(ref_global) - 2 and np.sum((state[:2] - ref_global[path_idx][:2]) ** 2) > 25.0:
            path_idx += 1
        if np.hypot(state[0] - maps.goal[0], state[1] - maps.goal[1]) < 8.0:
            break
    n = len(x0s)
    guesses = [None] + [np.concatenate([Us[k - 1][:, 1:], Us[k - 1][:, -1:]], axis=1) for k in range(1, n)]
    out = {"horizon": N, "windows": n, "reps": reps, "guess_passes": _lib.DEFAULT_GUESS_PASSES,
           "settings": dict(ctrl.settings)}

    def served(warm):
        def block():
            kw = lambda k: dict(U_guess=guesses[k]) if warm else {}  # noqa: E731
            ctrl.solve_one(x0s[1], wins[1], ups[1], **kw(1))  # the wave of this kind is resident
            t0 = time.perf_counter()
            for k in range(1, n):
                ctrl.solve_one(x0s[k], wins[k], ups[k], **kw(k))
            return (time.perf_counter() - t0) / (n - 1) * 1e6
        return block

    med, runs = _median_blocks({"cold": served(False), "warm": served(True)}, reps)
    out["solve_one_us"] = {**med, "runs": runs}
    hits = 0
    for k in range(1, n):
        ctrl.solve_one(x0s[k], wins[k], ups[k], U_guess=guesses[k])
        hits += int(ctrl.last_iters[0] == 0)
    out["hit_rate"] = {"hits": hits, "attempts": n - 1}

    # the host's share of a warm call: the shift and the write into the mapped block
    block = ctrl._one["guess"]

    def guess_write():
        t0 = time.perf_counter()
        for k in range(1, n):
            U = Us[k - 1]
            block[:] = np.asarray(np.concatenate([U[:, 1:], U[:, -1:]], axis=1), dtype=float)
        return (time.perf_counter() - t0) / (n - 1) * 1e6

    out["guess_write_us"] = _median_blocks({"shift_and_write": guess_write}, reps)[0]["shift_and_write"]

    # the kernels alone: the same QPs from device memory, HIP events around build + solve
    dev = torch.device("cuda:0")
    x0_t, w_t, up_t = (torch.from_numpy(np.stack(v)).to(dev) for v in (x0s, wins, ups))
    g_t = torch.from_numpy(np.stack([Us[0]] + guesses[1:])).to(dev)
    stream = torch.cuda.current_stream(dev)

    def kernel(warm):
        def block():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for q in range(1, n):
                ev[q][0].record(stream)
                ctrl.solve_raw(1, x0_t[q], w_t[q], up_t[q], stream, U_guess=g_t[q] if warm else None)
                ev[q][1].record(stream)
                torch.cuda.synchronize(dev)
            return float(np.mean([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[1:]]))
        return block

    med, runs = _median_blocks({"cold": kernel(False), "warm": kernel(True)}, reps)
    out["kernel_event_us"] = {**med, "runs": runs}

    trackers = {"cold": TrajectoryTracker(mpc, VizConfig()), "warm": TrajectoryTracker(mpc, VizConfig(), warm_start=True)}

    def track(name):
        def block():
            t0 = time.perf_counter()
            st = trackers[name].track(planning, maps, map_resolution=0.8, visualize=False).states
            return 1e3 * (time.perf_counter() - t0) / len(st)
        return block

    for name in trackers:
        track(name)()
    t = trackers["warm"]
    out["track_hit_rate"] = {"hits": t.warm_hits, "attempts": t.warm_attempts}
    med, runs = _median_blocks({name: track(name) for name in trackers}, reps)
    out["track_ms_per_step"] = {**med, "runs": runs}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warm", action="store_true", help="the warm start against the cold path, interleaved")
    ap.add_argument("--horizons", type=int, nargs="+", default=[10, 15, 20], help="with --warm")
    ap.add_argument("--reps", type=int, default=5, help="with --warm: repeats per figure (medians; at least 5)")
    a = ap.parse_args()
    if a.warm:
        if a.reps < 5:
            raise SystemExit("--reps must be at least 5")
        print(json.dumps({"warm": [warm_horizon(N, a.reps) for N in a.horizons]}, indent=1))
        return
    import torch

    from mpcqp import _lib
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.control.mpc_controller import MPCController, _single_controller
    from mpcqp.pipeline.control_stage import TrajectoryTracker

    N = a.horizon
    g = np.load(ROOT / "tests" / "golden" / "closed_loop.npz")
    key = f"N{N}_window" if f"N{N}_window" in g.files else None
    if key is None:
        raise SystemExit(f"closed_loop.npz has no N={N} windows ({g.files})")
    wins, x0s, ups = g[f"N{N}_window"], g[f"N{N}_x0"], g[f"N{N}_u_prev"]
    n = len(wins)
    params = MPCConfig(horizon=N).to_parameters(0.8)
    ctrl = _single_controller(params)
    L = _lib.lib()
    out = {"horizon": N, "calls": a.calls, "windows": n, "settings": dict(ctrl.settings)}

    ctrl.solve_one(x0s[0], wins[0], ups[0])  # warm: staging blocks, code objects
    io = ctrl._one

    def staged(k):
        q = k % n
        io["x0"][:] = x0s[q]
        io["ref"][:] = wins[q]
        io["up"][:] = ups[q]
        L.mpcqp_solve_staged(ctrl._ws)

    # the C call alone: the inputs written once, then the call repeated on them
    staged(0)
    out["staged_c_us"] = best_of(lambda k: L.mpcqp_solve_staged(ctrl._ws), a.calls)
    out["staged_with_input_writes_us"] = best_of(staged, a.calls)
    out["solve_one_us"] = best_of(lambda k: ctrl.solve_one(x0s[k % n], wins[k % n], ups[k % n]), a.calls)
    out["mpc_controller_us"] = best_of(
        lambda k: MPCController(params).solve(x0s[k % n], wins[k % n], u_prev=ups[k % n]), a.calls)

    dev = torch.device("cuda:0")
    x0_t = torch.from_numpy(x0s).to(dev)
    w_t = torch.from_numpy(wins).to(dev)
    up_t = torch.from_numpy(ups).to(dev)
    stream = torch.cuda.current_stream(dev)

    def device_call(k):
        q = k % n
        ctrl.solve_raw(1, x0_t[q], w_t[q], up_t[q], stream)
        torch.cuda.synchronize(dev)

    out["device_inputs_us"] = best_of(device_call, a.calls)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for q in range(n):
        ev[q][0].record(stream)
        ctrl.solve_raw(1, x0_t[q], w_t[q], up_t[q], stream)
        ev[q][1].record(stream)
        torch.cuda.synchronize(dev)
    ks = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])
    out["kernel_event_us"] = {"mean": float(ks.mean()), "min": float(ks.min()), "max": float(ks.max())}

    tracker = TrajectoryTracker(MPCConfig(horizon=N, sim_steps=100), VizConfig())
    planning, maps = default_track_args()
    tracker.track(planning, maps, map_resolution=0.8, visualize=False)
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        st = tracker.track(planning, maps, map_resolution=0.8, visualize=False).states
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["track_ms_per_step"] = 1e3 * best / len(st)
    out["track_steps"] = len(st)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
