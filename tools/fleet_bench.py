#!/usr/bin/env python3
"""Closed-loop fleet benchmark (BASELINE config 5 style): V vehicles on
RRT*-branch plans, references built on the device, `sim_steps` closed-loop MPC steps each, every
step on the GPU (mpcqp_fleet_run, hipGraph replay per step; --fused: mpcqp_fleet_loop, the whole
loop in one launch).  Reports vehicle-steps/s (one vehicle-step =
window + nominal QP (+ relaxed retry) + plant + path_idx/goal update) and, for scale, the
reference-style host loop (TrajectoryTracker.track, one B=1 solve per step) on one vehicle.

    python tools/fleet_bench.py [--vehicles 100 1024 4096] [--steps 100] [--horizon 15] [--fused]

--classes K: a heterogeneous fleet (vehicle v runs under parameter block v mod K) in ONE launch
(mpcqp_fleet_loop_mixed) against the same vehicles as K homogeneous fused sub-fleets launched back to
back (mpcqp_fleet_loop each, --pairing applies to them); K = 1 measures the mixed kernel against the plain
fused loop.  --class-pairing on off: the mixed launch also with two vehicles of one class per wave
(mpcqp_set_class_pairing, N <= 15; side "mixed_paired").  The sides alternate within every repeat, the order
rotating from repeat to repeat; the references are loaded before the timed window, which holds the loop
launches up to a synchronise.

--warm: the cold fused loop against the warm-started one, interleaved in one process (warm_bench).  With
several --pairing modes every mode gets a cold and a warm side (--pairing on off: cold paired, warm paired,
cold unpaired, warm unpaired); --launch-steps K ... adds the warm loop as launches of K steps, with and
without the carried guess (mpcqp_fleet_loop_warm_carry).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
from bench_common import class_blocks, interleaved, loop_counts, summary, timed, track_args

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rrt-mpc_amd"))


def seconds(ts) -> dict:
    """``bench_common.summary`` under this tool's key names."""
    s = summary(ts)
    return {"seconds_median": s["median"], "seconds_min": s["min"], "seconds_max": s["max"], "seconds": s["all"]}


def loop_leg(fts, steps: int, K: int):
    """A leg of ``interleaved``: the seconds of ``steps`` steps of each tracker of ``fts`` in turn, as launches of
    K steps, up to a synchronise."""
    import torch

    def launches():
        for ft in fts:
            for _ in range(-(-steps // K)):
                ft.step(K)
    return lambda: timed(launches, torch.cuda.synchronize, time.perf_counter)[0]


def mixed_bench(a) -> None:
    """One mixed launch against K homogeneous fused sub-launches (see the module docstring)."""
    import torch

    from mpcqp import scenarios
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker

    dev = torch.device("cuda:0")
    K = a.classes
    out = {"metric": "closed-loop vehicle-steps/s, loop launches only", "horizon": a.horizon, "sim_steps": a.steps,
           "classes": K, "pairing_of_sub_fleets": a.pairing, "class_pairing": a.class_pairing,
           "reps_per_order": a.reps, "runs": []}
    mpc = MPCConfig(horizon=a.horizon, sim_steps=a.steps)
    blocks = class_blocks(mpc.to_parameters(0.8), K)
    for V in a.vehicles:
        paths, starts, goals = scenarios.fleet5(V)
        cls = np.arange(V) % K
        groups = [np.flatnonzero(cls == c) for c in range(K)]
        kw = dict(map_resolution=0.8, max_ref_len=160, device=dev, fused=True)
        mixes = {("mixed_paired" if mode == "on" else "mixed"): FleetTracker(mpc, max_vehicles=V, class_pairing=mode, **kw)
                 for mode in a.class_pairing}
        for ft in mixes.values():
            ft.set_classes(blocks)
        mixed = next(iter(mixes.values()))
        subs = [FleetTracker(mpc, max_vehicles=len(g), params=blocks[c], pairing=a.pairing, **kw)
                for c, g in enumerate(groups)]

        def load():
            for ft in mixes.values():
                ft.reset_from_plans(paths, starts, goals, device_reference=True, classes=cls)
            for ft, g in zip(subs, groups):
                ft.reset_from_plans([paths[i] for i in g], starts[g], goals[g], device_reference=True)

        # 2 reps + 1 repeats, the fleets loaded again before each
        times, _ = interleaved({"split": loop_leg(subs, a.steps, a.steps),
                                **{side: loop_leg([ft], a.steps, a.steps) for side, ft in mixes.items()}}, 2 * a.reps, load)
        rm = mixed.result()
        steps_split = np.zeros(V, dtype=np.int64)
        for ft, g in zip(subs, groups):
            steps_split[g] = ft.result().steps
        vsteps = int(rm.steps.sum())
        run = {"vehicles": V, **loop_counts(rm), "same_step_counts": bool((steps_split == rm.steps).all()),
               "max_steps_of_a_vehicle": int(rm.steps.max())}
        for side in [*mixes, "split"]:
            run[side] = {**seconds(times[side]), "value": vsteps / float(np.median(times[side]))}
        for side, ft in mixes.items():
            info, rs = ft.launch_info(), ft.result()
            run[side].update(per_wave=info["per_wave"], workgroups=info["workgroups"],
                             same_steps_and_phases=bool((rs.steps == rm.steps).all() and (rs.phase == rm.phase).all()))
            run[f"{side}_over_split_time"] = run[side]["seconds_median"] / run["split"]["seconds_median"]
        if len(mixes) == 2:
            run["mixed_paired_over_mixed_time"] = run["mixed_paired"]["seconds_median"] / run["mixed"]["seconds_median"]
        # per class: vehicle-steps and the longest vehicle (what sets a sub-launch's tail)
        run["per_class"] = [{"vehicles": len(g), "vehicle_steps": int(rm.steps[g].sum()),
                             "max_steps": int(rm.steps[g].max())} for g in groups]
        out["runs"].append(run)
        for ft in [*mixes.values(), *subs]:
            ft.close()
        print(json.dumps(run), flush=True)
    print(json.dumps(out))


def warm_bench(a) -> None:
    """The cold fused loop against the warm-started one (mpcqp_fleet_loop_warm) at each --guess-passes value,
    on the same vehicles: the sides alternate within every repeat, the order rotating from repeat to repeat;
    the timed window holds the loop launches up to a synchronise.
    --pairing takes one mode or several.  One: the sides are "cold" and "warm:P" under it (a warm loop pairs
    under "on" only).  Several: a cold and a warm side per mode, "cold/on", "warm:P/on", ...
    --launch-steps K ...: the warm loop as ceil(steps / K) launches of K steps each (no host check between
    them), without the carried guess ("warm:P/launch K": cold at every launch) and with it ("carry:P/launch K",
    mpcqp_fleet_loop_warm_carry), under the first --pairing mode, beside that mode's single launch."""
    import torch

    from mpcqp import scenarios
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker

    dev = torch.device("cuda:0")
    out = {"metric": "closed-loop vehicle-steps/s, loop launch only", "horizon": a.horizon, "sim_steps": a.steps,
           "pairing": a.pairing, "launch_steps": a.launch_steps, "plan": a.plan, "reps": a.reps, "runs": []}
    mpc = MPCConfig(horizon=a.horizon, sim_steps=a.steps)
    for V in a.vehicles:
        if a.plan == "config1":  # the default plan itself, every vehicle from its start
            plan = scenarios.load_default_plan()
            paths = [plan["path"]] * V
            starts = np.tile(np.asarray(plan["start"], dtype=float)[:2], (V, 1))
            goals = np.tile(np.asarray(plan["path"][-1], dtype=float)[:2], (V, 1))
        else:
            paths, starts, goals = scenarios.fleet5(V)
        ref_len = 160
        if a.plan == "config1":
            from mpcqp.control.ref_builder import build_reference

            ref_len = len(build_reference(paths[0], mpc.v_px_s, a.horizon, mpc.dt))
        kw = dict(map_resolution=0.8, max_vehicles=V, max_ref_len=ref_len, device=dev, fused=True)
        sides, chunk = {}, {}
        for mode in a.pairing:
            tag = f"/{mode}" if len(a.pairing) > 1 else ""
            sides[f"cold{tag}"] = FleetTracker(mpc, pairing=mode, **kw)
            for gp in a.guess_passes:
                sides[f"warm:{gp}{tag}"] = FleetTracker(mpc, warm_start=True, guess_passes=gp, pairing=mode, **kw)
        for K in a.launch_steps:
            for gp in a.guess_passes:
                for what, carry in (("warm", False), ("carry", True)):
                    k = f"{what}:{gp}/launch {K}"
                    sides[k] = FleetTracker(mpc, warm_start=True, guess_passes=gp, carry_guess=carry,
                                            pairing=a.pairing[0], **kw)
                    chunk[k] = K
        names = list(sides)
        first_cold = names[0]

        def load():
            for ft in sides.values():
                ft.reset_from_plans(paths, starts, goals, device_reference=a.plan != "config1")

        times, _ = interleaved({k: loop_leg([ft], a.steps, chunk.get(k, a.steps)) for k, ft in sides.items()}, a.reps, load)
        res = {k: ft.result() for k, ft in sides.items()}
        launches = {k: sides[k].launch_info() for k in names}
        cold = res[first_cold]
        run = {"vehicles": V, **loop_counts(cold)}
        for k in names:
            ts, rk = times[k], res[k]
            med = float(np.median(ts))
            run[k] = {**seconds(ts),
                      "value": int(rk.steps.sum()) / med, "time_over_cold": med / float(np.median(times[first_cold])),
                      "launches": -(-a.steps // chunk.get(k, a.steps)), "per_wave": launches[k]["per_wave"],
                      "workgroups": launches[k]["workgroups"],
                      "same_steps_and_phases": bool((rk.steps == cold.steps).all() and (rk.phase == cold.phase).all()),
                      "max_state_diff_vs_cold": max((float(np.abs(x - y).max()) for x, y in zip(rk.states, cold.states)
                                                     if len(x) and x.shape == y.shape), default=0.0)}
        out["runs"].append(run)
        for ft in sides.values():
            ft.close()
        print(json.dumps(run), flush=True)
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, nargs="+", default=[100, 1024, 4096])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused", action="store_true", help="mpcqp_fleet_loop: one launch for the whole loop")
    ap.add_argument("--pairing", nargs="+", default=["auto"], choices=["auto", "on", "off"],
                    help="two vehicles per wave for N <= 15 (mpcqp_set_pairing); with --warm several modes may be "
                         "given: a cold and a warm side per mode")
    ap.add_argument("--launch-steps", type=int, nargs="+", default=[],
                    help="with --warm: also run the warm loop as launches of K steps, with and without the carried "
                         "guess (mpcqp_fleet_loop_warm_carry)")
    ap.add_argument("--classes", type=int, default=0,
                    help="K > 0: one mixed fused launch (mpcqp_fleet_loop_mixed) against K homogeneous fused launches")
    ap.add_argument("--class-pairing", nargs="+", default=["off"], choices=["on", "off"],
                    help="with --classes: the mixed launch at one vehicle per wave (off), at two of one class per wave "
                         "(on, mpcqp_set_class_pairing), or both as sides of their own")
    ap.add_argument("--warm", action="store_true",
                    help="the cold fused loop against the warm-started one (mpcqp_fleet_loop_warm), interleaved")
    ap.add_argument("--guess-passes", type=int, nargs="+", default=None,
                    help="with --warm: the attempt's pass limits to compare (default: the library's)")
    ap.add_argument("--plan", default="fleet5", choices=["fleet5", "config1"],
                    help="with --warm: RRT*-branch plans, or every vehicle on the default (config-1) plan")
    a = ap.parse_args()
    if any(K < 1 for K in a.launch_steps):
        ap.error("--launch-steps takes step counts >= 1")
    if not a.warm:
        if len(a.pairing) > 1 or a.launch_steps:
            ap.error("several --pairing modes and --launch-steps go with --warm")
        a.pairing = a.pairing[0]
    if a.classes:
        mixed_bench(a)
        return
    if a.warm:
        if a.guess_passes is None:
            from mpcqp import _lib

            a.guess_passes = [_lib.DEFAULT_GUESS_PASSES]
        warm_bench(a)
        return
    import torch

    from mpcqp import scenarios
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.pipeline.control_stage import TrajectoryTracker
    from mpcqp.pipeline.fleet import FleetTracker

    dev = torch.device("cuda:0")
    out = {"metric": "closed-loop vehicle-steps/s", "horizon": a.horizon, "sim_steps": a.steps,
           "mode": "fused loop (mpcqp_fleet_loop)" if a.fused else "graph-replayed steps (mpcqp_fleet_run)", "runs": []}
    for V in a.vehicles:
        paths, starts, goals = scenarios.fleet5(V)
        mpc = MPCConfig(horizon=a.horizon, sim_steps=a.steps)
        ft = FleetTracker(mpc, map_resolution=0.8, max_vehicles=V, max_ref_len=160, device=dev, fused=a.fused,
                          pairing=a.pairing)
        best = None
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ft.reset_from_plans(paths, starts, goals, device_reference=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ft.step(a.steps)  # masked vehicles cost an exiting wave; no host check inside the run
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            dt = t2 - t0
            res = ft.result()
            if r and (best is None or dt < best[0]):
                best = (dt, res, t2 - t1, t1 - t0)
        dt, res, loop_dt, reset_dt = best
        vsteps = int(res.steps.sum())
        out["runs"].append({
            "vehicles": V, "seconds": dt, **loop_counts(res), "value": vsteps / dt, "ms_per_step": 1e3 * dt / a.steps,
            # the loop alone (ft.step after the references are built and loaded): the fused kernel
            "loop_seconds": loop_dt, "loop_value": vsteps / loop_dt, "reset_seconds": reset_dt,
        })
        ft.close()
        print(json.dumps(out["runs"][-1]), flush=True)
    # reference-style host loop: one vehicle, one solve (B=1 kernel launch + sync) per step
    paths, starts, goals = scenarios.fleet5(1)
    tr = TrajectoryTracker(MPCConfig(horizon=a.horizon, sim_steps=a.steps), VizConfig())
    planning, maps = track_args(paths[0], starts[0], goals[0])
    tr.track(planning, maps, map_resolution=0.8, visualize=False)
    t0 = time.perf_counter()
    st = tr.track(planning, maps, map_resolution=0.8, visualize=False).states
    dt = time.perf_counter() - t0
    out["host_loop_one_vehicle"] = {"vehicle_steps": len(st), "seconds": dt, "value": len(st) / dt}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
