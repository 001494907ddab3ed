#!/usr/bin/env python3
"""Development check for kernel rewrites meant to be bit-identical: solves the same batches with
each library (tools/ablibs/<name>.so, one subprocess each) and compares every output bit for bit.

    python tools/ab_bitwise.py --libs base new --out gpurun_out/bitwise.json

--loops: beside the batches, the warm fused loops at the GPU tests' own sizes (tests/gpu_helpers.py): every
fleet buffer, masks included, and the carried guess after the warm fleet loop, after the carried loop split
into launches, and after the warm swarm with its trigger firing.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CASES = [  # (config, horizon, batch, pairing, settings)
    ("config3", 20, 4096, "auto", {}),
    ("config2", 20, 1024, "auto", {}),
    ("config4", 30, 2048, "auto", {}),
    ("config3", 15, 4096, "on", {}),
    ("config3", 10, 1024, "off", {"polish_from": 25}),
    ("config3", 20, 1024, "auto", {"max_iter": 40, "polish": 0}),
]
MID_CASES = [  # the mid-horizon kernel (N = 33..64)
    ("config3", 33, 1024, "auto", {}),
    ("config3", 40, 1024, "auto", {}),
    ("config3", 48, 512, "auto", {}),
    ("config3", 56, 512, "auto", {}),
    ("config3", 64, 512, "auto", {}),
    ("config3", 40, 512, "auto", {"max_iter": 40, "polish": 0}),
    ("config3", 37, 512, "auto", {}),  # N < NT: padding steps in every bucket
    ("config3", 45, 512, "auto", {}),
    ("config3", 53, 256, "auto", {}),
    ("config3", 61, 256, "auto", {}),
]
EXTRA_CASES = [  # the sweep's other paths: the first LDS-column horizon, packed Pbar, no padding lane, a small pair
    ("config3", 17, 1024, "auto", {}),
    ("config3", 24, 1024, "auto", {}),
    ("config3", 32, 1024, "auto", {}),
    ("config3", 9, 4096, "on", {}),
    ("config3", 16, 1024, "off", {}),
    ("config3", 15, 4096, "on", {"max_iter": 40, "polish": 0}),
]
if os.environ.get("MPCQP_AB_MID") == "1":
    CASES = MID_CASES
if os.environ.get("MPCQP_AB_EXTRA") == "1":
    CASES = CASES + EXTRA_CASES
# --loops: (kind, ...) with pairing last.  "fleet": horizon, steps (None: to the end) -- V = 5 on plans of
# different lengths (test_gpu_warm_pair.py); "carry": horizon, the launches before the rest -- V = 4 on the
# golden plan; "swarm": V, steps, replan distance, max_replans, seed (test_gpu_swarm_warm.py's swarms)
LOOP_CASES = [("fleet", N, steps, pairing) for N, steps in ((1, 40), (10, None), (15, None), (16, 40), (32, 40))
              for pairing in ("off", "on") if pairing == "off" or N <= 15]
LOOP_CASES += [("carry", 10, (1, 3), pairing) for pairing in ("off", "on")]
LOOP_CASES += [("swarm", *cfg, pairing) for cfg in ((40, 200, 2.5, 2, 21), (64, 120, 1.5, 1, 33), (64, 120, 1.5, 3, 33))
               for pairing in ("off", "on")]


def child(out: str, loops: bool = False) -> None:
    sys.path.insert(0, str(ROOT / "rrt-mpc_amd"))
    from mpcqp import scenarios
    from mpcqp.config import MPCConfig
    from mpcqp.control.mpc_controller import BatchedMPCController

    res = {}
    for i, (cfg, N, B, pairing, sett) in enumerate(CASES):
        b = getattr(scenarios, cfg)(B, horizon=N)
        ctrl = BatchedMPCController(MPCConfig(horizon=N).to_parameters(0.8), B, device="cuda:0", pairing=pairing,
                                    **sett)
        sol = ctrl.solve_batch(b.x0[:B], b.ref[:B], b.u_prev[:B])
        for k in ("u0", "X", "U", "status", "iters", "active"):
            res[f"{i}_{k}"] = getattr(sol, k).cpu().numpy()
        ctrl.close()
    if loops:
        res.update(loop_outputs())
    np.savez(out, **res)


def loop_outputs() -> dict:
    """LOOP_CASES under the library of this process: LOOP_BUFFERS_MASK and U_carry of each case's tracker,
    and the swarm's per-vehicle result arrays."""
    for p in (ROOT / "tests", ROOT / "oracle"):
        sys.path.insert(0, str(p))
    import gpu_helpers as gh

    golden = lambda name: dict(np.load(ROOT / "tests" / "golden" / name, allow_pickle=False))  # noqa: E731
    res = {}

    def keep(tag, ft):
        for k, v in gh.snap(ft).items():
            res[f"{tag}_{k}"] = v
        carry = ft.buffers().get("U_carry")
        if carry is not None:
            res[f"{tag}_U_carry"] = carry[:ft.vehicles].cpu().numpy().copy()
        ft.close()

    for case in LOOP_CASES:
        tag = "_".join(map(str, case)).replace(" ", "")
        if case[0] == "fleet":
            _, N, steps, pairing = case
            plans = gh.varied_fleet(golden, 5, seed=41 + N)[1:]
            ft = gh.fleet_tracker(N, 5, 128, sim_steps=steps or 300, fused=True, warm_start=True, pairing=pairing)
            ft.reset_from_plans(*plans)
            ft.run() if steps is None else ft.step(steps)
        elif case[0] == "carry":
            _, N, chunks, pairing = case
            g, path = gh.default_plan(golden)
            ft = gh.fleet_tracker(N, 4, 64, sim_steps=100, map_resolution=float(g["map_resolution"]), fused=True,
                                  warm_start=True, carry_guess=True, pairing=pairing)
            ft.reset_from_plans([path] * 4, np.tile(g["start"], (4, 1)), np.tile(g["goal"], (4, 1)))
            for k in (*chunks, ft.max_steps):
                ft.step(k)
        else:
            _, V, steps, dist, max_replans, seed, pairing = case
            occ = golden("default_plan.npz")["occupancy"]
            starts, goals = gh.pairs(occ, V, seed)
            sw = gh.swarm(occ, V, steps, replan_distance=dist, max_replans=max_replans, fused=True, warm_start=True,
                          pairing=pairing)
            r = sw.run(starts, goals, seeds=np.arange(V))
            assert r.replans.sum() > 0, "the trigger should fire"
            for k in ("phase", "steps", "replans", "replan_steps"):
                res[f"{tag}_result_{k}"] = np.asarray(getattr(r, k))
            ft = sw.fleet
        keep(tag, ft)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", default=None)
    ap.add_argument("--mid", action="store_true", help="the mid-horizon cases (N = 33..64) instead")
    ap.add_argument("--loops", action="store_true", help="also the warm fused loops (fleet, carried, swarm)")
    ap.add_argument("--extra", action="store_true", help="also EXTRA_CASES (N = 17, 24, 32, 16, pairs at 9 and 15)")
    a = ap.parse_args()
    if a.mid:
        os.environ["MPCQP_AB_MID"] = "1"
    if a.extra:  # the children read the environment; this process lists the cases in its summary
        global CASES
        os.environ["MPCQP_AB_EXTRA"] = "1"
        CASES = CASES + EXTRA_CASES
    if a.child:
        child(a.child, a.loops)
        return
    outs = []
    with tempfile.TemporaryDirectory() as d:
        for lib in a.libs:
            f = os.path.join(d, f"{lib}.npz")
            env = dict(os.environ, MPCQP_LIB=str(ROOT / "tools" / "ablibs" / f"{lib}.so"), MPCQP_ABI_ANY="1")
            subprocess.run([sys.executable, __file__, "--libs", *a.libs, "--out", a.out, "--child", f,
                            *(["--loops"] if a.loops else [])], env=env, check=True, timeout=300)
            outs.append(dict(np.load(f)))
    rep = {}
    assert set(outs[0]) == set(outs[1]), sorted(set(outs[0]) ^ set(outs[1]))
    for k in outs[0]:
        x, y = outs[0][k], outs[1][k]
        same = x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        rep[k] = {"bitwise_equal": bool(same)}
        if not same and x.dtype.kind == "f":
            rep[k]["max_abs_diff"] = float(np.nanmax(np.abs(x - y)))
    summary = {"cases": [list(map(str, c)) for c in CASES + (LOOP_CASES if a.loops else [])], "all_equal": all(v["bitwise_equal"] for v in rep.values()),
               "fields": rep}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(summary, indent=1))
    print(json.dumps({"all_equal": summary["all_equal"],
                      "differ": [k for k, v in rep.items() if not v["bitwise_equal"]]}))


if __name__ == "__main__":
    main()
