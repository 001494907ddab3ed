"""GPU tests of the warm start in the fused swarm (``mpcqp_swarm_loop_warm``, ``k_swarm_loop_warm<N, Pair>``,
``Swarm(fused=True, warm_start=True)``): the warm loop with the replan trigger live inside it.

The swarms are the ones test_gpu_swarm.py fires the trigger on with the cold loop.  With no passes the warm
swarm is the cold fused swarm bit for bit; with passes it is held to the reference as the cold swarm is
(host loop and host planner, the cold test's tolerances), it is the warm fleet loop vehicle by vehicle and
segment by segment bit for bit, paired equals unpaired bit for bit with one half of a wave leaving through
the trigger while the other goes on, and a refused call writes nothing.  Every swarm run is made once per
configuration and shared by the tests that read it; nothing mutates a shared run."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
from gpu_helpers import (ATOL, E_HORIZON, LOOP_BUFFERS_MASK, SWARM_HORIZON as N_HORIZON, assert_same, fleet_tracker,
                         oracle_plan, pairs, planner_params, snap, swarm)

pytestmark = pytest.mark.gpu

# V, steps, replan distance (px), max_replans, seed of the (start, goal) pairs: test_gpu_swarm.py's
V40 = (40, 200, 2.5, 2, 21)
V64 = (64, 120, 1.5, 3, 33)
V100 = (100, 150, 5.5, 1, 7)
RESULT_ARRAYS = ("phase", "steps", "replans", "planned", "replan_steps", "last_replan_start", "replan_over_capacity")
RESULT_LISTS = ("states", "inputs", "paths", "last_replan_path")

_RUNS: dict = {}


def _run(golden, V, steps, dist, max_replans, seed, **kw):
    """One Swarm.run of the configuration (cached): its result, the fleet's buffers afterwards, the final
    references, the launch record of the nominal workspace, and the problem."""
    key = (V, steps, dist, max_replans, seed, tuple(sorted(kw.items())))
    if key not in _RUNS:
        occ = golden("default_plan.npz")["occupancy"]
        starts, goals = pairs(occ, V, seed)
        sw = swarm(occ, V, steps, replan_distance=dist, max_replans=max_replans, **kw)
        res = sw.run(starts, goals, seeds=np.arange(V))
        b = sw.fleet.buffers()
        _RUNS[key] = SimpleNamespace(res=res, bufs=snap(sw.fleet), ref=b["ref_global"][:V].clone(),
                                     ref_len=b["ref_len"][:V].clone(), info=sw.fleet._nominal.launch_info(),
                                     occ=occ, starts=starts, goals=goals, steps=steps)
        sw.fleet.close()
    return _RUNS[key]


def _assert_same_result(a, b, what):
    """Every SwarmResult field but the timings, bit for bit."""
    for k in RESULT_ARRAYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what}: {k}")
    for k in RESULT_LISTS:
        la, lb = getattr(a, k), getattr(b, k)
        assert len(la) == len(lb), (what, k)
        for v, (x, y) in enumerate(zip(la, lb)):
            assert (x is None) == (y is None), (what, k, v)
            if x is not None:
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=f"{what}: {k}[{v}]")


# ---------------------------------------------------------------------- host checkers (no GPU in them)
def _c_solve(params, state, window, u_prev):
    """One QP by the C restatement (oracle/mpcqp_cpu.c)."""
    import cpu_solver

    out = cpu_solver.cpu_solve(params, np.asarray(state, float)[None], np.asarray(window, float)[None],
                               np.asarray(u_prev, float)[None], nthreads=1)
    if out["status"][0] not in (1, 2):
        return None, None, None
    return out["u0"][0].copy(), out["X"][0].copy(), out["U"][0].copy()


def _oracle_params():
    import mpc_oracle as mo

    return mo.default_params(N_HORIZON, 0.8)


def _host_track(path, start, goal, steps):
    """The reference's track loop (control_stage.py:79-150) restated by the oracle, C solves."""
    import mpc_oracle as mo
    from mpcqp.control.ref_builder import build_reference

    ref = build_reference(path, 15.0, N_HORIZON, 0.1)
    yaw0 = float(np.arctan2(path[1][1] - path[0][1], path[1][0] - path[0][0])) if len(path) > 1 else 0.0
    return np.asarray(mo.track_loop(_oracle_params(), ref, start, yaw0, goal, steps, solve_fn=_c_solve))


def _host_continue(state, u_prev, path, goal, steps):
    """The loop body of control_stage.py:100-150 from a given state / u_prev on a new plan."""
    import mpc_oracle as mo
    from mpcqp.control.ref_builder import build_reference

    ref = build_reference(path, 15.0, N_HORIZON, 0.1)
    return np.asarray(mo.track_from(_oracle_params(), ref, state, u_prev, goal, steps, solve_fn=_c_solve))


def _check_plan(occ, start, goal, seed, path, tol=1e-4):
    """The device plan against the host restatement of the reference planner: "libm" or "cr" (the plan with
    correctly rounded steer trig, rare)."""
    got = np.asarray(path)

    def same(plan):
        return plan is not None and np.asarray(plan).shape == got.shape and \
            np.abs(np.asarray(plan) - got).max() <= tol

    if same(oracle_plan(occ, start, goal, seed)):
        return "libm"
    plan = oracle_plan(occ, start, goal, seed, cr=True)
    assert plan is not None
    ref = np.asarray(plan)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    np.testing.assert_allclose(got, ref, rtol=0, atol=tol)
    return "cr"


# ---------------------------------------------------------------------- 1. no passes is the cold swarm
@pytest.mark.parametrize("pairing", ["off", "on"])
@pytest.mark.parametrize("cfg", [V40, V64], ids=["v40", "v64"])
def test_no_passes_is_the_cold_fused_swarm(cuda, golden, cfg, pairing):
    """guess_passes = 0: every SwarmResult field and every fleet buffer equals Swarm(fused=True)'s bit for
    bit, one and two vehicles per wave, with the trigger firing."""
    cold = _run(golden, *cfg, fused=True, pairing=pairing)
    warm = _run(golden, *cfg, fused=True, warm_start=True, guess_passes=0, pairing=pairing)
    assert cold.res.replans.sum() > 0, "the trigger should fire"
    _assert_same_result(warm.res, cold.res, f"{cfg} {pairing}")
    assert_same(warm.bufs, cold.bufs, f"{cfg} {pairing}", LOOP_BUFFERS_MASK)
    assert warm.info["name"] == "loop_warm" and cold.info["name"] == "loop", (warm.info, cold.info)
    assert warm.info["per_wave"] == (2 if pairing == "on" else 1), warm.info


# ---------------------------------------------------------------------- 2. held to the reference
def test_warm_swarm_100_vehicles_follows_the_reference(cuda, golden):
    """Config 5 at its size, warm with the default passes, under test_per_step_replan_100_vehicles' assertions
    and tolerances: every never-replanned vehicle equals the host loop on its own plan (1e-7 px), every
    replanned one equals it up to its replan step, plans from exactly where it stood, gets the reference
    planner's plan at its replan seed and follows the host loop on it (1e-6 px).  And the run is not the cold
    one: some trace differs from the cold fused swarm's in some bit."""
    from mpcqp import _lib
    from mpcqp.pipeline.swarm import replan_seed

    V, steps = V100[0], V100[1]
    run = _run(golden, *V100, fused=True, warm_start=True)
    res, occ, starts, goals = run.res, run.occ, run.starts, run.goals
    replanned = np.flatnonzero(res.replans > 0)
    assert len(replanned) >= 1, "the trigger never fired"
    assert res.planned.sum() >= 90
    ok_replans = [v for v in replanned if res.replan_steps[v, 0] > 0]
    assert len(ok_replans) >= 1, "no replan produced a new plan"
    never = np.flatnonzero(res.planned & (res.replans == 0))
    assert len(never) >= 1
    for v in never:
        host = _host_track(res.paths[v], starts[v], goals[v], steps)
        assert res.steps[v] == len(host), v
        np.testing.assert_allclose(res.states[v], host, rtol=0, atol=1e-7)
    kinds = [_check_plan(occ, starts[v], goals[v], v, res.paths[v]) for v in np.flatnonzero(res.planned)]
    assert kinds.count("cr") <= 2, kinds
    for v in ok_replans:
        s = int(res.replan_steps[v, 0])  # steps taken when the replan committed
        host = _host_track(res.paths[v], starts[v], goals[v], s)
        np.testing.assert_allclose(res.states[v][:s], host[:s], rtol=0, atol=1e-7)
        start = res.last_replan_start[v]
        np.testing.assert_array_equal(start, res.states[v][s - 1][:2])  # planned from where it stood, exactly
        _check_plan(occ, start, goals[v], replan_seed(v, 0), res.last_replan_path[v])
        cont = _host_continue(res.states[v][s - 1], res.inputs[v][s - 1], res.last_replan_path[v], goals[v],
                              int(res.steps[v]) - s)
        assert len(cont) == int(res.steps[v]) - s, v
        np.testing.assert_allclose(res.states[v][s:], cont, rtol=0, atol=1e-6)
    for v in np.flatnonzero(res.phase == _lib.FLEET_GOAL):
        assert np.hypot(*(res.states[v][-1, :2] - goals[v])) < 8.0
    # not the cold run: to rounding only
    cold = _run(golden, *V100, fused=True).res
    np.testing.assert_array_equal(cold.planned, res.planned)
    both = np.flatnonzero(res.planned & (res.replans == 0) & (cold.replans == 0))
    assert len(both) >= 1
    for v in both:
        assert res.states[v].shape == cold.states[v].shape, v
        np.testing.assert_allclose(res.states[v], cold.states[v], rtol=0, atol=ATOL)
    differ = [v for v in range(V) if res.states[v].shape != cold.states[v].shape
              or not np.array_equal(res.states[v], cold.states[v])]
    print(f"{len(differ)} of {V} traces differ from the cold fused swarm's in some bit; "
          f"{len(replanned)} replanned, {len(ok_replans)} with a new plan")
    assert len(differ) >= 1, "the warm swarm reproduced the cold one bit for bit: no attempt hit"


# ---------------------------------------------------------------------- 3. the warm fleet loop, vehicle by vehicle
def _segments_against_the_warm_fleet_loop(run):
    """One warm swarm with one replan per vehicle against mpcqp_fleet_loop_warm, bit for bit: the never-replanned
    vehicles whole, the replanned ones up to their replan step on a tracker run on the swarm's own initial paths,
    and the vehicles with a new plan from there on a second tracker.  Returns how many of each it compared."""
    import torch
    from mpcqp import _lib

    res, sb, steps = run.res, run.bufs, run.steps
    V = len(res.steps)
    paths = [p if p is not None else [tuple(s)] for p, s in zip(res.paths, run.starts)]
    ft = fleet_tracker(N_HORIZON, V, 512, steps, fused=True, warm_start=True)
    ft.reset_from_plans(paths, run.starts, run.goals, max_steps=steps, device_reference=True)
    if (~res.planned).any():
        ft.buffers()["phase"][torch.from_numpy(np.flatnonzero(~res.planned)).to(ft.device)] = _lib.FLEET_ABORTED
    ft.step(steps)
    tb = snap(ft)
    ft.close()
    never = np.flatnonzero(res.planned & (res.replans == 0))
    replanned = np.flatnonzero(res.replans > 0)
    ok = [int(v) for v in replanned if res.replan_steps[v, 0] > 0]
    for v in never:
        for k in ("trace", "u_trace", "steps", "phase"):
            np.testing.assert_array_equal(sb[k][v], tb[k][v], err_msg=f"vehicle {v}: {k}")
    for v in replanned:
        s = int(res.replan_steps[v, 0])
        s = s if s > 0 else -s - 1  # a failed replan: the steps taken when it failed
        assert tb["steps"][v] >= s, v
        for k in ("trace", "u_trace"):
            np.testing.assert_array_equal(sb[k][v, :s], tb[k][v, :s], err_msg=f"vehicle {v}: {k}[:{s}]")
    if not ok:
        return len(never), len(replanned), 0
    # the continuation of every vehicle with a new plan, in one launch of a second tracker
    at = np.array([int(res.replan_steps[v, 0]) for v in ok])
    ft = fleet_tracker(N_HORIZON, len(ok), 512, steps, fused=True, warm_start=True)
    ft.reset_device(run.ref[ok], run.ref_len[ok], np.stack([sb["trace"][v, s - 1] for v, s in zip(ok, at)]),
                    run.goals[ok], max_steps=steps)
    b = ft.buffers()
    b["u_prev"][:len(ok)] = torch.from_numpy(np.stack([sb["u_trace"][v, s - 1] for v, s in zip(ok, at)])).to(ft.device)
    b["steps"][:len(ok)] = torch.from_numpy(at.astype(np.int32)).to(ft.device)
    assert (snap(ft, ("path_idx",))["path_idx"] == 0).all()
    ft.step(steps)
    cb = snap(ft)
    ft.close()
    for i, (v, s) in enumerate(zip(ok, at)):
        n = int(sb["steps"][v])
        assert n >= s and cb["steps"][i] == n, (v, s, n, cb["steps"][i])
        for k in ("trace", "u_trace"):
            np.testing.assert_array_equal(cb[k][i, s:n], sb[k][v, s:n], err_msg=f"vehicle {v}: {k}[{s}:{n}]")
        for k in ("phase", "state", "u_prev", "path_idx"):
            np.testing.assert_array_equal(cb[k][i], sb[k][v], err_msg=f"vehicle {v}: {k}")
    return len(never), len(replanned), len(ok)


def test_each_vehicle_is_the_warm_fleet_loop_segment_by_segment(cuda, golden):
    """One replan per vehicle.  A never-replanned vehicle's trace, inputs, steps and phase are those of
    mpcqp_fleet_loop_warm on the swarm's own initial paths bit for bit; a vehicle replanned at step s has that
    tracker's first s rows; and a second warm tracker, started on the vehicle's final reference from the state,
    u_prev and step count it carried over (path_idx 0), reproduces its rows after s.
    The 40-vehicle swarm at 2.5 px replans every one of its vehicles (measured: 40 of 40, all with a new plan),
    so it holds no never-replanned vehicle; the 100-vehicle swarm at 5.5 px (7 replanned, 5 with a new plan,
    93 never) is compared in the same way, and the three subsets are asserted non-empty over the two swarms."""
    V, steps, dist, _, seed = V40
    counts = np.array([_segments_against_the_warm_fleet_loop(_run(golden, V, steps, dist, 1, seed, fused=True,
                                                                  warm_start=True)),
                       _segments_against_the_warm_fleet_loop(_run(golden, *V100, fused=True, warm_start=True))])
    print(f"(never replanned, replanned, with a new plan): 40 vehicles {counts[0]}, 100 vehicles {counts[1]}")
    assert counts[0, 1] >= 1 and counts[0, 2] >= 1, counts  # the issue's swarm: replanned vehicles, new plans
    assert (counts.sum(axis=0) >= 1).all(), counts


# ---------------------------------------------------------------------- 4. paired equals unpaired
def test_paired_warm_swarm_equals_unpaired(cuda, golden):
    """V = 41 (the last wave has an absent half), two replans: pairing "on" gives the one-vehicle-per-wave warm
    swarm's results and buffers bit for bit, the launches are recorded as warm with 2 per wave ("auto" and "off":
    1).  What this swarm cannot show is a wave with one half replanned and the other not: at 2.5 px every one
    of its vehicles triggers at step 4 and uses both replans (measured: replans == 2 and a first trigger at
    step 4 for all 41), so the halves of every wave leave the triggering rounds together and apart only at
    their goals.  That wave is asserted on the 100-vehicle swarm, where it exists:
    test_paired_warm_swarm_one_half_replans_the_other_runs_on."""
    from mpcqp import _lib

    V, steps, dist, max_replans, seed = 41, V40[1], V40[2], 2, V40[4]
    runs = {p: _run(golden, V, steps, dist, max_replans, seed, fused=True, warm_start=True, pairing=p)
            for p in ("off", "on", "auto")}
    np.testing.assert_array_equal(runs["off"].starts[:40], pairs(runs["off"].occ, 40, seed)[0])
    for p in ("on", "auto"):
        _assert_same_result(runs[p].res, runs["off"].res, p)
        assert_same(runs[p].bufs, runs["off"].bufs, p, LOOP_BUFFERS_MASK)
    for p, per_wave in (("on", 2), ("auto", 1), ("off", 1)):
        want = dict(kind=_lib.LAUNCH_LOOP_WARM, name="loop_warm", per_wave=per_wave,
                    workgroups=(V + per_wave - 1) // per_wave, count=V)
        assert runs[p].info == want, (p, runs[p].info)
    res = runs["on"].res
    assert res.replans.sum() >= 1, "the trigger should fire"
    print(f"replans {res.replans.tolist()}; replan steps {res.replan_steps.tolist()}")


def test_paired_warm_swarm_one_half_replans_the_other_runs_on(cuda, golden):
    """The 100-vehicle swarm (5.5 px, one replan: 7 vehicles replanned, 93 never), warm, two per wave: the
    unpaired warm swarm's results and buffers bit for bit, and in some wave one half was replanned and the other
    was not -- it left through to_replan while the other half went on to its end in the same launch.  No
    dispatch order at this V (it is set once the vehicles outnumber the wave slots): wave w holds 2w, 2w + 1."""
    V = V100[0]
    off = _run(golden, *V100, fused=True, warm_start=True)
    on = _run(golden, *V100, fused=True, warm_start=True, pairing="on")
    assert on.info["per_wave"] == 2 and on.info["workgroups"] == V // 2 and off.info["per_wave"] == 1, (on.info, off.info)
    _assert_same_result(on.res, off.res, "on")
    assert_same(on.bufs, off.bufs, "on", LOOP_BUFFERS_MASK)
    res = on.res
    split = [w for w in range(V // 2) if res.planned[2 * w] and res.planned[2 * w + 1]
             and (res.replans[2 * w] > 0) != (res.replans[2 * w + 1] > 0)]
    print(f"waves with one half replanned and the other not: {split}")
    assert len(split) >= 1


# ---------------------------------------------------------------------- 5. the other horizons
@pytest.mark.parametrize("N", [1, 15, 16, 32])
def test_dead_trigger_is_the_warm_fleet_loop_at_every_horizon_range(cuda, golden, N):
    """max_replans = 0: the trigger is dead and each launch is exactly the warm fleet loop.  N = 1, the last
    pairable horizon, the first unpairable one and the last: the fleet buffers equal
    fleet_tracker(fused=True, warm_start=True) on the same plans bit for bit."""
    import torch
    from mpcqp import _lib
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.swarm import Swarm

    occ = golden("default_plan.npz")["occupancy"]
    V, steps = 8, 60
    starts, goals = pairs(occ, V, 3)
    sw = Swarm(occ, MPCConfig(horizon=N, sim_steps=steps), planner_params(), map_resolution=0.8, max_vehicles=V,
               device="cuda:0", max_replans=0, fused=True, warm_start=True)
    res = sw.run(starts, goals, seeds=np.arange(V))
    got = snap(sw.fleet)
    info = sw.fleet._nominal.launch_info()
    sw.fleet.close()
    assert res.planned.sum() >= 1 and (res.replans == 0).all()
    assert info["name"] == "loop_warm" and info["per_wave"] == 1 and info["count"] == V, info
    paths = [p if p is not None else [tuple(s)] for p, s in zip(res.paths, starts)]
    ft = fleet_tracker(N, V, 512, steps, fused=True, warm_start=True)
    ft.reset_from_plans(paths, starts, goals, max_steps=steps, device_reference=True)
    if (~res.planned).any():
        ft.buffers()["phase"][torch.from_numpy(np.flatnonzero(~res.planned)).to(ft.device)] = _lib.FLEET_ABORTED
    ft.step(steps)
    want = snap(ft)
    ft.close()
    assert (want["steps"][res.planned] > 1).any(), want["steps"]  # steps beyond the cold first one were run
    assert_same(got, want, f"N={N}", LOOP_BUFFERS_MASK)


# ---------------------------------------------------------------------- 6. sharded
def test_sharded_warm_swarm_equals_one_warm_swarm(cuda, golden):
    """test_sharded_swarm_equals_one_swarm, warm: 40 vehicles in three emulated ranks, each on its own
    Swarm; the merged result equals the one warm swarm exactly, with the trigger live."""
    from mpcqp.pipeline.swarm import merge_swarm_results, run_swarm_sharded, shard_vehicles

    V, steps, dist, max_replans, seed = V40
    world = 3
    one = _run(golden, *V40, fused=True, warm_start=True)
    parts = []
    for r in range(world):
        lo, hi = shard_vehicles(V, world, r)
        sw = swarm(one.occ, hi - lo, steps, replan_distance=dist, max_replans=max_replans, fused=True, warm_start=True)
        p = run_swarm_sharded(sw.run, one.starts, one.goals, np.arange(V), rank=r, world=world,
                              all_gather_object=lambda out, obj, r=r: out.__setitem__(r, obj))
        sw.fleet.close()
        assert len(p.steps) == hi - lo
        parts.append(p)
    got = merge_swarm_results(parts)
    assert one.res.replans.sum() >= 1, "the trigger should fire at 2.5 px"
    _assert_same_result(got, one.res, "sharded")


# ---------------------------------------------------------------------- 7. refusals write nothing
@pytest.mark.parametrize("how", ["n40", "reproducible"])
def test_refused_warm_swarm_call_writes_nothing(cuda, golden, how):
    """Parameter blocks without the fused one-wave loop: MPCQP_E_HORIZON, no silent cold fallback -- every fleet
    buffer and the swarm's replans / start_goal are as they were, and a build made on each workspace before the
    call still solves."""
    import torch
    from mpcqp import scenarios
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.swarm import Swarm

    occ = golden("default_plan.npz")["occupancy"]
    N = 40 if how == "n40" else N_HORIZON
    V, steps = 4, 12
    starts, goals = pairs(occ, V, 3)
    settings = dict(reproducible=1) if how == "reproducible" else {}
    sw = Swarm(occ, MPCConfig(horizon=N, sim_steps=steps), planner_params(), map_resolution=0.8, max_vehicles=V,
               device="cuda:0", max_replans=1, replan_distance=2.5, fused=True, warm_start=True, **settings)
    ft = sw.fleet
    paths = [[tuple(s), tuple(g)] for s, g in zip(starts, goals)]  # a straight line each: the call never runs them
    ft.reset_from_plans(paths, starts, goals, max_steps=steps, device_reference=True)
    st, sbufs = sw._swarm_struct(V, np.arange(V), np.ones(V, dtype=bool))
    batch = scenarios.config3(V, horizon=N, seed=9)
    for ctrl in (ft._nominal, ft._relaxed):  # a build on each workspace, from before the call
        ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev)
    ft.buffers()["status"].fill_(77)
    sbufs["start_goal"].fill_(77.0)
    before = snap(ft)
    s = ctypes.c_void_p(torch.cuda.current_stream(ft.device).cuda_stream)
    rc = ft._L.mpcqp_swarm_loop_warm(ft._nominal._ws, ft._relaxed._ws, ctypes.byref(ft._fleet), ctypes.byref(st), 8, s)
    assert rc == E_HORIZON, (how, rc, ft._L.mpcqp_last_error())
    assert b"mpcqp_swarm_loop_warm" in ft._L.mpcqp_last_error()
    assert_same(snap(ft), before, how, LOOP_BUFFERS_MASK)
    assert (before["status"] == 77).all() and (before["steps"] == 0).all()
    assert bool((sbufs["start_goal"] == 77.0).all()) and bool((sbufs["replans"] == 0).all())
    for ctrl in (ft._nominal, ft._relaxed):  # both builds are still valid
        assert ctrl._L.mpcqp_solve(ctrl._ws, V, None, None, None, ctrl._status.data_ptr(), None, None, s) == 0
    torch.cuda.synchronize()
    ft.close()
