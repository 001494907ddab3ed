"""GPU tests of the swarm on a changing map (``mpcqp_swarm_loop_map``, ``mpcqp_swarm_run_map``,
``k_swarm_loop_map<N>``, ``Swarm(grids=...)``): grids by epoch, the blocked-path replan trigger and the
replanning on the grid of the moment.

The grid is the default inflated one (an open room with a block in the middle); the closed map shuts the
passage above the block.  With one grid and no lookahead the map calls are the plain swarm bit for bit; on
the closing map the fused call equals the stepped one bit for bit, the trigger's decisions are replayed on
the host from the device's own references and traces (numpy only), every new plan is the reference
planner's on the grid the vehicle triggered on, vehicles that never trigger are untouched by the map, and a
refused call writes nothing.  Every swarm run is made once per configuration and shared by the tests that
read it; nothing mutates a shared run."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
from gpu_helpers import (E_ARG, LOOP_BUFFERS_MASK, SWARM_HORIZON as N_HORIZON, assert_same, oracle_plan, pairs,
                         planner_params, snap, swarm)

pytestmark = pytest.mark.gpu

V40 = (40, 200, 2.5, 2, 21)  # test_fused_swarm_equals_stepped_swarm's: V, steps, replan distance, max_replans, pair seed
V, STEPS, LOOK = 16, 120, 20  # the closing-passage swarm: pairs(occ, 16, 7), seeds 0..15
RESULT_ARRAYS = ("phase", "steps", "replans", "planned", "replan_steps", "last_replan_start", "replan_over_capacity")
RESULT_LISTS = ("states", "inputs", "paths", "last_replan_path")
MAP_ARRAYS = ("replan_cause", "replan_grid", "hits")

_RUNS: dict = {}


def _grids(golden, which):
    """"static": the grid alone; "closing": the passage above the block closes; "reopen": and opens again."""
    occ = golden("default_plan.npz")["occupancy"]
    if which is None:
        return occ, None
    g1 = occ.copy()
    g1[2:34, 36:41] = 0
    return occ, {"static": occ[None], "closing": np.stack([occ, g1]), "reopen": np.stack([occ, g1, occ])}[which]


def _run(golden, which, cfg, vehicles=None, **kw):
    """One Swarm.run (cached) of cfg = (V, steps, replan distance, max_replans, pair seed) on the named map
    (None: no grids, the plain swarm), optionally of a subset of the vehicles with their own seeds: the result,
    the fleet's buffers afterwards, the references as they were before the first launch, grid_of and the launch
    record."""
    key = (which, cfg, vehicles, tuple(sorted(kw.items())))
    if key not in _RUNS:
        n, steps, dist, max_replans, seed = cfg
        occ, grids = _grids(golden, which)
        starts, goals = pairs(occ, n, seed)
        idx = np.arange(n) if vehicles is None else np.asarray(vehicles)
        if grids is not None:
            kw = dict(kw, grids=grids)
        sw = swarm(occ, len(idx), steps, replan_distance=dist, max_replans=max_replans, **kw)
        ref = {}

        def copy_refs(fb):
            ref["rows"] = fb["ref_global"][:len(idx)].cpu().numpy().copy()
            ref["len"] = fb["ref_len"][:len(idx)].cpu().numpy().copy()

        res = sw.run(starts[idx], goals[idx], seeds=idx, before_launch=copy_refs)
        grid_of = None if grids is None else sw._map_buffers["grid_of"][:len(idx)].cpu().numpy().copy()
        _RUNS[key] = SimpleNamespace(res=res, bufs=snap(sw.fleet), ref0=ref["rows"], len0=ref["len"], grid_of=grid_of,
                                     info=sw.fleet._nominal.launch_info(), occ=occ, grids=grids, idx=idx,
                                     starts=starts[idx], goals=goals[idx], steps=steps,
                                     epoch=kw.get("epoch_steps", 1), look=kw.get("lookahead", LOOK))
        sw.fleet.close()
    return _RUNS[key]


def _assert_same_result(a, b, what, names=RESULT_ARRAYS):
    """The named SwarmResult arrays and every per-vehicle list, bit for bit."""
    for k in names:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what}: {k}")
    for k in RESULT_LISTS:
        la, lb = getattr(a, k), getattr(b, k)
        assert len(la) == len(lb), (what, k)
        for v, (x, y) in enumerate(zip(la, lb)):
            assert (x is None) == (y is None), (what, k, v)
            if x is not None:
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=f"{what}: {k}[{v}]")


def _check_plan(occ, start, goal, seed, path, tol=1e-4):
    """The device plan against the host restatement of the reference planner on `occ`: "libm" or "cr" (the plan
    with correctly rounded steer trig, rare); test_gpu_swarm.py's checker and tolerance."""
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


def _replan_step(res, v):
    """steps[v] at the vehicle's first replan (None: it never replanned)."""
    if res.replans[v] == 0:
        return None
    rs = int(res.replan_steps[v, 0])
    return rs if rs >= 0 else -rs - 1


# ---------------------------------------------------------------------- 1. nothing changes
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stepped"])
def test_one_grid_without_lookahead_is_the_plain_swarm(cuda, golden, fused):
    """grids = occ[None], lookahead 0: mpcqp_swarm_loop_map equals mpcqp_swarm_loop and mpcqp_swarm_run_map equals
    mpcqp_swarm_run bit for bit -- states, inputs, phase, steps, replans, replan steps, replan starts, new plans
    and every fleet buffer -- with the off-track trigger firing."""
    from mpcqp import _lib

    plain = _run(golden, None, V40, fused=fused)
    on_map = _run(golden, "static", V40, fused=fused, lookahead=0)
    assert plain.res.replans.sum() > 0, "the trigger should fire"
    _assert_same_result(on_map.res, plain.res, f"fused={fused}")
    assert_same(on_map.bufs, plain.bufs, f"fused={fused}", LOOP_BUFFERS_MASK)
    res = on_map.res
    used = np.arange(res.replan_cause.shape[1])[None, :] < res.replans[:, None]
    assert np.isin(res.replan_cause[used], [_lib.REPLAN_ABORTED, _lib.REPLAN_OFF_TRACK]).all()
    assert (res.replan_cause[~used] == 0).all() and (res.replan_grid[used] == 0).all()
    if fused:
        assert on_map.info["name"] == "loop_map" and on_map.info["per_wave"] == 1, on_map.info
        assert plain.info["name"] == "loop", plain.info


# ---------------------------------------------------------------------- 2. fused against stepped
CLOSING = (V, STEPS, 1e9, 1, 7)
CLOSING_TWO = (V, STEPS, 5.5, 2, 7)


@pytest.mark.parametrize("cfg", [CLOSING, CLOSING_TWO], ids=["one_replan", "two_replans_5.5px"])
def test_fused_map_swarm_equals_stepped_map_swarm(cuda, golden, cfg):
    """The closing passage: mpcqp_swarm_loop_map equals mpcqp_swarm_run_map to the end bit for bit, replan_cause
    and grid_of included, with blocked vehicles and at least one new plan."""
    from mpcqp import _lib

    a = _run(golden, "closing", cfg, fused=False, epoch_steps=10, lookahead=LOOK)
    b = _run(golden, "closing", cfg, fused=True, epoch_steps=10, lookahead=LOOK)
    _assert_same_result(b.res, a.res, str(cfg), RESULT_ARRAYS + MAP_ARRAYS)
    np.testing.assert_array_equal(b.grid_of, a.grid_of)
    assert_same(b.bufs, a.bufs, str(cfg), tuple(k for k in LOOP_BUFFERS_MASK if k != "mask"))
    res = b.res
    print("causes", res.replan_cause.tolist(), "replan steps", res.replan_steps.tolist(), "hits", res.hits.tolist())
    assert (res.replan_cause == _lib.REPLAN_BLOCKED).sum() >= 1, "no vehicle was blocked"
    assert (res.replan_steps > 0).sum() >= 1, "no replan produced a new plan"
    assert b.info["name"] == "loop_map" and b.info["per_wave"] == 1, b.info


# ---------------------------------------------------------------------- 3. host replay
def _blocked(ref, n, pidx, grid, look):
    """The blocked test of include/mpcqp.h on the host: rows min(pidx + j, n - 1), j < look, the planner's lookup."""
    H, W = grid.shape
    r = np.minimum(pidx + np.arange(look), n - 1)
    xi = np.clip(np.rint(ref[r, 0]), 0, W - 1).astype(np.int64)
    yi = np.clip(np.rint(ref[r, 1]), 0, H - 1).astype(np.int64)
    return bool((grid[yi, xi] == 0).any())


def _replay(run):
    """Every planned vehicle of a one-replan run without the off-track test: path_idx replayed from its trace by
    the loop's own rule on the references the device held before the launch, the blocked test after every step.
    False at every tested step before the recorded replan step (at every one if there was none), true at the
    replan step of a blocked vehicle, whose grid_of is the grid of that step.  Returns the blocked vehicles."""
    from mpcqp import _lib

    res, T = run.res, len(run.grids)
    blocked = []
    for v in np.flatnonzero(res.planned):
        ref, n, st = run.ref0[v], int(run.len0[v]), res.states[v]
        s = _replan_step(res, v)
        cause = int(res.replan_cause[v, 0])
        assert cause in ((0,) if s is None else (_lib.REPLAN_ABORTED, _lib.REPLAN_BLOCKED)), (v, cause)
        last = len(st) if s is None else s
        pidx = 0
        for k in range(1, last + 1):
            x, y = st[k - 1, 0], st[k - 1, 1]
            if pidx < n - 2:
                dx, dy = x - ref[pidx, 0], y - ref[pidx, 1]
                if dx * dx + dy * dy > 25.0:
                    pidx += 1
            if s is None and k == len(st) and res.phase[v] in (_lib.FLEET_GOAL, _lib.FLEET_OUT_OF_STEPS):
                break  # the step that ended the run: the loop leaves before the trigger
            g = min(k // run.epoch, T - 1)
            hit = _blocked(ref, n, pidx, run.grids[g], run.look)
            if k == s and cause == _lib.REPLAN_BLOCKED:
                assert hit, f"vehicle {v}: recorded as blocked after step {k} (path_idx {pidx}), the replay says free"
                assert run.grid_of[v] == g and res.replan_grid[v, 0] == g, (v, run.grid_of[v], g)
                blocked.append(int(v))
            else:
                assert not hit, f"vehicle {v}: blocked after step {k} (path_idx {pidx}, grid {g}), recorded {s}"
    return blocked


def test_blocked_trigger_replayed_on_the_host(cuda, golden):
    run = _run(golden, "closing", CLOSING, fused=True, epoch_steps=10, lookahead=LOOK)
    blocked = _replay(run)
    print("blocked vehicles", blocked, "at steps", [_replan_step(run.res, v) for v in blocked])
    assert len(blocked) >= 1
    assert (run.res.replan_cause != 2).all()  # no off-track replans at 1e9 px


# ---------------------------------------------------------------------- 4. plans
def test_replans_are_the_reference_planner_on_the_vehicle_s_grid(cuda, golden):
    """Every new plan is the reference planner's plan on grids[grid_of] from exactly where the vehicle stood at its
    replan step, with its replan seed."""
    from mpcqp.pipeline.swarm import replan_seed

    run = _run(golden, "closing", CLOSING, fused=True, epoch_steps=10, lookahead=LOOK)
    res = run.res
    ok = [v for v in range(V) if res.replans[v] and res.replan_steps[v, 0] > 0]
    assert 1 <= len(ok) <= 4, ok
    for v in ok:
        s = int(res.replan_steps[v, 0])
        start = res.last_replan_start[v]
        np.testing.assert_array_equal(start, res.states[v][s - 1][:2])
        _check_plan(run.grids[run.grid_of[v]], start, run.goals[v], replan_seed(int(run.idx[v]), 0),
                    res.last_replan_path[v])


# ---------------------------------------------------------------------- 5. independence
def test_vehicles_that_never_trigger_equal_the_plain_fused_swarm(cuda, golden):
    run = _run(golden, "closing", CLOSING, fused=True, epoch_steps=10, lookahead=LOOK)
    plain = _run(golden, None, CLOSING, fused=True)
    never = np.flatnonzero(run.res.planned & (run.res.replans == 0))
    assert len(never) >= 1 and (plain.res.replans[never] == 0).all()
    for v in never:
        np.testing.assert_array_equal(run.res.states[v], plain.res.states[v], err_msg=str(v))
        np.testing.assert_array_equal(run.res.inputs[v], plain.res.inputs[v], err_msg=str(v))
        assert run.res.phase[v] == plain.res.phase[v] and run.res.steps[v] == plain.res.steps[v], v
        for k in ("state", "u_prev", "path_idx", "status", "u0", "X"):
            a, b = (r.bufs[k][:, v] if k in ("status", "u0") else r.bufs[k][v] for r in (run, plain))
            np.testing.assert_array_equal(a, b, err_msg=f"{k}[{v}]")


# ---------------------------------------------------------------------- 6. clamp and reopening
def test_reopening_map_clamps_to_the_last_grid(cuda, golden):
    kw = dict(epoch_steps=8, lookahead=LOOK)
    a = _run(golden, "reopen", CLOSING, fused=False, **kw)
    b = _run(golden, "reopen", CLOSING, fused=True, **kw)
    _assert_same_result(b.res, a.res, "reopen", RESULT_ARRAYS + MAP_ARRAYS)
    np.testing.assert_array_equal(b.grid_of, a.grid_of)
    assert (b.grid_of >= 0).all() and (b.grid_of <= 2).all(), b.grid_of
    assert (b.res.replan_grid <= 2).all()
    _replay(b)


# ---------------------------------------------------------------------- 7. fallback
def test_reproducible_blocks_fall_back_to_the_stepped_map_swarm(cuda, golden):
    """reproducible = 1 has no fused one-wave loop: mpcqp_swarm_loop_map runs mpcqp_swarm_run_map(max_steps, graph)."""
    kw = dict(vehicles=(4, 7, 8, 14), epoch_steps=10, lookahead=LOOK, reproducible=1)
    a = _run(golden, "closing", CLOSING, fused=False, **kw)
    b = _run(golden, "closing", CLOSING, fused=True, **kw)
    _assert_same_result(b.res, a.res, "reproducible", RESULT_ARRAYS + MAP_ARRAYS)
    np.testing.assert_array_equal(b.grid_of, a.grid_of)
    assert_same(b.bufs, a.bufs, "reproducible", tuple(k for k in LOOP_BUFFERS_MASK if k != "mask"))
    assert b.info["name"] == "none", b.info  # the stepped swarm records no launch
    assert b.res.steps.sum() > 0


# ---------------------------------------------------------------------- 8. sharding
def test_sharded_map_swarm_equals_one_map_swarm(cuda, golden):
    from mpcqp.pipeline.swarm import merge_swarm_results, run_swarm_sharded, shard_vehicles

    one = _run(golden, "closing", CLOSING, fused=True, epoch_steps=10, lookahead=LOOK)
    occ, grids = _grids(golden, "closing")
    starts, goals = pairs(occ, V, CLOSING[4])
    world, parts = 3, []
    for r in range(world):
        lo, hi = shard_vehicles(V, world, r)
        sw = swarm(occ, hi - lo, STEPS, replan_distance=CLOSING[2], max_replans=CLOSING[3], fused=True, grids=grids,
                   epoch_steps=10, lookahead=LOOK)
        parts.append(run_swarm_sharded(sw.run, starts, goals, np.arange(V), rank=r, world=world,
                                       all_gather_object=lambda out, obj, r=r: out.__setitem__(r, obj)))
        sw.fleet.close()
        assert len(parts[-1].steps) == hi - lo
    got = merge_swarm_results(parts)
    _assert_same_result(got, one.res, "sharded", RESULT_ARRAYS + MAP_ARRAYS)


# ---------------------------------------------------------------------- 9. refusals write nothing
def test_refused_map_calls_write_nothing(cuda, golden):
    """Each MPCQP_E_ARG case of the map struct, on both calls: every fleet and swarm buffer is as it was."""
    import torch
    from mpcqp import _lib

    occ, grids = _grids(golden, "closing")
    n, steps = 4, 12
    starts, goals = pairs(occ, n, 3)
    sw = swarm(occ, n, steps, max_replans=1, replan_distance=2.5, fused=True, grids=grids, epoch_steps=10)
    ft = sw.fleet
    paths = [[tuple(s), tuple(g)] for s, g in zip(starts, goals)]  # a straight line each: no call runs them
    ft.reset_from_plans(paths, starts, goals, max_steps=steps, device_reference=True)
    st, sbufs = sw._swarm_struct(n, np.arange(n), np.ones(n, dtype=bool))
    st.occupancy = None  # not read by the map calls
    good, mbufs = sw._map_struct(n)
    ft.buffers()["status"].fill_(77)
    for k in ("start_goal", "replan_step", "count", "new_len"):
        sbufs[k].fill_(77)
    mbufs["grid_of"].fill_(77)
    mbufs["replan_cause"].fill_(77)
    before = snap(ft)

    def variant(**fields):
        m = _lib.MpcqpSwarmMap()
        ctypes.memmove(ctypes.byref(m), ctypes.byref(good), ctypes.sizeof(m))
        for k, v in fields.items():
            setattr(m, k, v)
        return ctypes.byref(m)

    bad = {"null map": None, "num_grids": variant(num_grids=0), "epoch_steps": variant(epoch_steps=0),
           "lookahead -1": variant(lookahead=-1), "lookahead 65": variant(lookahead=65),
           "grids": variant(grids=None), "grid_of": variant(grid_of=None)}
    s = ctypes.c_void_p(torch.cuda.current_stream(ft.device).cuda_stream)
    head = (ft._nominal._ws, ft._relaxed._ws, ctypes.byref(ft._fleet), ctypes.byref(st))
    for what, m in bad.items():
        assert ft._L.mpcqp_swarm_loop_map(*head, m, s) == E_ARG, (what, ft._L.mpcqp_last_error())
        assert ft._L.mpcqp_swarm_run_map(*head, m, steps, 1, s) == E_ARG, (what, ft._L.mpcqp_last_error())
        assert ft._L.mpcqp_swarm_run_map(*head, m, steps, 0, s) == E_ARG, (what, ft._L.mpcqp_last_error())
    assert_same(snap(ft), before, "refused", LOOP_BUFFERS_MASK)
    assert (before["status"] == 77).all() and (before["steps"] == 0).all()
    for k in ("start_goal", "replan_step", "count", "new_len"):
        assert bool((sbufs[k] == 77).all()), k
    assert bool((sbufs["replans"] == 0).all())
    assert bool((mbufs["grid_of"] == 77).all()) and bool((mbufs["replan_cause"] == 77).all())
    assert ft._nominal.launch_info()["name"] == "none"
    ft.close()
