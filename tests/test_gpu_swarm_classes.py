"""GPU tests of the parameter classes in the fused swarm (``mpcqp_swarm_loop_mixed``, ``mpcqp_swarm_loop_mixed_warm``,
``k_swarm_loop_mixed<N>`` / ``k_swarm_loop_mixed_warm<N>``, ``Swarm.set_classes`` / ``run(classes=)``): mixed fleets
that replan.

The claim: vehicle v of a mixed swarm gets, bit for bit, the results, buffers and final reference of a
homogeneous fused swarm under its class's two blocks, cold (``mpcqp_swarm_loop``) and warm
(``mpcqp_swarm_loop_warm``, one vehicle per wave) -- so every comparison with a homogeneous run is
``assert_array_equal``.  The swarms are the ones test_gpu_swarm.py fires the trigger on; the classes are four
blocks at resolution 0.8 with one dt; ``cls[v] = v % 4``.  Against the oracle's loop the states agree to
``ATOL``.  Every swarm run is made once per configuration and shared by the tests that read it; nothing
mutates a shared run."""
from __future__ import annotations

import ctypes
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
from gpu_helpers import (ATOL, BAD_CLASS, E_ARG, E_HORIZON, E_STATE, FAIL_NOMINAL, LOOP_BUFFERS_MASK,
                         SWARM_HORIZON as N_HORIZON, TWO_SLOT, assert_same, base_params, fleet_tracker,
                         oracle_variant_params, pairs, planner_params, snap, swarm)
from param_variants import variant

pytestmark = pytest.mark.gpu

# V, steps, replan distance (px), max_replans, seed of the (start, goal) pairs: test_gpu_swarm.py's
V40 = (40, 200, 2.5, 2, 21)
V100 = (100, 150, 5.5, 1, 7)
RESULT_ARRAYS = ("phase", "steps", "replans", "planned", "replan_steps", "last_replan_start", "replan_over_capacity")
RESULT_LISTS = ("states", "inputs", "paths", "last_replan_path")
NAMES = ("default", "tight_bounds", "q_nondiag", "wheelbase_14")  # the four classes


def blocks(N=N_HORIZON):
    base = base_params(N)
    return [base, variant(base, "tight_bounds"), variant(base, "q_nondiag"), dataclasses.replace(base, wheelbase_px=14.0)]


_RUNS: dict = {}


def _run(golden, cfg, idx=None, block=None, table=None, **kw):
    """One Swarm.run (cached).  ``idx``: the vehicles of the configuration that run (their own starts, goals and
    seeds; None: all).  ``block``: the homogeneous swarm under blocks()[block].  ``table``: a mixed swarm under
    the first ``table`` blocks, vehicle v (of the whole configuration) in class v % table."""
    V, steps, dist, max_replans, seed = cfg
    idx = np.arange(V) if idx is None else np.asarray(idx)
    key = (cfg, tuple(idx.tolist()), block, table, tuple(sorted(kw.items())))
    if key not in _RUNS:
        occ = golden("default_plan.npz")["occupancy"]
        starts, goals = pairs(occ, V, seed)
        if block is not None:
            kw = dict(kw, params=blocks()[block])
        sw = swarm(occ, len(idx), steps, replan_distance=dist, max_replans=max_replans, **kw)
        more = {}
        if table:
            sw.set_classes(blocks()[:table])
            more["classes"] = (idx % table).astype(np.int64)
        res = sw.run(starts[idx], goals[idx], seeds=idx, **more)
        b = sw.fleet.buffers()
        n = len(idx)
        _RUNS[key] = SimpleNamespace(res=res, bufs=snap(sw.fleet), ref=b["ref_global"][:n].cpu().numpy().copy(),
                                     ref_len=b["ref_len"][:n].cpu().numpy().copy(),
                                     info=sw.fleet._nominal.launch_info(), occ=occ, starts=starts[idx],
                                     goals=goals[idx], steps=steps, idx=idx)
        sw.fleet.close()
    return _RUNS[key]


def _rows(bufs, idx):
    return {k: (a[:, idx] if k in TWO_SLOT else a[idx]) for k, a in bufs.items()}


def _assert_same_result(a, b, what, ia=None, ib=None):
    """Every SwarmResult field but the timings, bit for bit (vehicles ``ia`` of a against ``ib`` of b)."""
    n = len(a.steps)
    ia = np.arange(n) if ia is None else np.asarray(ia)
    ib = np.arange(len(b.steps)) if ib is None else np.asarray(ib)
    assert len(ia) == len(ib), what
    for k in RESULT_ARRAYS:
        np.testing.assert_array_equal(getattr(a, k)[ia], getattr(b, k)[ib], err_msg=f"{what}: {k}")
    for k in RESULT_LISTS:
        la, lb = getattr(a, k), getattr(b, k)
        for i, j in zip(ia, ib):
            x, y = la[i], lb[j]
            assert (x is None) == (y is None), (what, k, i)
            if x is not None:
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=f"{what}: {k}[{i}]")


def _assert_same_refs(a, b, lens, what):
    """The reference rows below ref_len, vehicle by vehicle (equal lengths asserted by the caller).  The rows from
    ref_len on are unused and never initialised: build_reference_batch hands out torch.empty memory."""
    for v, n in enumerate(lens):
        np.testing.assert_array_equal(a[v, :n], b[v, :n], err_msg=f"{what}: ref_global[{v}, :{n}]")


def _assert_same_rows(mixed, idx, homo, what):
    """Vehicles ``idx`` of the mixed run against the whole homogeneous run: results, buffers, final references."""
    _assert_same_result(mixed.res, homo.res, what, ia=idx)
    assert_same(_rows(mixed.bufs, idx), homo.bufs, what, LOOP_BUFFERS_MASK)
    np.testing.assert_array_equal(mixed.ref_len[idx], homo.ref_len, err_msg=f"{what}: ref_len")
    _assert_same_refs(mixed.ref[idx], homo.ref, homo.ref_len, what)


def _against_sub_swarms(golden, cfg, **kw):
    """The mixed run of the configuration against its four homogeneous sub-swarms; returns (mixed, sub-swarms)."""
    V = cfg[0]
    mixed = _run(golden, cfg, table=4, fused=True, **kw)
    subs = []
    for c in range(4):
        idx = np.flatnonzero(np.arange(V) % 4 == c)
        homo = _run(golden, cfg, idx=idx, block=c, fused=True, **kw)
        _assert_same_rows(mixed, idx, homo, f"class {c} ({NAMES[c]})")
        subs.append(homo)
    return mixed, subs


def _not_vacuous(golden, cfg, subs, **kw):
    """The conditions on the homogeneous runs that keep the comparison from passing vacuously."""
    V = cfg[0]
    res = [s.res for s in subs]
    replanned = [int((r.replans > 0).sum()) for r in res]
    never = [int((r.planned & (r.replans == 0)).sum()) for r in res]
    # the same vehicles under block 0: one extra homogeneous run (the whole swarm under the default block)
    zero = _run(golden, cfg, block=0, fused=True, **kw)
    differ = [c for c in range(1, 4) if not np.array_equal(subs[c].bufs["trace"], zero.bufs["trace"][subs[c].idx])]
    print(f"V = {V}: replanned per class {replanned}, never replanned {never}, classes whose traces differ from "
          f"block 0's on the same vehicles {differ}")
    assert len(differ) >= 2, differ
    return replanned, never


# ---------------------------------------------------------------------- 1. mixed equals the sub-swarms, cold
@pytest.mark.parametrize("cfg", [V40, V100], ids=["v40", "v100"])
def test_mixed_swarm_equals_the_homogeneous_sub_swarms(cuda, golden, cfg):
    """Cold.  Every SwarmResult field but the timings, every fleet buffer and the final reference rows of the
    vehicles of class c equal the homogeneous fused swarm's under block c on those vehicles, their seeds kept."""
    mixed, subs = _against_sub_swarms(golden, cfg)
    replanned, never = _not_vacuous(golden, cfg, subs)
    assert mixed.info["name"] == "loop_mixed" and mixed.info["per_wave"] == 1 and mixed.info["count"] == cfg[0], mixed.info
    if cfg is V40:
        assert sum(n > 0 for n in replanned) >= 2, replanned  # vehicles replanned in two classes at least
    else:
        assert sum(never) >= 1 and sum(replanned) >= 1, (never, replanned)


# ---------------------------------------------------------------------- 2. the same, warm
@pytest.mark.parametrize("cfg", [V40, V100], ids=["v40", "v100"])
def test_warm_mixed_swarm_equals_the_warm_homogeneous_sub_swarms(cuda, golden, cfg):
    """warm_start=True with the default passes against the warm homogeneous sub-swarms (one vehicle per wave);
    with guess_passes = 0 the warm mixed swarm is the cold mixed one; the launches are recorded as what they are."""
    from mpcqp import _lib

    V = cfg[0]
    mixed, subs = _against_sub_swarms(golden, cfg, warm_start=True)
    _not_vacuous(golden, cfg, subs, warm_start=True)
    assert all(s.info["name"] == "loop_warm" and s.info["per_wave"] == 1 for s in subs), [s.info for s in subs]
    cold = _run(golden, cfg, table=4, fused=True)
    none = _run(golden, cfg, table=4, fused=True, warm_start=True, guess_passes=0)
    _assert_same_result(none.res, cold.res, "guess_passes = 0")
    assert_same(none.bufs, cold.bufs, "guess_passes = 0", LOOP_BUFFERS_MASK)
    np.testing.assert_array_equal(none.ref_len, cold.ref_len)
    _assert_same_refs(none.ref, cold.ref, cold.ref_len, "guess_passes = 0")
    assert cold.info == dict(kind=_lib.LAUNCH_LOOP_MIXED, name="loop_mixed", per_wave=1, workgroups=V, count=V), cold.info
    for r in (mixed, none):
        assert r.info == dict(kind=_lib.LAUNCH_LOOP_MIXED_WARM, name="loop_mixed_warm", per_wave=1, workgroups=V,
                              count=V), r.info


# ---------------------------------------------------------------------- 3. dead trigger: the mixed fleet loops
@pytest.mark.parametrize("N", [1, 15, 16, 32])
def test_dead_trigger_is_the_mixed_fleet_loop_cold_and_warm(cuda, golden, N):
    """max_replans = 0, two classes.  Cold: the buffers of FleetTracker.set_classes' mpcqp_fleet_loop_mixed on the
    same plans.  Warm: those of the per-class homogeneous warm fleet loops -- the warm mixed fleet loop."""
    import torch
    from mpcqp import _lib
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.swarm import Swarm

    occ = golden("default_plan.npz")["occupancy"]
    V, steps = 8, 60
    starts, goals = pairs(occ, V, 3)
    base = base_params(N)
    two = [base, dataclasses.replace(base, wheelbase_px=14.0)]
    cls = np.arange(V) % 2

    def mixed_swarm(**kw):
        sw = Swarm(occ, MPCConfig(horizon=N, sim_steps=steps), planner_params(), map_resolution=0.8, max_vehicles=V,
                   device="cuda:0", max_replans=0, fused=True, **kw)
        sw.set_classes(two)
        res = sw.run(starts, goals, seeds=np.arange(V), classes=cls)
        got, info = snap(sw.fleet), sw.fleet._nominal.launch_info()
        sw.fleet.close()
        assert res.planned.sum() >= 1 and (res.replans == 0).all()
        assert info["per_wave"] == 1 and info["count"] == V, info
        return res, got, info

    def load(ft, res, idx, **kw):
        paths = [res.paths[v] if res.paths[v] is not None else [tuple(starts[v])] for v in idx]
        ft.reset_from_plans(paths, starts[idx], goals[idx], max_steps=steps, device_reference=True, **kw)
        lost = np.flatnonzero(~res.planned[idx])
        if len(lost):
            ft.buffers()["phase"][torch.from_numpy(lost).to(ft.device)] = _lib.FLEET_ABORTED

    res, got, info = mixed_swarm()
    assert info["name"] == "loop_mixed", info
    ft = fleet_tracker(N, V, 512, steps, fused=True)
    ft.set_classes(two)
    load(ft, res, np.arange(V), classes=cls)
    ft.step(steps)
    want = snap(ft)
    ft.close()
    assert (want["steps"][res.planned] > 1).any(), want["steps"]
    assert_same(got, want, f"N={N} cold", LOOP_BUFFERS_MASK)

    wres, wgot, info = mixed_swarm(warm_start=True)
    assert info["name"] == "loop_mixed_warm", info
    np.testing.assert_array_equal(wres.planned, res.planned)
    for c in range(2):
        idx = np.flatnonzero(cls == c)
        ft = fleet_tracker(N, len(idx), 512, steps, fused=True, warm_start=True, params=two[c])
        load(ft, wres, idx)
        ft.step(steps)
        want = snap(ft)
        ft.close()
        assert_same(_rows(wgot, idx), want, f"N={N} warm class {c}", LOOP_BUFFERS_MASK)
    assert (wgot["steps"][wres.planned] > 1).any(), wgot["steps"]


# ---------------------------------------------------------------------- 4. one class is the plain swarm
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_one_class_equals_the_plain_swarm(cuda, golden, warm):
    """K = 1 with the default block, no classes= (every vehicle class 0), against the plain fused swarm at one
    vehicle per wave."""
    kw = dict(warm_start=True) if warm else {}
    one = _run(golden, V40, table=1, fused=True, **kw)
    plain = _run(golden, V40, fused=True, pairing="off", **kw)
    assert plain.res.replans.sum() > 0, "the trigger should fire"
    assert plain.info["name"] == ("loop_warm" if warm else "loop") and plain.info["per_wave"] == 1, plain.info
    assert one.info["name"] == ("loop_mixed_warm" if warm else "loop_mixed"), one.info
    _assert_same_rows(one, np.arange(V40[0]), plain, "K = 1")


# ---------------------------------------------------------------------- 5. the abort path, per class
def test_abort_path_per_class(cuda, golden):
    """Distance 0 (only an abort triggers), two replans.  Class 1's settings fail every QP, nominal and retry:
    its vehicles abort at their first step, are replanned, abort again, and end ABORTED with both replans used.
    They equal a homogeneous swarm built with the same failing settings; class 0 equals its plain sub-swarm."""
    from mpcqp import _lib

    occ = golden("default_plan.npz")["occupancy"]
    V, steps = 12, 40
    starts, goals = pairs(occ, V, V40[4])
    base = base_params(N_HORIZON)
    two = [base, dataclasses.replace(base, wheelbase_px=14.0)]
    cls = np.arange(V) % 2
    kw = dict(replan_distance=0.0, max_replans=2, fused=True)

    def run(sw, idx, **more):
        res = sw.run(starts[idx], goals[idx], seeds=idx, **more)
        b = sw.fleet.buffers()
        out = SimpleNamespace(res=res, bufs=snap(sw.fleet), ref=b["ref_global"][:len(idx)].cpu().numpy().copy(),
                              ref_len=b["ref_len"][:len(idx)].cpu().numpy().copy())
        sw.fleet.close()
        return out

    sw = swarm(occ, V, steps, **kw)
    sw.set_classes(two, settings=[{}, FAIL_NOMINAL], relaxed_settings=[{}, FAIL_NOMINAL])
    mixed = run(sw, np.arange(V), classes=cls)
    i0, i1 = np.flatnonzero(cls == 0), np.flatnonzero(cls == 1)
    res = mixed.res
    print(f"planned {res.planned.tolist()}, phase {res.phase.tolist()}, replans {res.replans.tolist()}")
    assert res.planned[i1].all(), "choose pairs every class-1 vehicle has a plan for"
    assert (res.phase[i1] == _lib.FLEET_ABORTED).all() and (res.replans[i1] == 2).all(), (res.phase, res.replans)
    assert (res.steps[i1] == 0).all()
    assert (res.steps[i0] > 1).any()
    _assert_same_rows(mixed, i0, run(swarm(occ, len(i0), steps, params=two[0], **kw), i0), "class 0")
    failing = swarm(occ, len(i1), steps, params=two[1], relaxed_settings=FAIL_NOMINAL, **kw, **FAIL_NOMINAL)
    _assert_same_rows(mixed, i1, run(failing, i1), "class 1 (failing settings)")


# ---------------------------------------------------------------------- 6. a vehicle without a class
def test_bad_class_aborts_that_vehicle_and_never_replans_it(cuda, golden):
    """cls holds -1 and K for two vehicles that have a plan.  Each ends ABORTED with status BAD_CLASS, both masks
    0 and no replan used although replans were left in every later round: trace, state and reference rows are as
    loaded.  The others equal the run without them.  The index is checked before any use."""
    import torch
    from mpcqp import _lib

    cfg = (8, 60, 2.5, 2, 3)
    V, steps = cfg[0], cfg[1]
    valid = _run(golden, cfg, table=4, fused=True)  # which vehicles have a plan
    bad = np.flatnonzero(valid.res.planned)[[0, -1]]
    assert len(set(bad)) == 2
    good = np.setdiff1d(np.arange(V), bad)
    cls = np.arange(V) % 4
    cls[bad] = [-1, 4]
    sw = swarm(valid.occ, V, steps, replan_distance=cfg[2], max_replans=cfg[3], fused=True)
    sw.set_classes(blocks())
    res = sw.run(valid.starts, valid.goals, seeds=np.arange(V), classes=cls)
    torch.cuda.synchronize()  # no fault: an index outside the table was never used
    b = sw.fleet.buffers()
    got = SimpleNamespace(res=res, bufs=snap(sw.fleet), ref=b["ref_global"][:V].cpu().numpy().copy(),
                          ref_len=b["ref_len"][:V].cpu().numpy().copy())
    sw.fleet.close()
    assert (res.phase[bad] == _lib.FLEET_ABORTED).all(), res.phase
    assert (got.bufs["status"][0][bad] == BAD_CLASS).all(), got.bufs["status"]
    assert (got.bufs["mask"][:, bad] == 0).all()
    assert (res.replans[bad] == 0).all() and (res.replan_steps[bad] == 0).all(), (res.replans, res.replan_steps)
    assert (res.last_replan_start[bad] == 0).all()  # its start_goal row was never written
    assert all(res.last_replan_path[v] is None for v in bad)
    # as loaded: a tracker loaded with the same plans and stepped nowhere
    ft = fleet_tracker(N_HORIZON, len(bad), 512, steps, fused=True)
    ft.reset_from_plans([res.paths[v] for v in bad], valid.starts[bad], valid.goals[bad], max_steps=steps,
                        device_reference=True)
    loaded = snap(ft)
    lref = ft.buffers()["ref_global"][:len(bad)].cpu().numpy().copy()
    llen = ft.buffers()["ref_len"][:len(bad)].cpu().numpy().copy()
    ft.close()
    for k in ("state", "u_prev", "path_idx", "steps", "trace", "u_trace", "X", "u0"):
        np.testing.assert_array_equal(_rows(got.bufs, bad)[k], loaded[k], err_msg=f"buffer {k} of a vehicle without a class")
    np.testing.assert_array_equal(got.bufs["status"][1][bad], loaded["status"][1])
    np.testing.assert_array_equal(got.ref_len[bad], llen)
    _assert_same_refs(got.ref[bad], lref, llen, "a vehicle without a class")
    # the others ran as without them
    alone = _run(golden, cfg, idx=good, table=4, fused=True)
    assert (alone.res.steps > 1).any()
    _assert_same_rows(got, good, alone, "valid vehicles")


# ---------------------------------------------------------------------- 7. against the oracle
def _c_solve(params, state, window, u_prev):
    """One QP by the C restatement (oracle/mpcqp_cpu.c)."""
    import cpu_solver

    out = cpu_solver.cpu_solve(params, np.asarray(state, float)[None], np.asarray(window, float)[None],
                               np.asarray(u_prev, float)[None], nthreads=1)
    if out["status"][0] not in (1, 2):
        return None, None, None
    return out["u0"][0].copy(), out["X"][0].copy(), out["U"][0].copy()


def test_mixed_swarm_follows_the_oracle_under_each_class(cuda, golden):
    """The never-replanned vehicles of the tight-bounds and the 14 px wheelbase classes of the 100-vehicle mixed
    swarm, up to three each: step counts equal and states within ATOL of the oracle's track loop (C solves) under
    the oracle's block of that class."""
    import mpc_oracle as mo
    from mpcqp.control.ref_builder import build_reference

    V, steps = V100[0], V100[1]
    run = _run(golden, V100, table=4, fused=True)
    res = run.res
    oracle = {1: oracle_variant_params("tight_bounds", N_HORIZON),
              3: dataclasses.replace(mo.default_params(N_HORIZON, 0.8), wheelbase_px=14.0)}
    for c, op in oracle.items():
        never = [v for v in np.flatnonzero(res.planned & (res.replans == 0)) if v % 4 == c][:3]
        assert len(never) >= 1, f"class {c}: no never-replanned vehicle"
        for v in never:
            path = res.paths[v]
            ref = build_reference(path, 15.0, N_HORIZON, 0.1)
            yaw0 = float(np.arctan2(path[1][1] - path[0][1], path[1][0] - path[0][0])) if len(path) > 1 else 0.0
            host = np.asarray(mo.track_loop(op, ref, run.starts[v], yaw0, run.goals[v], steps, solve_fn=_c_solve))
            print(f"vehicle {v} ({NAMES[c]}): {res.steps[v]} steps, oracle {len(host)}, max |dx| "
                  f"{np.abs(res.states[v][:len(host)] - host[:res.steps[v]]).max():.3e}")
            assert res.steps[v] == len(host), (v, c)
            np.testing.assert_allclose(res.states[v], host, rtol=0, atol=ATOL, err_msg=f"vehicle {v} ({NAMES[c]})")


# ---------------------------------------------------------------------- 8. sharded
def test_sharded_mixed_swarm_equals_one_mixed_swarm(cuda, golden):
    """40 vehicles in three emulated ranks, each on its own Swarm with the class table, classes= cut like the
    seeds: the merged result equals the one mixed swarm exactly, with the trigger live."""
    from mpcqp.pipeline.swarm import merge_swarm_results, run_swarm_sharded, shard_vehicles

    V, steps, dist, max_replans, seed = V40
    world = 3
    one = _run(golden, V40, table=4, fused=True)
    cls = np.arange(V) % 4
    parts = []
    for r in range(world):
        lo, hi = shard_vehicles(V, world, r)
        sw = swarm(one.occ, hi - lo, steps, replan_distance=dist, max_replans=max_replans, fused=True)
        sw.set_classes(blocks())
        p = run_swarm_sharded(sw.run, one.starts, one.goals, np.arange(V), rank=r, world=world, classes=cls,
                              all_gather_object=lambda out, obj, r=r: out.__setitem__(r, obj))
        sw.fleet.close()
        assert len(p.steps) == hi - lo
        parts.append(p)
    got = merge_swarm_results(parts)
    assert one.res.replans.sum() >= 1, "the trigger should fire at 2.5 px"
    _assert_same_result(got, one.res, "sharded")


# ---------------------------------------------------------------------- 9. refusals write nothing
REFUSALS = {  # how: (horizon, settings, return code, what the message names)
    "n40": (40, {}, E_HORIZON, "fused"),
    "reproducible": (N_HORIZON, dict(reproducible=1), E_HORIZON, "fused"),
    "no_table": (N_HORIZON, {}, E_STATE, "nominal workspace"),
    "no_relaxed_table": (N_HORIZON, {}, E_STATE, "relaxed workspace"),
    "different_k": (N_HORIZON, {}, E_STATE, "1 classes"),
    "other_dt": (N_HORIZON, {}, E_ARG, "class 1"),
}


@pytest.mark.parametrize("how", list(REFUSALS))
def test_refused_mixed_swarm_calls_write_nothing(cuda, golden, how):
    """Both calls, each refusal: every fleet buffer and the swarm's replans / start_goal are as they were, and a
    build made on each workspace before the call still solves."""
    import torch
    from mpcqp import scenarios
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import relaxed_parameters
    from mpcqp.pipeline.swarm import Swarm

    occ = golden("default_plan.npz")["occupancy"]
    N, settings, code, names = REFUSALS[how]
    V, steps = 4, 12
    starts, goals = pairs(occ, V, 3)
    sw = Swarm(occ, MPCConfig(horizon=N, sim_steps=steps), planner_params(), map_resolution=0.8, max_vehicles=V,
               device="cuda:0", max_replans=1, replan_distance=2.5, fused=True, **settings)
    ft = sw.fleet
    p = ft.params
    other = dataclasses.replace(p, dt=0.05)
    nominal, relaxed = {"no_table": (None, None), "no_relaxed_table": ([p, p], None),
                        "different_k": ([p, p], [relaxed_parameters(p)]),
                        "other_dt": ([p, other], [relaxed_parameters(p), relaxed_parameters(other)])}.get(
                            how, ([p], [relaxed_parameters(p)]))
    ft._nominal.set_classes(nominal)  # straight on the controllers: Swarm.set_classes refuses some of these itself
    ft._relaxed.set_classes(relaxed)
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
    cls = ft.buffers()["cls"].data_ptr()
    fleet = (ft._nominal._ws, ft._relaxed._ws, ctypes.byref(ft._fleet), ctypes.byref(st), cls)
    for name, args in (("mpcqp_swarm_loop_mixed", ()), ("mpcqp_swarm_loop_mixed_warm", (8,))):
        rc = getattr(ft._L, name)(*fleet, *args, s)
        msg = ft._L.mpcqp_last_error().decode()
        assert rc == code, (how, name, rc, msg)
        assert name + (":" if code != E_HORIZON else " ") in msg and names in msg, (how, name, msg)
        assert_same(snap(ft), before, f"{how} {name}", LOOP_BUFFERS_MASK)
        assert (before["status"] == 77).all() and (before["steps"] == 0).all()
        assert bool((sbufs["start_goal"] == 77.0).all()) and bool((sbufs["replans"] == 0).all())
        for ctrl in (ft._nominal, ft._relaxed):  # both builds are still valid
            assert ctrl._L.mpcqp_solve(ctrl._ws, V, None, None, None, ctrl._status.data_ptr(), None, None, s) == 0
    torch.cuda.synchronize()
    if how == "other_dt":  # and Swarm.set_classes refuses it before the device does
        with pytest.raises(ValueError, match="one dt"):
            sw.set_classes([p, other])
    ft.close()
