"""GPU tests of the fused fleet loop with a parameter class per vehicle (``mpcqp_fleet_loop_mixed``,
``k_fleet_loop_mixed`` in csrc/mpcqp_solve.h; ``FleetTracker.set_classes`` / ``classes=``).

The claim: vehicle v of a mixed fleet gets, bit for bit, the buffers of a homogeneous fused fleet
(``mpcqp_fleet_loop``) under its class's nominal and relaxed blocks -- so every comparison with a
homogeneous fleet is ``assert_array_equal`` over every buffer row.  Against the exact oracle's loop
the states agree to the 1e-7 px of test_gpu_fleet.py.  Fleets are those of
``gpu_helpers.varied_fleet``, the blocks come from ``param_variants``, and each vehicle's
reference is built with its class's ``dt``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
from gpu_helpers import (ATOL, E_HORIZON, E_STATE, FAIL_NOMINAL, LOOP_BUFFERS_MASK, TWO_SLOT, assert_same,
                         fleet_tracker, oracle_variant_params, snap, variant_blocks, variant_params, varied_fleet)

pytestmark = pytest.mark.gpu

BLOCKS = ["default", "dt_0.05", "dt_0.2", "wheelbase_14px", "tight_bounds", "q_nondiag"]
M_REF = 128  # reference rows per vehicle (the longest of these plans has 45, at every dt used here)


def _rows(bufs, idx):
    return {k: (a[:, idx] if k in TWO_SLOT else a[idx]) for k, a in bufs.items()}


def _sub(seq, idx):
    return [seq[i] for i in idx]


def _homogeneous(N, max_steps, block, paths, starts, goals, steps=None, **settings):
    """The buffers of a homogeneous fused fleet under ``block`` (reference at the block's dt)."""
    ft = fleet_tracker(N, len(paths), M_REF, max_steps, fused=True, params=block, **settings)
    ft.reset_from_plans(paths, starts, goals)
    for k in ([max_steps] if steps is None else steps):
        ft.step(k)
    out = snap(ft)
    ft.close()
    return out


def _check_against_per_class_fleets(got, cls, N, max_steps, blocks, paths, starts, goals, steps=None, per_class=None):
    for c, block in enumerate(blocks):
        idx = np.flatnonzero(cls == c)
        assert len(idx), f"class {c} has no vehicle"
        kw = per_class[c] if per_class else {}
        want = _homogeneous(N, max_steps, block, _sub(paths, idx), starts[idx], goals[idx], steps, **kw)
        assert_same(_rows(got, idx), want, f"class {c}", LOOP_BUFFERS_MASK)


@pytest.mark.parametrize("N", [3, 10, 20, 32])
def test_mixed_fleet_equals_homogeneous_fleets_bitwise(cuda, golden, N):
    """18 vehicles, six classes (two dt's off the default, another wheelbase, tighter bounds, a
    non-diagonal Q), 25 steps; N = 10 is a horizon at which homogeneous loops may pair."""
    from mpcqp import _lib

    V, steps = 18, 25
    _, paths, starts, goals = varied_fleet(golden, V, seed=5)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.arange(V) % len(blocks)
    ft = fleet_tracker(N, V, M_REF, steps, fused=True)
    ft.set_classes(blocks)
    ft.reset_from_plans(paths, starts, goals, classes=cls)
    res = ft.run()
    got = snap(ft)
    ft.close()
    assert (res.steps > 0).any(), "no vehicle stepped"
    assert np.isin(res.phase, [_lib.FLEET_GOAL, _lib.FLEET_OUT_OF_STEPS]).any(), res.phase
    assert not (res.phase == _lib.FLEET_RUNNING).any()
    _check_against_per_class_fleets(got, cls, N, steps, blocks, paths, starts, goals)


@pytest.mark.parametrize("N,pairing", [(3, "on"), (20, "auto")])
def test_one_class_equals_the_plain_loop_bitwise(cuda, golden, N, pairing):
    """K = 1 with the tracker's own block against plain mpcqp_fleet_loop (N = 3: the plain side runs two
    vehicles per wave, the mixed side never does)."""

    V, steps = 9, 20
    _, paths, starts, goals = varied_fleet(golden, V, seed=7)
    ft = fleet_tracker(N, V, M_REF, steps, fused=True)
    ft.set_classes([ft.params])
    ft.reset_from_plans(paths, starts, goals, classes=np.zeros(V, np.int32))
    ft.run()
    got = snap(ft)
    ft.close()
    want = _homogeneous(N, steps, None, paths, starts, goals, pairing=pairing)
    assert_same(got, want, "K = 1", LOOP_BUFFERS_MASK)


def test_mixed_fleet_matches_exact_oracle_loop(cuda, golden):
    """N = 15, 30 steps, 12 vehicles over the six blocks: each vehicle against the exact oracle's loop
    under its own block and reference.  Step counts equal, states within 1e-7 px."""
    import mpc_oracle as mo
    from mpcqp import _lib
    from mpcqp.control.ref_builder import build_reference

    N, steps, V = 15, 30, 12
    _, paths, starts, goals = varied_fleet(golden, V, seed=5)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.arange(V) % len(blocks)
    ft = fleet_tracker(N, V, M_REF, steps, fused=True)
    ft.set_classes(blocks)
    refs = ft.reset_from_plans(paths, starts, goals, classes=cls)
    res = ft.run()
    ft.close()
    assert not (res.phase == _lib.FLEET_ABORTED).any(), res.phase
    assert (res.phase == _lib.FLEET_GOAL).any() and (res.phase == _lib.FLEET_OUT_OF_STEPS).any(), res.phase
    for v in range(V):
        name = BLOCKS[cls[v]]
        op = oracle_variant_params(name, N)
        ref = build_reference(paths[v], 15.0, N, op.dt)
        np.testing.assert_array_equal(refs[v], ref)
        p = paths[v]
        yaw0 = float(np.arctan2(p[1][1] - p[0][1], p[1][0] - p[0][0]))
        ex = np.asarray(mo.track_loop(op, ref, starts[v], yaw0, goals[v], steps))
        print(f"vehicle {v} ({name}): {res.steps[v]} steps, oracle {len(ex)}, "
              f"max |dx| {np.abs(res.states[v][:len(ex)] - ex[:res.steps[v]]).max():.3e}")
        assert res.steps[v] == len(ex), (v, name)
        np.testing.assert_allclose(res.states[v], ex, rtol=0, atol=ATOL, err_msg=f"vehicle {v} ({name})")


def test_relaxed_retry_per_class(cuda, golden):
    """Class 1's nominal settings fail every QP, so its vehicles take the retry under relaxed block 1
    (another wheelbase than class 0's): a wrong 2c + relax index would show in the bits."""
    from mpcqp import _lib

    N, V, max_steps, steps = 10, 8, 50, 5
    _, paths, starts, goals = varied_fleet(golden, V, seed=2)
    blocks = [variant_params("default", N), variant_params("wheelbase_14px", N)]
    cls = np.array([0, 1, 1, 0, 1, 0, 0, 1])
    ft = fleet_tracker(N, V, M_REF, max_steps, fused=True)
    ft.set_classes(blocks, settings=[{}, FAIL_NOMINAL], relaxed_settings=[{}, {}])
    ft.reset_from_plans(paths, starts, goals, classes=cls)
    ft.step(steps)
    got = snap(ft)
    ft.close()
    assert (got["phase"] == _lib.FLEET_RUNNING).all(), got["phase"]
    assert (got["steps"] == steps).all()
    np.testing.assert_array_equal(got["mask"][1], (cls == 1).astype(np.uint8))
    assert (got["status"][0][cls == 1] == _lib.MAX_ITER_REACHED).all() and (got["status"][1][cls == 1] == 1).all()
    assert (got["status"][0][cls == 0] == 1).all()
    _check_against_per_class_fleets(got, cls, N, max_steps, blocks, paths, starts, goals, steps=[steps],
                                    per_class=[{}, dict(relaxed_settings={}, **FAIL_NOMINAL)])


def test_bad_class_aborts_that_vehicle_only(cuda, golden):
    import torch
    from mpcqp import _lib

    N, V, max_steps, steps = 10, 10, 40, 6
    SENT = -777.0
    _, paths, starts, goals = varied_fleet(golden, V, seed=4)
    blocks = variant_blocks(N, ("default", "dt_0.2", "tight_bounds"))
    cls = np.array([0, 1, -1, 2, 0, len(blocks), 1, 2**31 - 1, 2, 0], dtype=np.int64)
    bad = np.flatnonzero((cls < 0) | (cls >= len(blocks)))
    good = np.flatnonzero((cls >= 0) & (cls < len(blocks)))
    assert list(bad) == [2, 5, 7]

    def run(idx):
        ft = fleet_tracker(N, len(idx), M_REF, max_steps, fused=True)
        ft.set_classes(blocks)
        ft.reset_from_plans(_sub(paths, idx), starts[idx], goals[idx], classes=cls[idx])
        for k in ("trace", "X", "u0"):
            ft.buffers()[k].fill_(SENT)
        before = snap(ft)
        ft.step(steps)
        torch.cuda.synchronize()  # no fault: an index outside the table was never used
        after = snap(ft)
        ft.close()
        return before, after

    before, after = run(np.arange(V))
    assert (after["phase"][bad] == _lib.FLEET_ABORTED).all(), after["phase"]
    assert (after["status"][0][bad] == _lib.BAD_CLASS).all(), after["status"]
    assert (after["mask"][:, bad] == 0).all()
    for k in LOOP_BUFFERS_MASK:  # nothing else of a bad vehicle is written
        if k in ("phase", "mask"):
            continue
        a, b = _rows(after, bad)[k], _rows(before, bad)[k]
        if k == "status":
            a, b = a[1], b[1]  # the relaxed slot; the nominal one holds BAD_CLASS
        np.testing.assert_array_equal(a, b, err_msg=f"buffer {k} of a vehicle without a class")
    assert (after["trace"][bad] == SENT).all() and (after["X"][bad] == SENT).all() and (after["u0"][:, bad] == SENT).all()
    # the others ran as without them
    assert (after["steps"][good] == steps).all()
    _, alone = run(good)
    assert_same(_rows(after, good), alone, "valid vehicles", LOOP_BUFFERS_MASK)


def test_partial_runs_add_up_bitwise(cuda, golden):
    """step(3) then step(4) == step(7): the loop state written back between launches is complete."""

    N, V, max_steps = 10, 9, 30
    _, paths, starts, goals = varied_fleet(golden, V, seed=9)
    blocks = variant_blocks(N, ("default", "dt_0.05", "q_nondiag"))
    cls = np.arange(V) % 3
    out = []
    for parts in ([3, 4], [7]):
        ft = fleet_tracker(N, V, M_REF, max_steps, fused=True)
        ft.set_classes(blocks)
        ft.reset_from_plans(paths, starts, goals, classes=cls)
        for k in parts:
            ft.step(k)
        out.append(snap(ft))
        ft.close()
    assert (out[0]["steps"] == 7).any()
    assert_same(out[0], out[1], "3 + 4 steps against 7", LOOP_BUFFERS_MASK)


def test_longest_first_dispatch_order(cuda, golden):
    """More vehicles than wave slots (8 per CU): the launch dispatches through the order table."""
    import torch
    from mpcqp.control.ref_builder import build_reference
    from mpcqp.pipeline.fleet import initial_states

    N, steps = 3, 4
    V = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    _, paths, starts, goals = varied_fleet(golden, V, seed=6)
    names = ["default", "dt_0.2", "wheelbase_14px"]
    blocks = variant_blocks(N, names)
    cls = np.arange(V) % 3
    distinct = {}  # varied_fleet cycles through 13 plans: one reference per (plan, dt)

    def ref_of(v):
        key = (v % 13, blocks[cls[v]].dt)
        if key not in distinct:
            distinct[key] = build_reference(paths[v], 15.0, N, blocks[cls[v]].dt)
        return distinct[key]

    for v in range(13, 26):
        assert paths[v] is paths[v - 13]
    refs = [ref_of(v) for v in range(V)]
    s0 = initial_states(paths, starts)
    ft = fleet_tracker(N, V, M_REF, steps, fused=True)
    ft.set_classes(blocks)
    ft.reset(refs, s0, goals, classes=cls)
    ft.run()
    got = snap(ft)
    ft.close()
    assert (got["steps"] == steps).any()
    for c, block in enumerate(blocks):
        idx = np.flatnonzero(cls == c)
        h = fleet_tracker(N, len(idx), M_REF, steps, fused=True, params=block)
        h.reset(_sub(refs, idx), s0[idx], goals[idx])
        h.run()
        want = snap(h)
        h.close()
        assert_same(_rows(got, idx), want, f"class {c}", LOOP_BUFFERS_MASK)


def _raw_mixed(ft, steps=2):
    from mpcqp import _lib
    import torch

    L = _lib.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream(ft.device).cuda_stream)
    rc = L.mpcqp_fleet_loop_mixed(ft._nominal._ws, ft._relaxed._ws, ctypes.byref(ft._fleet),
                                  ft.buffers()["cls"].data_ptr(), steps, s)
    return rc, L.mpcqp_last_error().decode()


def test_mixed_loop_refusals(cuda, golden):
    import torch
    from mpcqp import _lib
    from mpcqp.pipeline.fleet import relaxed_parameters

    V, max_steps = 4, 12
    _, paths, starts, goals = varied_fleet(golden, V, seed=8)

    def fresh(N, **settings):
        ft = fleet_tracker(N, V, M_REF, max_steps, fused=True, **settings)
        ft.reset_from_plans(paths, starts, goals)
        return ft

    # a class table on one workspace only, and tables of different sizes
    ft = fresh(10)
    p = ft.params
    before = snap(ft)
    ft._nominal.set_classes([p, p])
    rc, msg = _raw_mixed(ft)
    assert rc == E_STATE and "relaxed workspace" in msg, (rc, msg)
    ft._relaxed.set_classes([relaxed_parameters(p)])
    rc, msg = _raw_mixed(ft)
    assert rc == E_STATE and "1 classes" in msg and "2" in msg, (rc, msg)
    ft._nominal.set_classes(None)
    rc, msg = _raw_mixed(ft)
    assert rc == E_STATE and "nominal workspace" in msg, (rc, msg)
    assert_same(snap(ft), before, "after the refused calls", LOOP_BUFFERS_MASK)
    ft.close()

    # parameter blocks that do not run the fused kernel: refused, nothing enqueued
    for N, settings in ((33, {}), (10, dict(reproducible=1))):
        ft = fresh(N, **settings)
        ft._nominal.set_classes([ft.params])
        ft._relaxed.set_classes([relaxed_parameters(ft.params)])
        before = snap(ft)
        rc, msg = _raw_mixed(ft)
        assert rc == E_HORIZON and "fused" in msg, (N, settings, rc, msg)
        assert_same(snap(ft), before, f"N = {N} {settings}: fleet buffers after the refusal", LOOP_BUFFERS_MASK)
        if N > 32:  # the tracker itself refuses earlier
            with pytest.raises(ValueError, match="horizon <= 32"):
                ft.set_classes([ft.params])
        ft.close()

    # a mixed loop invalidates the workspaces' builds ...
    N = 10
    ft = fresh(N)
    ctrl = ft._nominal
    x0 = np.tile([10.0, 10.0, 0.0, 5.0], (V, 1))
    ref = np.tile(np.array([[10.0 + 1.5 * k, 10.0, 0.0, 15.0] for k in range(N + 1)]), (V, 1, 1))
    ctrl.solve_batch(x0, ref)
    ft.set_classes([ft.params, variant_params("dt_0.2", N)])
    ft.reset_from_plans(paths, starts, goals, classes=np.array([0, 1, 1, 0]))
    ft.step(3)
    torch.cuda.synchronize()
    L = _lib.lib()
    rc = L.mpcqp_solve(ctrl._ws, V, ctrl._u0.data_ptr(), ctrl._X.data_ptr(), ctrl._U.data_ptr(), ctrl._status.data_ptr(),
                       ctrl._iters.data_ptr(), ctrl._active.data_ptr(), None)
    assert rc == E_STATE, (rc, L.mpcqp_last_error())
    # ... and leaves them fit for the plain loop: the same buffers as on fresh workspaces
    ft.reset_from_plans(paths, starts, goals)
    s = ctypes.c_void_p(torch.cuda.current_stream(ft.device).cuda_stream)
    assert L.mpcqp_fleet_loop(ft._nominal._ws, ft._relaxed._ws, ctypes.byref(ft._fleet), max_steps, s) == 0
    got = snap(ft)
    ft.close()
    assert_same(got, _homogeneous(N, max_steps, None, paths, starts, goals), "plain loop after a mixed one",
                LOOP_BUFFERS_MASK)
