"""GPU tests of the fused fleet loop with a class per vehicle at two vehicles per wave
(``mpcqp_set_class_pairing`` on the nominal workspace, ``k_fleet_loop_pair_mixed`` in csrc/mpcqp_solve.h;
``FleetTracker(class_pairing="on")``).

The claim: every buffer the loop owns (``LOOP_BUFFERS_MASK``) equals, bit for bit, what the same mixed loop
leaves at one vehicle per wave -- while the two vehicles of a wave reach the goal at different steps, abort,
are not RUNNING at entry or have no class -- and ``launch_info()`` reports two per wave.  The unpaired mixed
loop is tied to the homogeneous loops and the exact oracle by ``test_gpu_fleet_classes.py``."""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import (FAIL_NOMINAL, LOOP_BUFFERS_MASK, TWO_SLOT, assert_same, fleet_tracker, snap, variant_blocks,
                         varied_fleet)

pytestmark = pytest.mark.gpu

M_REF = 128  # reference rows per vehicle (the longest of these plans has 45, at every dt used here)
BLOCKS = ("default", "dt_0.2", "wheelbase_14px")  # another dt, another wheelbase
SENT = -777.0


def _rows(bufs, idx):
    return {k: (a[:, idx] if k in TWO_SLOT else a[idx]) for k, a in bufs.items()}


def _run(N, max_steps, blocks, cls, fleet, class_pairing, parts, *, prep=None, set_classes_kw=None, fill=False):
    """One mixed fused run in launches of ``parts`` steps: (snapshot before, snapshot after, launch_info)."""
    paths, starts, goals = fleet
    ft = fleet_tracker(N, len(paths), M_REF, max_steps, fused=True, class_pairing=class_pairing)
    ft.set_classes(blocks, **(set_classes_kw or {}))
    ft.reset_from_plans(paths, starts, goals, classes=cls)
    if fill:
        for k in ("trace", "X", "u0"):
            ft.buffers()[k].fill_(SENT)
    if prep:
        prep(ft)
    before = snap(ft)
    for k in parts:
        ft.step(k)
    after = snap(ft)
    info = ft._nominal.launch_info()
    ft.close()
    return before, after, info


def _waves(V, K):
    from mpcqp import _lib

    return _lib.lib().mpcqp_class_slot_waves(V, K)


# ---------------------------------------------------------------------- 6. paired against unpaired
@pytest.mark.parametrize("N", [3, 15])
def test_class_paired_loop_equals_unpaired_bitwise(cuda, golden, N):
    """Seven vehicles in three classes (3 + 2 + 2), run to their ends: class-mates leave the loop at different
    steps, so halves of a wave run on alone."""
    from mpcqp import _lib

    V, max_steps = 7, 40
    _, paths, starts, goals = varied_fleet(golden, V, seed=5)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.arange(V) % 3
    fleet = (paths, starts, goals)
    _, off, info_off = _run(N, max_steps, blocks, cls, fleet, "off", [max_steps])
    _, on, info_on = _run(N, max_steps, blocks, cls, fleet, "on", [max_steps])
    print("steps", off["steps"].tolist(), "phase", off["phase"].tolist())
    assert any(len(set(off["steps"][cls == c])) > 1 for c in range(3)), "no class whose vehicles differ in steps"
    assert (off["phase"] == _lib.FLEET_GOAL).any() and not (off["phase"] == _lib.FLEET_RUNNING).any(), off["phase"]
    assert info_off["kind"] == info_on["kind"] == _lib.LAUNCH_LOOP_MIXED
    assert info_off["per_wave"] == 1 and info_off["workgroups"] == V
    assert info_on["per_wave"] == 2 and info_on["workgroups"] == _waves(V, 3) and info_on["count"] == V
    assert_same(on, off, f"N={N} class pairing on against off", LOOP_BUFFERS_MASK)


# ---------------------------------------------------------------------- 7. halves that leave at once
def test_a_class_that_fails_aborts_beside_running_waves(cuda, golden):
    """Class 1 fails every solve on both tables: its vehicles abort in their first step, in waves of their
    own, and the other classes run as without the switch."""
    from mpcqp import _lib

    N, V, max_steps, steps = 10, 7, 40, 6
    _, paths, starts, goals = varied_fleet(golden, V, seed=4)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.arange(V) % 3
    kw = dict(settings=[{}, FAIL_NOMINAL, {}], relaxed_settings=[{}, FAIL_NOMINAL, {}])
    fleet = (paths, starts, goals)
    _, off, _ = _run(N, max_steps, blocks, cls, fleet, "off", [steps], set_classes_kw=kw)
    _, on, info = _run(N, max_steps, blocks, cls, fleet, "on", [steps], set_classes_kw=kw)
    assert (off["phase"][cls == 1] == _lib.FLEET_ABORTED).all() and (off["steps"][cls == 1] == 0).all()
    assert (off["steps"][cls != 1] == steps).all(), off["steps"]
    assert info["per_wave"] == 2
    assert_same(on, off, "a failing class", LOOP_BUFFERS_MASK)


def test_a_vehicle_not_running_leaves_its_partner_alone(cuda, golden):
    """A class of two: vehicle 1 is at its goal when the launch starts and vehicle 4 is RUNNING.  The first is
    not touched, the second runs alone in its wave."""
    from mpcqp import _lib

    N, V, max_steps, steps = 10, 6, 40, 6
    _, paths, starts, goals = varied_fleet(golden, V, seed=4)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.arange(V) % 3  # class 1: vehicles 1 and 4

    def prep(ft):
        ft.buffers()["phase"][1] = _lib.FLEET_GOAL

    fleet = (paths, starts, goals)
    _, off, _ = _run(N, max_steps, blocks, cls, fleet, "off", [steps], prep=prep, fill=True)
    before, on, info = _run(N, max_steps, blocks, cls, fleet, "on", [steps], prep=prep, fill=True)
    assert info["per_wave"] == 2 and info["workgroups"] == _waves(V, 3)
    assert_same(_rows(on, [1]), _rows(before, [1]), "the vehicle that was not RUNNING", LOOP_BUFFERS_MASK)
    assert on["steps"][4] == steps
    assert_same(on, off, "a partner that is not RUNNING", LOOP_BUFFERS_MASK)


def test_bad_class_aborts_that_vehicle_only(cuda, golden):
    """Vehicles without a class share the further bucket: ABORTED, BAD_CLASS, both masks 0, nothing else of
    them written, and the others as in the unpaired loop -- which is as without them (test_gpu_fleet_classes)."""
    from mpcqp import _lib

    N, V, max_steps, steps = 10, 8, 40, 6
    _, paths, starts, goals = varied_fleet(golden, V, seed=4)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.array([0, 1, -1, 2, 0, 3, 1, 2], dtype=np.int64)
    bad = np.array([2, 5])
    fleet = (paths, starts, goals)
    _, off, _ = _run(N, max_steps, blocks, cls, fleet, "off", [steps], fill=True)
    before, on, info = _run(N, max_steps, blocks, cls, fleet, "on", [steps], fill=True)
    assert info["per_wave"] == 2
    assert (on["phase"][bad] == _lib.FLEET_ABORTED).all(), on["phase"]
    assert (on["status"][0][bad] == _lib.BAD_CLASS).all(), on["status"]
    assert (on["mask"][:, bad] == 0).all()
    for k in LOOP_BUFFERS_MASK:  # nothing else of a bad vehicle is written
        if k in ("phase", "mask"):
            continue
        a, b = _rows(on, bad)[k], _rows(before, bad)[k]
        if k == "status":
            a, b = a[1], b[1]  # the relaxed slot; the nominal one holds BAD_CLASS
        np.testing.assert_array_equal(a, b, err_msg=f"buffer {k} of a vehicle without a class")
    good = np.setdiff1d(np.arange(V), bad)
    assert (on["steps"][good] == steps).all()
    assert_same(on, off, "with vehicles that have no class", LOOP_BUFFERS_MASK)


# ---------------------------------------------------------------------- 8. split launches
def test_split_launches_add_up_bitwise(cuda, golden):
    """Ten steps as 5 + 5 equal ten steps in one launch, and both equal the unpaired loop."""
    N, V, max_steps = 10, 7, 30
    _, paths, starts, goals = varied_fleet(golden, V, seed=9)
    blocks = variant_blocks(N, BLOCKS)
    cls = np.arange(V) % 3
    fleet = (paths, starts, goals)
    _, off, _ = _run(N, max_steps, blocks, cls, fleet, "off", [10])
    _, whole, _ = _run(N, max_steps, blocks, cls, fleet, "on", [10])
    _, split, info = _run(N, max_steps, blocks, cls, fleet, "on", [5, 5])
    assert info["per_wave"] == 2
    assert (off["steps"] == 10).any()
    assert_same(split, whole, "5 + 5 steps against 10", LOOP_BUFFERS_MASK)
    assert_same(whole, off, "10 steps against the unpaired loop", LOOP_BUFFERS_MASK)


# ---------------------------------------------------------------------- 9. the longest-first path
def test_longest_first_dispatch_order(cuda, golden):
    """More vehicles than wave slots (8 per CU): the slot table is built over the dispatch order."""
    import torch
    from mpcqp.control.ref_builder import build_reference
    from mpcqp.pipeline.fleet import initial_states

    N, steps = 3, 3
    V = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    _, paths, starts, goals = varied_fleet(golden, V, seed=6)
    blocks = variant_blocks(N, BLOCKS + ("tight_bounds",))
    cls = np.arange(V) % 4
    distinct = {}  # varied_fleet cycles through 13 plans: one reference per (plan, dt)

    def ref_of(v):
        key = (v % 13, blocks[cls[v]].dt)
        if key not in distinct:
            distinct[key] = build_reference(paths[v], 15.0, N, blocks[cls[v]].dt)
        return distinct[key]

    refs = [ref_of(v) for v in range(V)]
    s0 = initial_states(paths, starts)
    out = []
    for mode in ("off", "on"):
        ft = fleet_tracker(N, V, M_REF, steps, fused=True, class_pairing=mode)
        ft.set_classes(blocks)
        ft.reset(refs, s0, goals, classes=cls)
        ft.run()
        out.append(snap(ft))
        info = ft._nominal.launch_info()
        ft.close()
    assert info["per_wave"] == 2 and info["workgroups"] == _waves(V, 4) and info["count"] == V, info
    assert (out[0]["steps"] == steps).any()
    assert_same(out[1], out[0], "longest first, class pairing on against off", LOOP_BUFFERS_MASK)
