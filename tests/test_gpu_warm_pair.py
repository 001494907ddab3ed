"""GPU tests of warm start at two QPs per wave (``k_solve_pair_warm``, ``k_fleet_loop_warm_carry<N, true>``) and
of the guess carried across launches (``mpcqp_fleet_loop_warm_carry``).

The contract (include/mpcqp.h): under ``pairing="on"`` a warm launch runs two QPs (vehicles) per wave, each
half through its own attempt, and every output equals the one-per-wave warm launch bit for bit -- so the
yardstick here is the unpaired warm kernel, which this change leaves untouched, and the exact oracle beside
it.  A run split into launches over one carried buffer equals the same run in one ``mpcqp_fleet_loop_warm``
launch bit for bit.  ``launch_info()`` tells what a launch did, so "paired" is an observation, not a belief.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
from gpu_helpers import (E_ARG, E_HORIZON, LOOP_BUFFERS_MASK, OUTS, assert_exact, assert_same, base_params, config3_case,
                         controller, default_plan, fleet_tracker, loop_buffers, run_loop, snap, take, varied_fleet)

pytestmark = pytest.mark.gpu

# the eight waves of the pattern test: H M | M H | H U | U H | M U | H H | M M | H and an absent half
PATTERN = "HM" "MH" "HU" "UH" "MU" "HH" "MM" "H"


def _guesses(case, kinds):
    """Row b's guess by its kind: H the exact optimum, M zeros, U the optimum with one NaN entry."""
    N = case["guesses"].shape[2]
    g = case["guesses"][:len(kinds)].copy()
    for b, kind in enumerate(kinds):
        if kind == "M":
            g[b] = 0.0
        elif kind == "U":
            g[b, b % 2, (3 * b) % N] = np.nan
    return g


def _warm_both_ways(case, g, passes, N, want_pairs=True):
    """The rows of `g` solved warm under pairing "off" and "on" (and cold, unpaired), with what
    launch_info said of the two warm launches."""
    from mpcqp import _lib

    B = len(g)
    args = (case["x0"][:B], case["ref"][:B], case["u_prev"][:B])
    out = {}
    for mode in ("off", "on"):
        ctrl = controller(case["params"], B, pairing=mode)
        assert ctrl.launch_info()["kind"] == _lib.LAUNCH_NONE
        out[mode] = take(ctrl.solve_batch(*args, U_guess=g, guess_passes=passes))
        info = ctrl.launch_info()
        per_wave = 2 if (mode == "on" and want_pairs) else 1
        assert info == dict(kind=_lib.LAUNCH_SOLVE_WARM, name="solve_warm", per_wave=per_wave,
                            workgroups=(B + per_wave - 1) // per_wave, count=B), (N, mode, info)
        if mode == "off":
            out["cold"] = take(ctrl.solve_batch(*args))
            assert ctrl.launch_info()["kind"] == _lib.LAUNCH_SOLVE
        ctrl.close()
    return out


# ---------------------------------------------------------------------- 1. the batch
@pytest.mark.parametrize("N", [10, 15])
def test_half_patterns(cuda, N):
    """One half hits while the other misses, holds an unusable guess or is absent: every output of the
    paired launch, iters included, is the unpaired warm launch's bit for bit, and the unpaired launch shows
    that the rows were what they were meant to be (tests/test_warm_pair_host.py: zeros miss by a wide
    margin under two passes; the optima are clear of their bounds)."""
    case = config3_case(N, 16, 5200 + N, margins=True)
    B = len(PATTERN)
    assert B == 15
    out = _warm_both_ways(case, _guesses(case, PATTERN), 2, N)
    off, on, cold = out["off"], out["on"], out["cold"]
    assert_same(on, off, f"N={N} paired against unpaired warm")
    # what each row was, from the unpaired run (the kernel that was there before)
    seen = ""
    for b in range(B):
        if off["iters"][b, 0] == 0:
            seen += "H"
        elif all(np.array_equal(off[k][b], cold[k][b]) for k in OUTS):
            seen += "U"
        elif off["iters"][b, 0] > 0 and off["iters"][b, 1] > cold["iters"][b, 1]:
            seen += "M"
        else:
            seen += "?"
    print(f"N={N}: meant {PATTERN}, seen {seen}; iters {off['iters'].tolist()}")
    waves = [(PATTERN[i:i + 2], seen[i:i + 2]) for i in range(0, B, 2)]
    assert sum(meant == got for meant, got in waves) >= 7, (PATTERN, seen)
    got = [w for _, w in waves]
    assert "HM" in got and "MH" in got and ("HU" in got or "UH" in got), seen
    for b in range(B):
        assert_exact(on, b, case["exact"][b], f"N={N} paired warm", solved=True)


@pytest.mark.parametrize("N,B", [(1, 5), (2, 5), (15, 2), (16, 5)])
def test_paired_warm_small_and_edge(cuda, N, B):
    """N = 1, 2: a half of one or two variable pairs; B odd: an absent half; N = 15, B = 2: one full wave at
    the pair limit; N = 16: no paired kernel, "on" runs one QP per wave."""
    case = config3_case(N, 16, 5200 + N, margins=True)
    out = _warm_both_ways(case, _guesses(case, "HMUHM"[:B]), 2, N, want_pairs=N <= 15)
    assert_same(out["on"], out["off"], f"N={N} paired against unpaired warm")
    for b in range(B):
        assert_exact(out["on"], b, case["exact"][b], f"N={N}", solved=True)


def test_guess_may_be_the_output_buffer_when_paired(cuda):
    """U_guess aliasing U under pairing "on": each half reads its row before it writes it."""
    import warm_newton as wn

    N = 10
    case = config3_case(N, 16, 5200 + N, margins=True)
    B = 15  # an absent half too
    ctrl = controller(case["params"], B, pairing="on")
    args = (case["x0"][:B], case["ref"][:B], case["u_prev"][:B])
    first = ctrl.solve_batch(*args)
    assert ctrl.launch_info()["per_wave"] == 2
    again = take(ctrl.solve_batch(*args, U_guess=first.U))  # the controller's own U tensor
    assert ctrl.launch_info()["per_wave"] == 2 and ctrl.launch_info()["workgroups"] == 8
    ctrl.close()
    clear = case["margins"] > wn.MARGIN
    for b in range(B):
        assert_exact(again, b, case["exact"][b], "aliased", solved=True)
        if clear[b]:
            assert again["iters"][b, 0] == 0, (b, again["iters"][b])


def test_auto_does_not_pair_warm_launches(cuda):
    """More QPs than wave slots: "auto" pairs the cold solve and leaves the warm one at one QP per wave."""
    import torch
    from mpcqp import _lib, scenarios

    N = 3
    B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    batch = scenarios.config3(B, horizon=N, seed=77)
    ctrl = controller(base_params(N), B, pairing="auto")
    cold = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev))
    info = ctrl.launch_info()
    assert info == dict(kind=_lib.LAUNCH_SOLVE, name="solve", per_wave=2, workgroups=(B + 1) // 2, count=B), info
    warm = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, U_guess=np.zeros((B, 2, N))))
    info = ctrl.launch_info()
    assert info == dict(kind=_lib.LAUNCH_SOLVE_WARM, name="solve_warm", per_wave=1, workgroups=B, count=B), info
    ctrl.close()
    np.testing.assert_array_equal(warm["status"], cold["status"])


# ---------------------------------------------------------------------- 2. the fused loop, paired
@pytest.mark.parametrize("N,steps", [(10, None), (1, 6), (15, 6)])
def test_paired_warm_loop_is_the_unpaired_warm_loop_bit_for_bit(cuda, golden, N, steps):
    """Odd V and plans of different lengths: the halves of a wave hit, miss and leave at different steps."""
    from mpcqp import _lib

    V = 5
    plans = varied_fleet(golden, V, seed=41 + N)[1:]
    kw = dict(sim_steps=300 if steps is None else steps, fused=True)
    out = {}
    for name, opts in (("off", dict(warm_start=True, pairing="off")), ("on", dict(warm_start=True, pairing="on")),
                       ("cold_on", dict(pairing="on")), ("p0_on", dict(warm_start=True, guess_passes=0, pairing="on"))):
        ft = fleet_tracker(N, V, 128, **kw, **opts)
        ft.reset_from_plans(*plans)
        res = ft.run() if steps is None else (ft.step(steps), ft.result())[1]
        info = ft._nominal.launch_info()
        per_wave = 1 if name == "off" else 2
        assert info == dict(kind=_lib.LAUNCH_LOOP if name == "cold_on" else _lib.LAUNCH_LOOP_WARM,
                            name="loop" if name == "cold_on" else "loop_warm", per_wave=per_wave,
                            workgroups=(V + per_wave - 1) // per_wave, count=V), (name, info)
        out[name] = (res, loop_buffers(ft, LOOP_BUFFERS_MASK))
        ft.close()
    res = out["off"][0]
    print(f"N={N}: steps {res.steps.tolist()}, phases {res.phase.tolist()}")
    assert (res.steps > 0).all()
    if steps is None:
        assert (res.phase != _lib.FLEET_RUNNING).all() and len(set(res.steps.tolist())) > 1
    for k in LOOP_BUFFERS_MASK:
        np.testing.assert_array_equal(out["on"][1][k], out["off"][1][k], err_msg=f"warm: {k}")
        np.testing.assert_array_equal(out["p0_on"][1][k], out["cold_on"][1][k], err_msg=f"guess_passes=0: {k}")


def test_paired_warm_loop_relaxation_branches(cuda, golden):
    """test_warm_loop_relaxation_branches' scenario with two vehicles per wave: the vehicle whose QP is
    non-finite is retried relaxed and aborts alone; its wave partner runs on as in the unpaired warm loop."""
    from mpcqp import _lib

    N, steps, V = 10, 20, 6
    g, path = default_plan(golden)
    out = []
    for mode in ("off", "on"):
        ft = fleet_tracker(N, V, 64, steps, float(g["map_resolution"]), fused=True, warm_start=True, pairing=mode)
        ft.reset_from_plans([path] * V, np.tile(g["start"], (V, 1)), np.tile(g["goal"], (V, 1)))
        ft.buffers()["state"][2, 0] = float("nan")
        res = ft.run()
        assert ft._nominal.launch_info()["per_wave"] == (2 if mode == "on" else 1)
        out.append((res, loop_buffers(ft, LOOP_BUFFERS_MASK)))
        ft.close()
    (_, off), (ron, on) = out
    for k in LOOP_BUFFERS_MASK:  # the partner (vehicle 3) and everybody else; NaNs compare equal
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    assert on["mask"][:, 2].tolist() == [1, 1]  # nominal solve, then the relaxed retry
    assert (on["status"][:, 2] == _lib.NUMERICAL_ERROR).all()
    assert ron.phase[2] == _lib.FLEET_ABORTED and ron.steps[2] == 0
    others = [v for v in range(V) if v != 2]
    assert (ron.phase[others] == _lib.FLEET_OUT_OF_STEPS).all() and (ron.steps[others] == steps).all()


def test_paired_warm_loop_longest_first_dispatch_order(cuda, golden):
    """More vehicles than wave slots, an odd number: the paired warm loop goes through the order table
    (slot 2 w + h -> order[slot]) and equals the unpaired warm loop bit for bit."""
    import torch
    from mpcqp.control.ref_builder import build_reference
    from mpcqp.pipeline.fleet import initial_states

    N, steps = 3, 4
    V = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    _, paths, starts, goals = varied_fleet(golden, V, seed=6)
    s0 = initial_states(paths, starts)
    out, refs = [], None
    for mode in ("off", "on"):
        ft = fleet_tracker(N, V, 128, steps, fused=True, warm_start=True, pairing=mode)
        if refs is None:  # varied_fleet cycles through 13 plans: one reference per plan, built once
            distinct = [build_reference(paths[i], ft.mpc.v_px_s, N, ft.mpc.dt) for i in range(13)]
            refs = [distinct[v % 13] for v in range(V)]
        ft.reset(refs, s0, goals)
        ft.run()
        info = ft._nominal.launch_info()
        assert (info["per_wave"], info["workgroups"]) == ((2, (V + 1) // 2) if mode == "on" else (1, V)), info
        out.append(loop_buffers(ft, LOOP_BUFFERS_MASK))
        ft.close()
    off, on = out
    assert (off["steps"] == steps).any()
    for k in LOOP_BUFFERS_MASK:
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)


# ---------------------------------------------------------------------- 3. the carried guess
def _golden_fleet(golden, V=4):
    g, path = default_plan(golden)
    plans = ([path] * V, np.tile(g["start"], (V, 1)), np.tile(g["goal"], (V, 1)))
    return plans, dict(sim_steps=100, map_resolution=float(g["map_resolution"]), fused=True, warm_start=True)


def _chunked(ft, plans, chunks, check_rows=False):
    """The run in launches of `chunks` steps, then the rest; the loop buffers at the end."""
    ft.reset_from_plans(*plans)
    for k in list(chunks) + [ft.max_steps]:
        ft.step(k)
        if check_rows:  # a row holds the last accepted U: its first column is the input applied last
            b = snap(ft, ("steps", "u_trace"))
            rows = ft.buffers()["U_carry"][:ft.vehicles].cpu().numpy()
            for v in range(ft.vehicles):
                np.testing.assert_array_equal(rows[v, :, 0], b["u_trace"][v, b["steps"][v] - 1], err_msg=f"chunk {k}, row {v}")
    out = loop_buffers(ft, LOOP_BUFFERS_MASK)
    ft.close()
    return out


@pytest.mark.parametrize("pairing", ["off", "on"])
def test_carried_guess_makes_a_split_run_the_single_launch(cuda, golden, pairing):
    """Launches of 1, 1, 5 steps and the rest over one carried buffer: the single mpcqp_fleet_loop_warm launch
    bit for bit, under the same pairing.  Without the carry the same chunking restarts cold four times."""
    from mpcqp import _lib

    N, V = 10, 4
    plans, kw = _golden_fleet(golden, V)
    kw["pairing"] = pairing
    _, single = run_loop(fleet_tracker(N, V, 64, **kw), *plans)
    assert (single["phase"][:V] == _lib.FLEET_GOAL).all()
    carried = _chunked(fleet_tracker(N, V, 64, carry_guess=True, **kw), plans, (1, 1, 5), check_rows=True)
    for k in LOOP_BUFFERS_MASK:
        np.testing.assert_array_equal(carried[k], single[k], err_msg=k)
    uncarried = _chunked(fleet_tracker(N, V, 64, **kw), plans, (1, 1, 5))
    print(f"pairing {pairing}: the same chunks without the carry land "
          f"{np.abs(uncarried['trace'] - single['trace']).max():.3e} px from the single launch (trace), "
          f"{np.abs(uncarried['u_trace'] - single['u_trace']).max():.3e} (u_trace)")


def test_nan_carry_in_one_launch_is_the_warm_loop(cuda, golden):
    """A NaN-filled carry (what every reset leaves) in one launch: mpcqp_fleet_loop_warm's buffers bit for bit,
    and the launch is recorded as the carrying one."""
    from mpcqp import _lib

    N, V = 10, 4
    plans, kw = _golden_fleet(golden, V)
    _, warm = run_loop(fleet_tracker(N, V, 64, **kw), *plans)
    ft = fleet_tracker(N, V, 64, carry_guess=True, **kw)
    ft.reset_from_plans(*plans)
    ft.run()
    info = ft._nominal.launch_info()
    assert info == dict(kind=_lib.LAUNCH_LOOP_WARM_CARRY, name="loop_warm_carry", per_wave=1, workgroups=V, count=V), info
    got = loop_buffers(ft, LOOP_BUFFERS_MASK)
    assert bool(ft.buffers()["U_carry"][:V].isfinite().all())
    ft.reset_from_plans(*plans)  # every reset starts without a guess
    assert bool(ft.buffers()["U_carry"][:V].isnan().all())
    ft.close()
    for k in LOOP_BUFFERS_MASK:
        np.testing.assert_array_equal(got[k], warm[k], err_msg=k)


@pytest.mark.parametrize("pairing", ["off", "on"])
def test_rows_of_vehicles_without_an_accepted_solve_stay(cuda, golden, pairing):
    """A vehicle at its goal at entry, and one that aborts at its first step (a NaN state), keep their rows."""
    from mpcqp import _lib

    N, V = 10, 4
    plans, kw = _golden_fleet(golden, V)
    ft = fleet_tracker(N, V, 64, carry_guess=True, pairing=pairing, **kw)
    ft.reset_from_plans(*plans)
    b = ft.buffers()
    b["U_carry"][:V] = 77.0
    b["phase"][0] = _lib.FLEET_GOAL
    b["state"][2, 0] = float("nan")
    ft.step(3)
    s = snap(ft, ("phase", "steps"))
    rows = b["U_carry"][:V].cpu().numpy()
    ft.close()
    assert s["phase"].tolist() == [_lib.FLEET_GOAL, _lib.FLEET_RUNNING, _lib.FLEET_ABORTED, _lib.FLEET_RUNNING]
    assert s["steps"].tolist() == [0, 3, 0, 3]
    assert (rows[[0, 2]] == 77.0).all()
    assert np.isfinite(rows[[1, 3]]).all() and (rows[[1, 3]] != 77.0).all()


@pytest.mark.parametrize("how", ["null_carry", "n40"])
def test_carry_call_errors_enqueue_and_invalidate_nothing(cuda, golden, how):
    import torch
    from mpcqp import scenarios

    N = 40 if how == "n40" else 10
    V = 4
    plans, kw = _golden_fleet(golden, V)
    ft = fleet_tracker(N, V, 64, carry_guess=True, **kw)
    ft.reset_from_plans(*plans)
    batch = scenarios.config3(V, horizon=N, seed=9)
    for ctrl in (ft._nominal, ft._relaxed):  # a build on each workspace, from before the call
        ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev)
    b = ft.buffers()
    b["status"].fill_(77)
    before = snap(ft, ("phase", "steps", "status", "state"))
    s = ctypes.c_void_p(torch.cuda.current_stream(ft.device).cuda_stream)
    carry = None if how == "null_carry" else b["U_carry"].data_ptr()
    rc = ft._L.mpcqp_fleet_loop_warm_carry(ft._nominal._ws, ft._relaxed._ws, ctypes.byref(ft._fleet), 3, 2, carry, s)
    assert rc == (E_ARG if how == "null_carry" else E_HORIZON), (how, rc, ft._L.mpcqp_last_error())
    after = snap(ft, ("phase", "steps", "status", "state"))
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert (after["status"] == 77).all() and bool(b["U_carry"][:V].isnan().all())
    for ctrl in (ft._nominal, ft._relaxed):  # both builds are still valid
        assert ctrl._L.mpcqp_solve(ctrl._ws, V, None, None, None, ctrl._status.data_ptr(), None, None, s) == 0
    torch.cuda.synchronize()
    ft.close()
