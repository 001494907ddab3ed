"""GPU tests of the warm start on the B = 1 path: ``mpcqp_solve_served_warm`` (the resident wave,
``k_serve_warm<N>``) and ``mpcqp_solve_staged_warm`` (one launch of ``k_solve_warm<N>``) from the
workspace's guess block (``mpcqp_stage_guess``), and the drop-in on top of them
(``BatchedMPCController.solve_one(U_guess=...)``, ``TrajectoryTracker(warm_start=True)``).

The contract is ``mpcqp_solve_warm``'s (include/mpcqp.h), so the yardsticks are the ones of
tests/test_gpu_warm.py: the batch warm solve of the same QP and guess (bit for bit, every output and the
counters), the cold B = 1 call of the same QP (bit for bit for an unusable guess), the exact oracle
(<= 1e-8 relative, equal active codes) where the host model ``warm_newton`` predicts a hit, and the
reference's own closed loop (closed_loop.npz, 1e-7).  Every test closes its controllers: no wave stays
resident behind it.
"""
from __future__ import annotations

import ctypes
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import warm_newton as wn
from gpu_helpers import (ATOL, E_HORIZON, E_STATE, OUTS, assert_exact, assert_same, base_params, config3_case, controller,
                         golden_case, is_live, take)

pytestmark = pytest.mark.gpu

def _one(ctrl, case, k, guess=None, passes=None):
    """All six outputs of one B = 1 solve of the case's QP k (from `guess` when given)."""
    kw = {} if guess is None else dict(U_guess=guess, guess_passes=passes)
    ctrl.solve_one(case["x0"][k], case["ref"][k], case["u_prev"][k], **kw)
    out = {n: ctrl._one[n].copy() for n in OUTS}
    assert np.array_equal(out["iters"], ctrl.last_iters)
    return out


def _shifted_golden_case(golden, N):
    """gpu_helpers.golden_case with the guesses a closed loop carries (``shifted``) as the case's guesses."""
    case = golden_case(golden, N)
    return dict(case, guesses=case["shifted"])


_BATCH = {}


def _batch(case, passes, key):
    """The batch API's answers for the whole case: mpcqp_solve_warm from the case's guesses
    (`passes` not None) or the cold mpcqp_solve; computed once per session."""
    k = (key, passes)
    if k not in _BATCH:
        ctrl = controller(case["params"], len(case["x0"]))
        kw = {} if passes is None else dict(U_guess=case["guesses"], guess_passes=passes)
        _BATCH[k] = take(ctrl.solve_batch(case["x0"], case["ref"], case["u_prev"], **kw))
        ctrl.close()
    return _BATCH[k]


# ---------------------------------------------------------------------- 1. served = staged = batch
@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("N", [10, 15])
def test_b1_warm_equals_the_batch_warm_solve_on_the_golden_windows(cuda, golden, monkeypatch, N, mode):
    """The 65 windows of the reference's closed loop from the guesses a closed loop carries (window k
    from window k - 1's optimum, shifted), with 1 and 8 passes: the launched (MPCQP_B1_SERVER=0) and the
    served B = 1 warm calls return mpcqp_solve_warm's outputs bit for bit, the counters included."""
    monkeypatch.setenv("MPCQP_B1_SERVER", mode)
    case = _shifted_golden_case(golden, N)
    ctrl = controller(case["params"], 1)
    hits = {}
    for passes in (1, 8):
        want = _batch(case, passes, ("golden", N))
        for k in range(len(case["x0"])):
            got = _one(ctrl, case, k, case["guesses"][k], passes)
            assert_same(got, {n: want[n][k] for n in OUTS}, f"N={N} mode {mode} passes {passes} window {k}")
        hits[passes] = int((want["iters"][:, 0] == 0).sum())
    assert is_live(ctrl) == (mode == "1")
    ctrl.close()
    print(f"N={N} mode {mode}: hits of 65 by passes {hits}")


@pytest.mark.parametrize("N", [1, 16, 24, 29, 32])
def test_b1_warm_equals_the_batch_warm_solve_from_exact_guesses(cuda, monkeypatch, N):
    """Exact guesses at N = 1 (nothing to shift), 16 (past the pair limit), 24 (packed Pbar), 29 (the
    spill range) and 32 (every lane a column), both B = 1 calls against the batch warm solve."""
    case = config3_case(N, 4, 6100 + N)
    want = _batch(case, 2, ("config3", N))
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCQP_B1_SERVER", mode)
        ctrl = controller(case["params"], 1)
        for k in range(len(case["x0"])):
            got = _one(ctrl, case, k, case["guesses"][k], 2)
            assert_same(got, {n: want[n][k] for n in OUTS}, f"N={N} mode {mode} QP {k}")
        ctrl.close()
    assert (want["status"] == 1).all()


# ---------------------------------------------------------------------- 2. unusable guesses
def _raw(ctrl, case, k, call, *args):
    """One B = 1 library call on the staged QP k without touching the guess block."""
    io = ctrl._one
    io["x0"][:] = case["x0"][k]
    io["ref"][:] = case["ref"][k]
    io["up"][:] = case["u_prev"][k]
    rc = getattr(ctrl._L, call)(ctrl._ws, *args)
    assert rc == 0, (call, rc, ctrl._L.mpcqp_last_error())
    return {n: io[n].copy() for n in OUTS}


@pytest.mark.parametrize("mode", ["0", "1"])
def test_unusable_guess_is_the_cold_b1_solve_bit_for_bit(cuda, golden, monkeypatch, mode):
    """A fresh guess block (all NaN), a NaN in one entry and guess_passes = 0: every output, iters
    included, is the cold call's (mpcqp_solve_served / mpcqp_solve_staged) of the same QP."""
    monkeypatch.setenv("MPCQP_B1_SERVER", mode)
    N = 10
    case = _shifted_golden_case(golden, N)
    cold_call, warm_call = (("mpcqp_solve_staged", "mpcqp_solve_staged_warm") if mode == "0"
                            else ("mpcqp_solve_served", "mpcqp_solve_served_warm"))
    ctrl = controller(case["params"], 1)
    ctrl._one = ctrl._stage()
    rows = (0, 7, 30, 64)
    cold = {k: _raw(ctrl, case, k, cold_call) for k in rows}
    assert all(cold[k]["status"][0] == 1 and cold[k]["iters"][0] > 0 for k in rows)
    block = ctrl._stage_guess()
    assert block.shape == (2, N) and np.isnan(block).all()  # fresh: NaN, so a solve before any write is cold
    for k in rows:
        assert_same(_raw(ctrl, case, k, warm_call, 8), cold[k], f"fresh block, window {k}")
    for k in rows:
        g = case["exact"][k].Umat.copy()
        g[1, N - 1] = np.nan  # the last steering angle
        assert_same(_one(ctrl, case, k, g, 8), cold[k], f"NaN entry, window {k}")
        for passes in (0, -3):
            assert_same(_one(ctrl, case, k, case["exact"][k].Umat, passes), cold[k], f"passes {passes}, window {k}")
    # and the same block, usable: a hit
    out = _one(ctrl, case, rows[1], case["exact"][rows[1]].Umat, 8)
    assert out["status"][0] == 1 and out["iters"][0] == 0
    ctrl.close()


# ---------------------------------------------------------------------- 3. hits where the host model says so
@pytest.mark.parametrize("N", [10, 15])
def test_served_warm_hits_where_the_host_model_converges_in_one_pass(cuda, golden, monkeypatch, N):
    monkeypatch.setenv("MPCQP_B1_SERVER", "1")
    case = _shifted_golden_case(golden, N)
    runs = case["shifted_runs"]
    expected = [k for k in range(1, len(runs)) if runs[k].passes == 1 and runs[k].margin > wn.MARGIN]
    assert len(expected) >= 25
    ctrl = controller(case["params"], 1)
    for k in expected:
        out = _one(ctrl, case, k, case["guesses"][k])
        ex = case["exact"][k]
        assert out["status"][0] == 1, (N, k, out["status"])
        assert out["iters"][0] == 0 and out["iters"][1] == 1, (N, k, out["iters"])
        assert_exact(out, None, ex, f"N={N} window {k}", solved=True)
    ctrl.close()


# ---------------------------------------------------------------------- 4. the closed loop
def _close_cache():
    from mpcqp.control import mpc_controller as mc

    while mc._CACHE:
        mc._CACHE.popitem()[1].close()


@pytest.mark.parametrize("N,sim_steps", [(10, 100), (15, 300)])
def test_warm_tracker_reproduces_the_reference_closed_loop(cuda, golden, N, sim_steps):
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.pipeline.control_stage import TrajectoryTracker

    g = golden("default_plan.npz")
    planning = SimpleNamespace(plan=SimpleNamespace(success=True, path=[tuple(map(float, p)) for p in g["path"]]))
    maps = SimpleNamespace(start=tuple(g["start"]), goal=tuple(g["goal"]))
    tracker = TrajectoryTracker(MPCConfig(horizon=N, sim_steps=sim_steps), VizConfig(), warm_start=True)
    try:
        result = tracker.track(planning, maps, map_resolution=float(g["map_resolution"]), visualize=False)
    finally:
        _close_cache()
    states = np.asarray(result.states)
    ref_states = golden("closed_loop.npz")[f"N{N}_states"]
    assert states.shape == ref_states.shape == (65, 4)
    print(f"N={N}: max |state - golden| {np.abs(states - ref_states).max():.3e}, "
          f"{tracker.warm_hits} hits of {tracker.warm_attempts} attempts")
    np.testing.assert_allclose(states, ref_states, rtol=0, atol=ATOL)
    assert tracker.warm_attempts == 64
    assert tracker.warm_hits >= 25


# ---------------------------------------------------------------------- 5. the server's lifecycle
def _launched(case, rows, monkeypatch):
    """The launched counterparts (MPCQP_B1_SERVER=0) of the rows' cold and warm (exact guess, 2 passes) solves."""
    monkeypatch.setenv("MPCQP_B1_SERVER", "0")
    ctrl = controller(case["params"], 1)
    cold = {k: _one(ctrl, case, k) for k in rows}
    warm = {k: _one(ctrl, case, k, case["guesses"][k], 2) for k in rows}
    ctrl.close()
    monkeypatch.setenv("MPCQP_B1_SERVER", "1")
    return cold, warm


def test_cold_and_warm_served_calls_alternate_on_one_workspace(cuda, monkeypatch):
    """A workspace has one resident wave, of the kind of its last served call: every answer equals its
    launched counterpart, whichever kind served before."""
    case = config3_case(16, 4, 6100 + 16)
    rows = range(len(case["x0"]))
    cold, warm = _launched(case, rows, monkeypatch)
    ctrl = controller(case["params"], 1)
    for rep, kinds in enumerate(("cw", "wc", "wwcc")):
        for i, kind in enumerate(kinds * 2):
            k = (rep + i) % len(case["x0"])
            if kind == "c":
                assert_same(_one(ctrl, case, k), cold[k], f"cold {rep}.{i}")
            else:
                assert_same(_one(ctrl, case, k, case["guesses"][k], 2), warm[k], f"warm {rep}.{i}")
            assert is_live(ctrl)
    assert all(warm[k]["iters"][0] == 0 for k in rows) and all(cold[k]["iters"][0] > 0 for k in rows)
    ctrl.close()


def test_two_workspaces_alternate_warm_calls(cuda, monkeypatch):
    """The drop-in's nominal and relaxed workspaces, both warm: a switch stops the other workspace's wave."""
    case = config3_case(16, 4, 6100 + 16)
    nominal = case["params"]
    du = nominal.du_bounds
    relaxed = dataclasses.replace(nominal, du_bounds=((du[0][0] - 5.0, du[0][1] + 5.0),
                                                      (du[1][0] - 0.05, du[1][1] + 0.05)))
    cases = [case, dict(case, params=relaxed)]
    rows = range(len(case["x0"]))
    want = [_launched(c, rows, monkeypatch)[1] for c in cases]
    ctrls = [controller(c["params"], 1) for c in cases]
    for i in range(12):
        w, k = i % 2 if i % 5 else 0, i % len(case["x0"])
        assert_same(_one(ctrls[w], cases[w], k, case["guesses"][k], 2), want[w][k], f"call {i} workspace {w}")
        live = [is_live(c) for c in ctrls]
        assert live[w] and sum(live) == 1, (i, live)
    for c in ctrls:
        c.close()


def test_served_warm_failure_paths_and_set_params(cuda, monkeypatch):
    """A wave that left unannounced is relaunched by the next warm request; a refused launch fails the
    warm call (LibraryError) and the next one succeeds; mpcqp_set_params between warm calls stops the wave."""
    from mpcqp import _lib

    case = config3_case(16, 4, 6100 + 16)
    rows = range(len(case["x0"]))
    _, warm = _launched(case, rows, monkeypatch)
    ctrl = controller(case["params"], 1)
    L = ctrl._L

    def check(k):
        assert_same(_one(ctrl, case, k, case["guesses"][k], 2), warm[k], f"QP {k}")
        assert is_live(ctrl)

    check(0)
    assert L.mpcqp_debug_serve_fault(ctrl._ws, 2) == 0  # the wave leaves; the host still believes it resident
    assert is_live(ctrl)
    check(1)
    assert L.mpcqp_debug_serve_fault(ctrl._ws, 2) == 0
    assert L.mpcqp_debug_serve_fault(ctrl._ws, 1) == 0
    with pytest.raises(_lib.LibraryError, match="refused"):
        _one(ctrl, case, 2, case["guesses"][2], 2)
    check(2)
    ctrl.set_params(case["params"])
    assert not is_live(ctrl)
    check(3)
    ctrl.close()


# ---------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("how", ["n40", "reproducible", "debug_state", "no_guess_block"])
def test_b1_warm_refusals_write_nothing(cuda, how):
    from mpcqp import scenarios

    N = 40 if how == "n40" else 10
    b = scenarios.config3(1, horizon=N, seed=11)
    ctrl = controller(base_params(N), 1,
                      **{"reproducible": dict(reproducible=1), "debug_state": dict(debug_state=1)}.get(how, {}))
    io = ctrl._one = ctrl._stage()
    if how != "no_guess_block":
        ctrl._stage_guess()[:] = 0.0
    io["x0"][:], io["ref"][:], io["up"][:] = b.x0[0], b.ref[0], b.u_prev[0]
    io["status"][0] = 77
    want = E_STATE if how == "no_guess_block" else E_HORIZON
    for call in ("mpcqp_solve_staged_warm", "mpcqp_solve_served_warm"):
        assert getattr(ctrl._L, call)(ctrl._ws, 2) == want, (how, call, ctrl._L.mpcqp_last_error())
        assert io["status"][0] == 77
        assert not is_live(ctrl)
    assert ctrl._L.mpcqp_solve_served(ctrl._ws) == 0  # the cold call still runs on this workspace
    assert io["status"][0] != 77
    ctrl.close()


def test_stage_guess_needs_the_staging_blocks(cuda):
    ctrl = controller(base_params(10), 1)
    g = ctypes.c_void_p(77)
    assert ctrl._L.mpcqp_stage_guess(ctrl._ws, ctypes.byref(g)) == E_STATE
    assert g.value == 77
    ctrl._one = ctrl._stage()
    a, b = ctrl._stage_guess(), ctrl._stage_guess()
    assert a.ctypes.data == b.ctypes.data  # allocated once
    ctrl.close()
