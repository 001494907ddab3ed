"""CPU tests of the warm start on the B = 1 path (``mpcqp_stage_guess``, ``mpcqp_solve_staged_warm``,
``mpcqp_solve_served_warm``; ``k_serve_warm<N>``): the entry points in the header and the library, the
recorded resources of the new server kernel, and the host logic of the drop-in -- ``MPCController``'s
``u_init`` and ``TrajectoryTracker``'s carried guess -- against a stub ``solve_one`` that records its
arguments and answers from the C restatement.  No GPU calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import warm_newton as wn
from host_helpers import E_ARG
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"
CALLS = ("mpcqp_stage_guess", "mpcqp_solve_staged_warm", "mpcqp_solve_served_warm")


def test_header_declares_and_library_exports_the_b1_warm_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_stage_guess\(mpcqp_ws\* ws, double\*\* guess\);", text, re.M)
    assert re.search(r"^int mpcqp_solve_staged_warm\(mpcqp_ws\* ws, int guess_passes\);", text, re.M)
    assert re.search(r"^int mpcqp_solve_served_warm\(mpcqp_ws\* ws, int guess_passes\);", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    assert _lib.ABI_VERSION == 9
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in CALLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())
    # the contract a caller has to know is in the header
    doc = text[text.index(" * The B = 1 path from a caller's guess"):text.index("int mpcqp_stage_guess(")]
    for phrase in ("MPCQP_E_STATE", "MPCQP_E_HORIZON", "MPCQP_E_ARG", "bit for bit", "iters[0] == 0", "NaN",
                   "no silent cold fallback", "`out` block's U", "mpcqp_destroy", "mpcqp_set_params",
                   "of the other kind"):
        assert phrase in doc, phrase


def test_b1_warm_calls_refuse_a_null_workspace():
    _lib = _binding()
    L = _lib.lib()
    guess = ctypes.c_void_p(77)
    assert L.mpcqp_stage_guess(None, ctypes.byref(guess)) == E_ARG
    assert b"null" in L.mpcqp_last_error()
    assert guess.value == 77  # the caller's pointer is untouched
    assert L.mpcqp_solve_staged_warm(None, 2) == E_ARG
    assert L.mpcqp_solve_served_warm(None, 2) == E_ARG
    assert b"null ws" in L.mpcqp_last_error()


def test_serve_warm_kernel_resources():
    """k_serve_warm<N> is recorded for every one-wave horizon; one resident wave has the whole register
    file, so its scratch is no larger than k_solve_warm<N>'s at two waves per SIMD, and its LDS is the
    solver block (<= 20 KB)."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith("serve_warm:")}
    assert sorted(own) == list(range(1, 33))
    for n, r in own.items():
        b = res[f"warm:{n}"]
        print(f"serve_warm:{n}", r, "warm scratch", b["ScratchSize"])
        assert r["LDS"] <= 20 * 1024, (n, r)
        assert r["ScratchSize"] <= b["ScratchSize"], (n, r, b)


# ---------------------------------------------------------------------- the drop-in's host logic
class _Stub:
    """Stand-in for the B = 1 device controller with the warm ``solve_one`` signature: records each call's
    guess and answers from the C restatement (a cold solve: the answer does not depend on the guess).
    ``fail_at``: call numbers answered with a numerical error; ``hit``: report a guess as a hit."""

    def __init__(self, params, log, fail_at=(), hit=False, **settings):
        self.params, self.settings, self.log, self.fail_at, self.hit = params, settings, log, set(fail_at), hit
        self.last_iters = None
        self._cparams = SimpleNamespace(scaling=10, method=0)  # no re-solve under OSQP's scaling (_unpolished_fallback)

    def solve_one(self, x0, ref, u_prev=None, *, U_guess=None, guess_passes=None):
        import cpu_solver

        up = np.zeros((1, 2)) if u_prev is None else np.asarray(u_prev, float).reshape(1, 2)
        out = cpu_solver.cpu_solve(self.params, np.asarray(x0, float).reshape(1, 4),
                                   np.asarray(ref, float)[None], up, nthreads=1, **self.settings)
        n = len(self.log)
        status = -10 if n in self.fail_at else int(out["status"][0])
        self.log.append(SimpleNamespace(guess=None if U_guess is None else np.array(U_guess, copy=True),
                                        passes=guess_passes, U=out["U"][0].copy(), status=status,
                                        wheelbase=float(self.params.wheelbase_px), du=self.params.du_bounds))
        self.last_iters = out["iters"][0].copy()
        if self.hit and U_guess is not None:
            self.last_iters[0] = 0
        return status, out["u0"][0].copy(), out["X"][0].copy(), out["U"][0].copy()


class _ColdStub(_Stub):
    """Today's three-argument ``solve_one``: a guess handed to it is a TypeError."""

    def solve_one(self, x0, ref, u_prev=None):  # noqa: D102
        return _Stub.solve_one(self, x0, ref, u_prev)


def _patch(monkeypatch, cls=_Stub, **kw):
    import mpcqp.control.mpc_controller as mc

    log, keys = [], []

    def single(params, method="admm", **settings):
        keys.append(dict(settings))
        return cls(params, log, **kw, **settings)

    monkeypatch.setattr(mc, "_single_controller", single)
    return log, keys


def _plan(golden):
    g = golden("default_plan.npz")
    planning = SimpleNamespace(plan=SimpleNamespace(success=True, path=[tuple(map(float, p)) for p in g["path"]]))
    maps = SimpleNamespace(start=tuple(g["start"]), goal=tuple(g["goal"]))
    return float(g["map_resolution"]), planning, maps


def test_tracker_carries_the_shifted_guess_along_the_golden_loop(golden, monkeypatch):
    """track() on the golden plan at N = 10: the first step is cold, step k + 1 receives exactly
    shifted(U_k) with the tracker's guess_passes, the loop is the golden one, and a new track() starts
    cold again."""
    from mpcqp import _lib
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.pipeline.control_stage import TrajectoryTracker

    log, keys = _patch(monkeypatch, hit=True)
    res, planning, maps = _plan(golden)
    loop = golden("closed_loop.npz")
    t = TrajectoryTracker(MPCConfig(horizon=10, sim_steps=100), VizConfig(), warm_start=True)
    assert t.guess_passes is None and t.warm_attempts == 0 and t.warm_hits == 0
    states = np.asarray(t.track(planning, maps, map_resolution=res, visualize=False).states)
    np.testing.assert_allclose(states, loop["N10_states"], rtol=0, atol=1e-7)
    assert len(log) == 65
    assert log[0].guess is None
    for k in range(64):
        g = log[k + 1].guess
        assert g is not None and g.shape == (2, 10), k
        np.testing.assert_array_equal(g, wn.shifted(log[k].U), err_msg=f"step {k + 1}")
        assert log[k + 1].passes == _lib.DEFAULT_GUESS_PASSES
    assert t.warm_attempts == 64 and t.warm_hits == 64  # the stub reports every guess as a hit
    # neither new name is a solver setting: nothing of them reaches the controller cache's key
    assert all("warm_start" not in k and "guess_passes" not in k for k in keys)
    # a new run starts cold
    t.mpc = MPCConfig(horizon=10, sim_steps=3)
    t.guess_passes = 3
    del log[:]
    t.track(planning, maps, map_resolution=res, visualize=False)
    assert len(log) == 3 and log[0].guess is None
    np.testing.assert_array_equal(log[1].guess, wn.shifted(log[0].U))
    assert log[1].passes == 3
    assert t.warm_attempts == 66


def test_tracker_clears_the_guess_after_a_failed_step(golden, monkeypatch):
    """The relaxed retry of a step gets the same guess as its nominal solve; a step that stays unsolved
    returns (None, None, None) and the next one is cold."""
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.pipeline.control_stage import TrajectoryTracker

    # calls: 0 step 0 (cold) | 1 step 1 nominal fails, 2 its retry | 3 step 2 nominal fails, 4 retry fails | 5 step 3
    log, _ = _patch(monkeypatch, fail_at=(1, 3, 4))
    loop = golden("closed_loop.npz")
    t = TrajectoryTracker(MPCConfig(horizon=10), VizConfig(), warm_start=True, guess_passes=2)
    args = [(loop["N10_x0"][k], loop["N10_window"][k], loop["N10_u_prev"][k]) for k in range(4)]
    assert t.step(*args[0])[0] is not None
    assert t.step(*args[1])[0] is not None
    assert log[1].guess is not None and log[1].du != log[2].du  # nominal, then the relaxed block
    np.testing.assert_array_equal(log[1].guess, wn.shifted(log[0].U))
    np.testing.assert_array_equal(log[2].guess, log[1].guess)
    assert t.step(*args[2]) == (None, None, None)
    np.testing.assert_array_equal(log[3].guess, wn.shifted(log[2].U))  # the accepted (relaxed) solve's U
    np.testing.assert_array_equal(log[4].guess, log[3].guess)
    assert t.step(*args[3])[0] is not None
    assert log[5].guess is None
    assert all(c.passes == 2 for c in log if c.guess is not None)
    assert t.warm_attempts == 4 and t.warm_hits == 0  # cold answers: iters[0] > 0


def test_cold_tracker_and_controller_never_hand_over_a_guess(golden, monkeypatch):
    """warm_start=False (the default): today's three-argument solve_one is all the drop-in calls, and
    u_init stays ignored whatever its shape."""
    import mpcqp.control.mpc_controller as mc
    from mpcqp.config import MPCConfig, VizConfig
    from mpcqp.pipeline.control_stage import TrajectoryTracker

    log, _ = _patch(monkeypatch, cls=_ColdStub)
    loop = golden("closed_loop.npz")
    t = TrajectoryTracker(MPCConfig(horizon=10), VizConfig())
    assert t.warm_start is False
    for k in range(3):
        assert t.step(loop["N10_x0"][k], loop["N10_window"][k], loop["N10_u_prev"][k])[0] is not None
    assert t.warm_attempts == 0 and t._carried_U is None
    c = mc.MPCController(t.mpc.to_parameters(0.8))
    u0, X, U = c.solve(loop["N10_x0"][0], loop["N10_window"][0], u_init=np.zeros((3, 7)), u_prev=loop["N10_u_prev"][0])
    assert u0 is not None and len(log) == 4 and all(e.guess is None for e in log)
    assert c.last_iters is not None and len(c.last_iters) == 4


def test_controller_u_init_layout_and_argument_checks(golden, monkeypatch):
    import dataclasses

    import mpcqp.control.mpc_controller as mc
    from mpcqp.config import MPCConfig

    log, keys = _patch(monkeypatch)
    loop = golden("closed_loop.npz")
    params = MPCConfig(horizon=10).to_parameters(0.8)
    x0, win, up = loop["N10_x0"][5], loop["N10_window"][5], loop["N10_u_prev"][5]
    c = mc.MPCController(params, warm_start=True, guess_passes=4, max_iter=500)
    G = np.arange(20.0).reshape(10, 2)  # the reference's layout: a row per step
    assert c.solve(x0, win, u_init=G, u_prev=up)[0] is not None
    np.testing.assert_array_equal(log[-1].guess, G.T)
    assert log[-1].passes == 4 and keys[-1] == {"max_iter": 500}
    assert c.solve(x0, win, u_prev=up)[0] is not None  # u_init=None: cold
    assert log[-1].guess is None
    for bad in (np.zeros((2, 10)), np.zeros(20), np.zeros((11, 2))):
        with pytest.raises(ValueError, match=r"u_init must have shape \(10, 2\)"):
            c.solve(x0, win, u_init=bad, u_prev=up)
    with pytest.raises(ValueError, match="horizon <= 32"):
        mc.MPCController(dataclasses.replace(params, horizon=33), warm_start=True)
    mc.MPCController(dataclasses.replace(params, horizon=32), warm_start=True)
    mc.MPCController(dataclasses.replace(params, horizon=40))  # cold: any horizon, as before


def test_unpolished_resolve_gets_the_same_guess(golden, monkeypatch):
    """A solve that does not end at the polished optimum is repeated under OSQP's scaling: with the same guess."""
    import mpcqp.control.mpc_controller as mc
    from mpcqp.config import MPCConfig

    log, keys = _patch(monkeypatch)
    monkeypatch.setattr(mc, "_unpolished_fallback", lambda ctrl: True)
    loop = golden("closed_loop.npz")
    params = MPCConfig(horizon=10).to_parameters(0.8)
    c = mc.MPCController(params, warm_start=True, max_iter=5, polish_from=0, polish_near=0.0)
    G = np.full((10, 2), 0.25)
    c.solve(loop["N10_x0"][0], loop["N10_window"][0], u_init=G, u_prev=loop["N10_u_prev"][0])
    assert len(log) == 2 and log[0].status != 1
    assert keys[1]["scaling"] == 10 and "scaling" not in keys[0]
    np.testing.assert_array_equal(log[0].guess, G.T)
    np.testing.assert_array_equal(log[1].guess, G.T)


def test_solve_one_guess_argument_checks():
    """What solve_one checks before any device call."""
    from mpcqp.control.mpc_controller import BatchedMPCController

    c = object.__new__(BatchedMPCController)
    c.horizon = 10
    c._one = dict(x0=np.zeros(4), ref=np.zeros((11, 4)), up=np.zeros(2))
    c._solve1 = c._solve1_warm = None
    with pytest.raises(ValueError, match="needs U_guess"):
        c.solve_one(np.zeros(4), np.zeros((11, 4)), guess_passes=2)
    for bad in (np.zeros((10, 2)), np.zeros((2, 11)), np.zeros(20)):
        with pytest.raises(ValueError, match=r"U_guess must have shape \(2, 10\)"):
            c.solve_one(np.zeros(4), np.zeros((11, 4)), U_guess=bad)
    c._one = None
    assert c.last_iters is None  # before the first solve
    c._one = dict(iters=np.arange(4, dtype=np.int32))
    it = c.last_iters
    it[0] = 9  # a copy: the block is untouched
    assert c.last_iters.tolist() == [0, 1, 2, 3]
