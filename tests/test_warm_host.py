"""CPU tests of the warm start (``mpcqp_solve_warm``, ``mpcqp_fleet_loop_warm``): the entry points in
the header and the library, the recorded resources of ``k_solve_warm<N>`` / ``k_fleet_loop_warm<N>``, the
premise on the reference's own closed loops (a Newton run from the previous optimum, ``warm_newton``),
and the argument checks of ``solve_batch`` and ``FleetTracker`` that come before any device call.  No GPU
calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest
import warm_newton as wn
from host_helpers import E_ARG
from host_helpers import bare_controller as _bare_controller
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"


def test_header_declares_and_library_exports_the_warm_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_solve_warm\(mpcqp_ws\* ws, int B, const double\* U_guess, int guess_passes, "
                     r"double\* u0, double\* X, double\* U,\s+int32_t\* status, int32_t\* iters, uint8_t\* active, "
                     r"void\* stream\);", text, re.M)
    assert re.search(r"^int mpcqp_fleet_loop_warm\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"int steps, int guess_passes,\s+void\* stream\);", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    assert _lib.ABI_VERSION == 9
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("mpcqp_solve_warm", "mpcqp_fleet_loop_warm"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())
    assert isinstance(_lib.DEFAULT_GUESS_PASSES, int) and _lib.DEFAULT_GUESS_PASSES >= 1
    # the contract a caller has to know is in the header
    doc = text[text.index(" * mpcqp_solve from a caller's guess"):text.index("int mpcqp_solve_warm(")]
    for phrase in ("unusable", "bit for bit", "iters[0] == 0", "miss", "MPCQP_E_STATE", "MPCQP_E_HORIZON",
                   "MPCQP_E_ARG", "to rounding", "may be the U output itself"):
        assert phrase in doc, phrase
    doc = text[text.index("/* mpcqp_fleet_loop with a warm start"):text.index("int mpcqp_fleet_loop_warm(")]
    for phrase in ("restarts cold at each launch", "guess_passes <= 0", "bit for bit", "to rounding",
                   "MPCQP_E_HORIZON"):
        assert phrase in doc, phrase


def test_warm_calls_check_their_arguments_before_the_device():
    _lib = _binding()
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    st = (ctypes.c_int32 * 2)(77, 77)
    a = ctypes.addressof
    assert L.mpcqp_solve_warm(None, 1, a(buf), 2, None, None, None, a(st), None, None, None) == E_ARG
    assert b"null argument" in L.mpcqp_last_error()
    f = _lib.MpcqpFleet()
    assert L.mpcqp_fleet_loop_warm(None, None, ctypes.byref(f), 1, 2, None) == E_ARG
    assert L.mpcqp_fleet_loop_warm(None, None, None, 1, 2, None) == E_ARG
    assert list(st) == [77, 77]


def test_warm_kernel_resources():
    """k_solve_warm<N> and k_fleet_loop_warm<N> keep the one-wave budget: two waves per SIMD, no AGPRs, eight
    workgroups of LDS per CU (20 KB), and the scratch of k_solve<N> / k_fleet_loop<N> plus at most 64 bytes
    (the carried guess and the attempt's flags)."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    for prefix, base in (("warm:", ""), ("loop_warm:", "loop:")):
        own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith(prefix)}
        assert sorted(own) == list(range(1, 33)), prefix
        for n, r in own.items():
            b = res[f"{base}{n}"]
            print(f"{prefix}{n}", r, "base scratch", b["ScratchSize"])
            assert r["Occupancy"] >= 2, (prefix, n, r)
            assert r["AGPRs"] == 0, (prefix, n, r)
            assert r["LDS"] <= 20 * 1024, (prefix, n, r)
            assert r["ScratchSize"] <= b["ScratchSize"] + 64, (prefix, n, r, b)


def _params(golden, N):
    import mpc_oracle as mo

    return mo.default_params(N, float(golden("default_plan.npz")["map_resolution"]))


@pytest.mark.parametrize("N", [10, 15])
def test_exact_guess_converges_in_one_pass_on_the_golden_windows(golden, N):
    """From a window's exact optimum the Newton run reproduces the active set at once, and every row
    of every optimum is clear of its bounds: the GPU test may hold all 65 windows to the counters."""
    w = wn.golden_windows(golden("closed_loop.npz"), _params(golden, N), N)
    assert len(w["exact"]) == 65
    for k, (qp, ex) in enumerate(zip(w["qps"], w["exact"])):
        assert ex.converged
        r = wn.newton_from(qp, ex.Umat)
        assert r.converged and r.passes == 1, (k, r.passes)
        assert np.abs(r.U - ex.U).max() <= 1e-9 * max(1.0, np.abs(ex.U).max())
        assert np.array_equal(r.codes, ex.active)
    assert (w["margins"] > wn.MARGIN).all(), w["margins"].min()


@pytest.mark.parametrize("N", [10, 15])
def test_shifted_guess_converges_in_one_pass_often_enough(golden, N):
    """The previous window's optimum, shifted one step, is in the optimum's active set on a good share
    of the loop (measured: 29 of 64 at N = 10, 30 at N = 15): the GPU test's hit subset is not empty."""
    w = wn.golden_windows(golden("closed_loop.npz"), _params(golden, N), N)
    runs = w["shifted_runs"][1:]
    assert len(runs) == 64 and all(r.converged for r in runs)
    for k, r in enumerate(runs, start=1):  # wherever it started, the run ends at the window's optimum
        assert np.array_equal(r.codes, w["exact"][k].active), k
        assert np.abs(r.U - w["exact"][k].U).max() <= 1e-8 * max(1.0, np.abs(r.U).max()), k
    one = sum(r.passes == 1 and r.margin > wn.MARGIN for r in runs)
    print(f"N={N}: 1 pass with margin on {one} of 64; passes {sorted(r.passes for r in runs)}")
    assert one >= 25, one


def test_shifted_guess_layout():
    U = np.arange(8.0).reshape(2, 4)
    np.testing.assert_array_equal(wn.shifted(U), [[1, 2, 3, 3], [5, 6, 7, 7]])
    np.testing.assert_array_equal(wn.shifted(U[:, :1]), U[:, :1])  # N = 1: nothing to shift


def test_solve_batch_guess_argument_checks():
    B, N = 4, 10
    c = _bare_controller(N, num_classes=2)
    x0, ref = np.zeros((B, 4)), np.zeros((B, N + 1, 4))
    with pytest.raises(ValueError, match="classes"):
        c.solve_batch(x0, ref, U_guess=np.zeros((B, 2, N)), classes=np.zeros(B, np.int32))
    c = _bare_controller(N)
    with pytest.raises(ValueError, match="shape"):
        c.solve_batch(x0, ref, U_guess=np.zeros((B, N, 2)))
    with pytest.raises(ValueError, match="shape"):
        c.solve_batch(x0, ref, U_guess=np.zeros((B + 1, 2, N)))
    with pytest.raises(ValueError, match="needs U_guess"):
        c.solve_batch(x0, ref, guess_passes=2)


def test_fleet_tracker_warm_argument_checks():
    from mpcqp import _lib
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker

    mpc = MPCConfig(horizon=10, sim_steps=5)
    kw = dict(map_resolution=0.8, max_vehicles=4, max_ref_len=64)
    with pytest.raises(ValueError, match="fused=True"):  # raised before any workspace is created
        FleetTracker(mpc, warm_start=True, **kw)
    with pytest.raises(ValueError, match="warm_start=True"):
        FleetTracker(mpc, fused=True, guess_passes=3, **kw)
    # a warm tracker takes no classes
    t = object.__new__(FleetTracker)
    t.fused, t.horizon, t.warm_start = True, 10, True
    with pytest.raises(ValueError, match="warm_start"):
        t.set_classes([object()])
    assert FleetTracker.warm_start is False and FleetTracker.guess_passes == _lib.DEFAULT_GUESS_PASSES
