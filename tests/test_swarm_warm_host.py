"""CPU tests of the warm start in the fused swarm (``k_swarm_loop_warm``, ``mpcqp_swarm_loop_warm``,
``Swarm(fused=True, warm_start=True)``): the entry point in the header and the library, its contract's
phrases, the argument checks that come before any device call, ``Swarm``'s own checks, and the recorded
resources of the new kernels.  No GPU calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest
from host_helpers import E_ARG
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"


def test_header_declares_and_library_exports_the_warm_swarm_call():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_swarm_loop_warm\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"const mpcqp_swarm\* s,\s+int guess_passes, void\* stream\);", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    assert _lib.ABI_VERSION == 9
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(handle, "mpcqp_swarm_loop_warm"), "mpcqp_swarm_loop_warm not exported"
    assert "mpcqp_swarm_loop_warm" in _lib.exported_symbols()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())
    # the contract a caller has to know is in the header
    doc = text[text.index("/* mpcqp_swarm_loop with every fused-loop launch warm"):text.index("int mpcqp_swarm_loop_warm(")]
    for phrase in ("bit for bit", "to rounding", "guess_passes <= 0", "first step", "MPCQP_E_HORIZON",
                   "no silent cold fallback"):
        assert phrase in doc, phrase
    # and what follows from "to rounding": a replanned vehicle's plan may differ from the cold swarm's
    for phrase in ("knife edges", "may differ", "MPCQP_PAIR_ON", "MPCQP_PAIR_AUTO", "MPCQP_LAUNCH_LOOP_WARM"):
        assert phrase in doc, phrase


def test_warm_swarm_call_checks_its_arguments_before_the_device():
    _lib = _binding()
    L = _lib.lib()
    st = (ctypes.c_int32 * 2)(77, 77)
    f = _lib.MpcqpFleet()
    f.status = ctypes.addressof(st)
    s = _lib.MpcqpSwarm()
    s.rrt.max_iterations, s.rrt.width, s.rrt.height = 10, 8, 8
    s.path_cap, s.horizon, s.dt, s.desired_speed = 16, 15, 0.1, 15.0
    # a null swarm, a null fleet, null workspaces: each refused, in this order, with nothing touched
    assert L.mpcqp_swarm_loop_warm(None, None, ctypes.byref(f), None, 8, None) == E_ARG
    assert b"null swarm" in L.mpcqp_last_error()
    assert L.mpcqp_swarm_loop_warm(None, None, None, ctypes.byref(s), 8, None) == E_ARG
    assert L.mpcqp_swarm_loop_warm(None, None, ctypes.byref(f), ctypes.byref(s), 8, None) == E_ARG
    # the swarm struct's checks are mpcqp_swarm_loop's: the same code for the same bad struct
    s.max_replans = -1
    assert L.mpcqp_swarm_loop_warm(None, None, ctypes.byref(f), ctypes.byref(s), 8, None) == E_ARG
    assert b"max_replans" in L.mpcqp_last_error()
    assert L.mpcqp_swarm_loop(None, None, ctypes.byref(f), ctypes.byref(s), None) == E_ARG
    assert list(st) == [77, 77]


def test_swarm_warm_argument_checks():
    """Raised before any workspace or planner is created: no device is needed to get them."""
    from mpcqp import _lib
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.swarm import Swarm
    from mpcqp.planning.rrt_star import default_planner_parameters

    occ = np.ones((8, 8), dtype=np.uint8)
    mpc = MPCConfig(horizon=15, sim_steps=5)
    kw = dict(map_resolution=0.8, max_vehicles=4)
    with pytest.raises(ValueError, match="fused=True"):
        Swarm(occ, mpc, default_planner_parameters(), warm_start=True, **kw)
    with pytest.raises(ValueError, match="warm_start=True"):
        Swarm(occ, mpc, default_planner_parameters(), fused=True, guess_passes=3, **kw)
    with pytest.raises(ValueError, match="warm_start=True"):
        Swarm(occ, mpc, default_planner_parameters(), guess_passes=3, **kw)
    assert Swarm.warm_start is False and Swarm.guess_passes == _lib.DEFAULT_GUESS_PASSES


def test_swarm_warm_kernel_resources():
    """k_swarm_loop_warm<N> (N = 1..32) and <N, true> (N = 1..15) keep the budget the other warm loops are
    held to (test_warm_pair_host.py): two waves per SIMD, no AGPRs, no more LDS than the paired carry loop,
    and the scratch of the cold loop of the same layout (k_fleet_loop<N>, k_fleet_loop<N, true>) plus at
    most 64 bytes."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    lds_cap = max(v["LDS"] for k, v in res.items() if k.startswith("loop_warm_carry_pair:"))
    for prefix, base, top in (("swarm_warm:", "loop:", 32), ("swarm_warm_pair:", "loop_pair:", 15)):
        own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith(prefix)}
        assert sorted(own) == list(range(1, top + 1)), prefix
        for n, r in own.items():
            b = res[f"{base}{n}"]
            print(f"{prefix}{n}", r, "base scratch", b["ScratchSize"])
            assert r["Occupancy"] >= 2, (prefix, n, r)
            assert r["AGPRs"] == 0, (prefix, n, r)
            assert r["LDS"] <= lds_cap, (prefix, n, r, lds_cap)
            assert r["ScratchSize"] <= b["ScratchSize"] + 64, (prefix, n, r, b)
    # the new keys are not selected by the prefixes the tests before them use
    for k in res:
        if k.startswith("swarm_warm"):
            assert not k.startswith(("pair:", "loop_pair:", "warm:", "loop_warm:", "loop:", "loop_warm_carry",
                                     "pair_warm:", "serve_warm:", "mixed:", "loop_mixed:")), k
