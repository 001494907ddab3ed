"""CPU tests of warm start at two QPs per wave and of the guess carried across launches
(``k_solve_pair_warm``, ``k_fleet_loop_warm_carry``, ``mpcqp_fleet_loop_warm_carry``, ``mpcqp_launch_info``):
the entry points in the header and the library, the argument checks that come before any device call, the
recorded resources of the new kernels, the tracker's checks, and the property of the inputs that the GPU
pattern test (tests/test_gpu_warm_pair.py) leans on.  No GPU calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest
import warm_newton as wn
from host_helpers import E_ARG
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"


def test_header_declares_and_library_exports_the_new_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_fleet_loop_warm_carry\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"int steps,\s+int guess_passes, double\* U_carry, void\* stream\);", text, re.M)
    assert re.search(r"^int mpcqp_launch_info\(const mpcqp_ws\* ws, int32_t info\[4\]\);", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    assert _lib.ABI_VERSION == 9
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("mpcqp_fleet_loop_warm_carry", "mpcqp_launch_info"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())
    # the launch kinds, in the header and in the binding
    kinds = dict(re.findall(r"^#define MPCQP_LAUNCH_([A-Z_]+) (\d+)$", text, re.M))
    assert kinds["NONE"] == "0" and len(set(kinds.values())) == len(kinds) == 8
    for name, value in kinds.items():
        assert getattr(_lib, f"LAUNCH_{name}") == int(value), name
    # the contract a caller has to know is in the header
    doc = text[text.index("/* mpcqp_fleet_loop_warm with the guess carried"):text.index("int mpcqp_fleet_loop_warm_carry(")]
    for phrase in ("bit for bit", "non-finite", "MPCQP_E_ARG", "MPCQP_E_HORIZON", "split", "guess_passes <= 0",
                   "left as they were", "MPCQP_PAIR_AUTO keeps one vehicle"):
        assert phrase in doc, phrase
    # the ON / OFF / AUTO rule of the two warm calls that were there
    doc = text[text.index(" * mpcqp_solve from a caller's guess"):text.index("int mpcqp_solve_warm(")]
    for phrase in ("MPCQP_PAIR_ON", "MPCQP_PAIR_OFF", "MPCQP_PAIR_AUTO keeps one QP per wave", "bit for bit"):
        assert phrase in doc, phrase
    doc = text[text.index("/* mpcqp_fleet_loop with a warm start"):text.index("int mpcqp_fleet_loop_warm(")]
    for phrase in ("MPCQP_PAIR_ON", "MPCQP_PAIR_OFF", "MPCQP_PAIR_AUTO keeps one vehicle per wave", "bit for bit"):
        assert phrase in doc, phrase
    doc = text[text.index("/* What the last solver launch"):text.index("#define MPCQP_LAUNCH_NONE")]
    for phrase in ("host bookkeeping", "MPCQP_E_ARG", "mpcqp_set_params"):
        assert phrase in doc, phrase


def test_new_calls_check_their_arguments_before_the_device():
    _lib = _binding()
    L = _lib.lib()
    st = (ctypes.c_int32 * 2)(77, 77)
    info = (ctypes.c_int32 * 4)(77, 77, 77, 77)
    buf = (ctypes.c_double * 8)()
    a = ctypes.addressof
    f = _lib.MpcqpFleet()
    f.status = a(st)
    assert L.mpcqp_fleet_loop_warm_carry(None, None, ctypes.byref(f), 1, 2, None, None) == E_ARG
    assert b"U_carry" in L.mpcqp_last_error()
    assert L.mpcqp_fleet_loop_warm_carry(None, None, ctypes.byref(f), 1, 2, a(buf), None) == E_ARG
    assert L.mpcqp_fleet_loop_warm_carry(None, None, None, 1, 2, a(buf), None) == E_ARG
    assert L.mpcqp_launch_info(None, info) == E_ARG
    assert b"null argument" in L.mpcqp_last_error()
    assert L.mpcqp_launch_info(a(buf), None) == E_ARG  # info is tested before ws is read
    assert list(st) == [77, 77] and list(info) == [77] * 4


def test_new_kernel_resources():
    """k_solve_pair_warm<N>, k_fleet_loop_warm_carry<N> and <N, true> keep the one-wave budget: two waves per
    SIMD, no AGPRs, eight workgroups of LDS per CU (20 KB), and the scratch of their cold counterparts
    (k_solve_pair<N>, k_fleet_loop<N>, k_fleet_loop<N, true>) plus at most 64 bytes: test_warm_kernel_resources'
    rule for the unpaired warm kernels."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    for prefix, base, top in (("pair_warm:", "pair:", 15), ("loop_warm_carry:", "loop:", 32),
                              ("loop_warm_carry_pair:", "loop_pair:", 15)):
        own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith(prefix)}
        assert sorted(own) == list(range(1, top + 1)), prefix
        for n, r in own.items():
            b = res[f"{base}{n}"]
            print(f"{prefix}{n}", r, "base scratch", b["ScratchSize"])
            assert r["Occupancy"] >= 2, (prefix, n, r)
            assert r["AGPRs"] == 0, (prefix, n, r)
            assert r["LDS"] <= 20480, (prefix, n, r)
            assert r["ScratchSize"] <= b["ScratchSize"] + 64, (prefix, n, r, b)
    # the new keys are not selected by the prefixes the tests before them use
    for k in res:
        if k.startswith(("pair_warm:", "loop_warm_carry")):
            assert not k.startswith(("pair:", "loop_pair:", "warm:", "loop_warm:", "loop:")), k


def test_fleet_tracker_carry_argument_checks():
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker

    mpc = MPCConfig(horizon=10, sim_steps=5)
    kw = dict(map_resolution=0.8, max_vehicles=4, max_ref_len=64)
    with pytest.raises(ValueError, match="carry_guess needs warm_start=True"):  # before any workspace is created
        FleetTracker(mpc, fused=True, carry_guess=True, **kw)
    with pytest.raises(ValueError, match="fused=True"):
        FleetTracker(mpc, warm_start=True, carry_guess=True, **kw)
    assert FleetTracker.carry_guess is False
    # a carrying tracker is a warm one: it takes no classes either
    t = object.__new__(FleetTracker)
    t.fused, t.horizon, t.warm_start, t.carry_guess = True, 10, True, True
    with pytest.raises(ValueError, match="warm_start"):
        t.set_classes([object()])


@pytest.mark.parametrize("N", [10, 15])
def test_zero_guess_misses_by_a_wide_margin(N):
    """The GPU pattern test gives its miss rows the zero guess with guess_passes = 2.  On the host model the
    Newton run from zeros needs at least 7 passes on every QP of the case (measured: 10..38 at N = 10,
    7..33 at N = 15), so two passes cannot hit; and the optima are clear of their bounds (15 of 16 at
    N = 10, all 16 at N = 15), so the exact guess does."""
    import mpc_oracle as mo
    from gpu_helpers import config3_case

    case = config3_case(N, 16, 5200 + N, margins=True)
    passes = []
    for b in range(16):
        qp = mo.condense(case["params"], case["x0"][b], case["ref"][b], case["u_prev"][b])
        r = wn.newton_from(qp, np.zeros((2, N)))
        assert r.converged, b
        passes.append(r.passes)
    print(f"N={N}: passes from zeros {sorted(passes)}; margins {np.sort(case['margins'])[:3]}")
    assert min(passes) >= 7, passes
    assert int((case["margins"] > wn.MARGIN).sum()) == (15 if N == 10 else 16)
