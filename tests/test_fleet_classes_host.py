"""CPU tests of the per-vehicle parameter classes in the fused fleet loop (``mpcqp_fleet_loop_mixed``,
``FleetTracker.set_classes`` / ``classes=``): the entry point in the header and the library, the
argument checks that come before any device call, the recorded resources of ``k_fleet_loop_mixed<N>``
and the host-side checks of ``FleetTracker``.  No GPU calls are made here."""
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


def test_header_declares_and_library_exports_the_mixed_loop():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_fleet_loop_mixed\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"const int32_t\* cls,\s+int steps,\s+void\* stream\);", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(handle, "mpcqp_fleet_loop_mixed"), "mpcqp_fleet_loop_mixed not exported"
    assert "mpcqp_fleet_loop_mixed" in _lib.exported_symbols()
    # exported_symbols() is still exactly what the header declares
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert "mpcqp_fleet_loop_mixed" in declared
    assert declared == set(_lib.exported_symbols())
    assert _lib.ABI_VERSION == 9
    # the limits a caller has to know are in the header: fused loop only, never paired, swarm unchanged
    doc = text[text.index("/* mpcqp_fleet_loop for a heterogeneous fleet"):text.index("int mpcqp_fleet_loop_mixed(")]
    assert "fused loop only" in doc and "MPCQP_E_HORIZON" in doc
    assert "Never paired" in doc
    assert "the swarm is unchanged" in doc
    assert "MPCQP_BAD_CLASS" in doc and "MPCQP_E_STATE" in doc
    # ... and the sentence about every other fleet and swarm call stands as it was
    assert "keep using the workspace's own block" in text


def test_mixed_loop_checks_its_arguments_before_the_device():
    """Null workspaces, a null fleet and a null cls are refused before anything touches a device."""
    _lib = _binding()
    L = _lib.lib()
    cls = (ctypes.c_int32 * 4)()
    f = _lib.MpcqpFleet()
    assert L.mpcqp_fleet_loop_mixed(None, None, ctypes.byref(f), ctypes.addressof(cls), 1, None) == E_ARG
    assert b"null argument" in L.mpcqp_last_error()
    assert L.mpcqp_fleet_loop_mixed(None, None, None, ctypes.addressof(cls), 1, None) == E_ARG
    assert L.mpcqp_fleet_loop_mixed(None, None, ctypes.byref(f), None, 1, None) == E_ARG
    assert b"null cls" in L.mpcqp_last_error()


def test_mixed_loop_kernel_resources():
    """k_fleet_loop_mixed<N> keeps k_fleet_loop<N>'s budget: two waves per SIMD, no AGPRs, eight
    workgroups of LDS per CU, and the scratch caps tests/test_host.py applies to ``loop:N`` (the body is
    the same; the kernel adds a table offset computed once)."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    mixed = {k: v for k, v in res.items() if k.startswith("loop_mixed:")}
    assert sorted(int(k.split(":")[1]) for k in mixed) == list(range(1, 33))
    for key, r in mixed.items():
        n = int(key.split(":")[1])
        print(key, r)
        assert r["Occupancy"] >= 2, (key, r)
        assert r["AGPRs"] == 0, (key, r)
        assert r["LDS"] <= 160 * 1024 // 8, (key, r)
        assert r["ScratchSize"] <= (640 if n == 32 else 512), (key, r)


def _bare_tracker(N=10, max_vehicles=8, num_classes=0, fused=True, dts=()):
    """A tracker object without workspaces (no device here): what the argument checks read."""
    import torch
    from types import SimpleNamespace

    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker

    t = object.__new__(FleetTracker)
    t._torch = torch
    t.device = torch.device("cpu")
    t.mpc = MPCConfig(horizon=N, sim_steps=5)
    t.params = t.mpc.to_parameters(0.8)
    t._ref_dt = float(t.mpc.dt)
    t.horizon, t.max_vehicles, t.max_ref_len = N, max_vehicles, 64
    t.fused = fused
    t.num_classes = num_classes
    t._class_params = [SimpleNamespace(dt=dt) for dt in dts] or None
    t._bufs = t._fleet = None
    return t


def _plan(V):
    paths = [np.array([[10.0 + v, 10.0], [40.0 + v, 12.0], [80.0 + v, 30.0]]) for v in range(V)]
    return paths, np.array([p[0] for p in paths]), np.array([p[-1] for p in paths])


def test_fleet_tracker_classes_argument_checks():
    import torch

    V = 4
    refs = [np.zeros((6, 4))] * V
    s0, goals = np.zeros((V, 4)), np.zeros((V, 2))
    # classes without a table: refused by reset, reset_device and reset_from_plans
    t = _bare_tracker()
    with pytest.raises(ValueError, match="set_classes"):
        t.reset(refs, s0, goals, classes=np.zeros(V, np.int32))
    with pytest.raises(ValueError, match="set_classes"):
        t.reset_device(torch.zeros((V, 64, 4), dtype=torch.float64), torch.full((V,), 6, dtype=torch.int32), s0, goals,
                       classes=np.zeros(V, np.int32))
    paths, starts, pgoals = _plan(V)
    with pytest.raises(ValueError, match="set_classes"):
        t.reset_from_plans(paths, starts, pgoals, classes=np.zeros(V, np.int32))
    # wrong shape, non-integer dtype
    t = _bare_tracker(num_classes=3, dts=(0.1, 0.1, 0.1))
    with pytest.raises(ValueError, match="shape"):
        t.reset(refs, s0, goals, classes=np.zeros(V + 1, np.int32))
    with pytest.raises(ValueError, match="shape"):
        t.reset(refs, s0, goals, classes=np.zeros((V, 1), np.int32))
    with pytest.raises(ValueError, match="integer"):
        t.reset(refs, s0, goals, classes=np.zeros(V))
    with pytest.raises(ValueError, match="integer"):
        t.reset(refs, s0, goals, classes=torch.zeros(V, dtype=torch.float32))
    # the stepped loop has no classes; neither has a horizon past the fused kernel
    with pytest.raises(ValueError, match="fused=True"):
        _bare_tracker(fused=False).set_classes([object()])
    with pytest.raises(ValueError, match="horizon <= 32"):
        _bare_tracker(N=33).set_classes([object()])
    # the batched reference builder takes one dt
    t = _bare_tracker(num_classes=2, dts=(0.1, 0.05))
    with pytest.raises(ValueError, match="one dt"):
        t.reset_from_plans(paths, starts, pgoals, device_reference=True, classes=np.array([0, 1, 0, 1]))


def test_fleet_tracker_class_indices_reach_the_device_as_int32():
    import torch

    t = _bare_tracker(num_classes=4, dts=(0.1, 0.05, 0.2, 0.1))
    V = 6
    for given in (np.array([0, 2, 1, -1, 3, 2**31 - 1], np.int64), [0, 2, 1, -1, 3, 2**31 - 1],
                  torch.tensor([0, 2, 1, -1, 3, 2**31 - 1], dtype=torch.int64)):
        c = t._class_indices(given, V)
        assert c.dtype == torch.int32 and c.is_contiguous()
        assert c.tolist() == [0, 2, 1, -1, 3, 2**31 - 1]
    assert t._class_indices(np.array([2**40, 1], np.int64), 2).tolist() == [-1, 1]  # no index: stays out of range
    # a table without classes=: every vehicle is class 0
    assert t._class_indices(None, 3).tolist() == [0, 0, 0]
    assert _bare_tracker()._class_indices(None, 3) is None
    # each vehicle's reference is built with its class's dt (the tracker's own where the index is no class)
    np.testing.assert_array_equal(t._class_dts(t._class_indices([0, 1, 2, 3, -1, 7], V), V),
                                  [0.1, 0.05, 0.2, 0.1, 0.1, 0.1])
    # reset() carries the indices into buffers()["cls"] (host tensors here: the bare tracker has no device)
    from mpcqp.control.ref_builder import build_reference

    paths, starts, goals = _plan(4)
    refs = t.reset_from_plans(paths, starts, goals, classes=np.array([1, 0, 2, 9], np.int64))
    assert t.buffers()["cls"].dtype == torch.int32 and t.buffers()["cls"].tolist() == [1, 0, 2, 9]
    for v, dt in enumerate([0.05, 0.1, 0.2, 0.1]):
        np.testing.assert_array_equal(refs[v], build_reference(paths[v], t.mpc.v_px_s, t.horizon, dt))
