"""CPU tests of the parameter classes in the fused swarm (``k_swarm_loop_mixed``, ``k_swarm_loop_mixed_warm``,
``mpcqp_swarm_loop_mixed``, ``mpcqp_swarm_loop_mixed_warm``, ``Swarm.set_classes`` / ``run(classes=)``): the entry
points in the header and the library, their contract's phrases, the argument checks that come before any
device call, the recorded resources of the new kernels, ``Swarm``'s own checks on a bare object, and the cut
of ``classes`` in ``run_swarm_sharded``.  No GPU calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
from host_helpers import E_ARG
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"


def test_header_declares_and_library_exports_the_mixed_swarm_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_swarm_loop_mixed\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"const mpcqp_swarm\* s,\s+const int32_t\* cls, void\* stream\);", text, re.M)
    assert re.search(r"^int mpcqp_swarm_loop_mixed_warm\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"const mpcqp_swarm\* s,\s+const int32_t\* cls, int guess_passes, void\* stream\);", text, re.M)
    # the ninth launch kind (its line carries a comment: test_warm_pair_host.py counts the bare ones, eight)
    assert re.search(r"^#define MPCQP_LAUNCH_LOOP_MIXED_WARM 8\b", text, re.M)
    kinds = dict(re.findall(r"^#define MPCQP_LAUNCH_([A-Z_]+) (\d+)\b", text, re.M))
    assert sorted(map(int, kinds.values())) == list(range(9))
    for name, value in kinds.items():
        assert getattr(_lib, f"LAUNCH_{name}") == int(value) and int(value) in _lib.LAUNCH_KINDS, name
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    assert _lib.ABI_VERSION == 9
    assert _lib.LAUNCH_LOOP_MIXED_WARM == 8 and _lib.LAUNCH_KINDS[8] == "loop_mixed_warm"
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("mpcqp_swarm_loop_mixed", "mpcqp_swarm_loop_mixed_warm"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())
    # the contract a caller has to know is in the header
    doc = text[text.index("/* mpcqp_swarm_loop for a heterogeneous swarm"):text.index("int mpcqp_swarm_loop_mixed(")]
    for phrase in ("one dt", "Never paired", "MPCQP_BAD_CLASS", "MPCQP_E_HORIZON", "MPCQP_E_STATE", "MPCQP_E_ARG",
                   "bit for bit", "not handed to the replanner", "no stepped fallback", "MPCQP_LAUNCH_LOOP_MIXED"):
        assert phrase in doc, phrase
    warm = text[text.index("/* mpcqp_swarm_loop_mixed with every fused-loop launch warm"):
                text.index("int mpcqp_swarm_loop_mixed_warm(")]
    for phrase in ("guess_passes <= 0", "bit for bit", "MPCQP_E_HORIZON", "MPCQP_E_STATE", "never paired",
                   "MPCQP_LAUNCH_LOOP_MIXED_WARM", "warm mixed fleet loop"):
        assert phrase in warm, phrase
    # the sentences about the calls that stay as they were stand word for word, with a pointer beside them
    assert "the swarm is unchanged" in text and "keep using the workspace's own block" in text
    classes_doc = text[text.index(" * Per-QP parameter classes"):text.index("#define MPCQP_BAD_CLASS")]
    assert "mpcqp_swarm_loop_mixed" in classes_doc


def _swarm_struct(_lib):
    s = _lib.MpcqpSwarm()
    s.rrt.max_iterations, s.rrt.width, s.rrt.height = 10, 8, 8
    s.path_cap, s.horizon, s.dt, s.desired_speed = 16, 15, 0.1, 15.0
    return s


def test_mixed_swarm_calls_check_their_arguments_before_the_device():
    """Null workspaces, a null fleet, a null swarm and a null cls: E_ARG, nothing touched."""
    _lib = _binding()
    L = _lib.lib()
    st = (ctypes.c_int32 * 2)(77, 77)
    cls = (ctypes.c_int32 * 4)()
    c = ctypes.addressof(cls)
    f = _lib.MpcqpFleet()
    f.status = ctypes.addressof(st)
    s = _swarm_struct(_lib)
    for call in (lambda *a: L.mpcqp_swarm_loop_mixed(*a, None),
                 lambda *a: L.mpcqp_swarm_loop_mixed_warm(*a, 8, None)):
        assert call(None, None, ctypes.byref(f), ctypes.byref(s), None) == E_ARG
        assert b"null cls" in L.mpcqp_last_error()
        assert call(None, None, ctypes.byref(f), None, c) == E_ARG
        assert b"null swarm" in L.mpcqp_last_error()
        assert call(None, None, None, ctypes.byref(s), c) == E_ARG
        assert call(None, None, ctypes.byref(f), ctypes.byref(s), c) == E_ARG  # null workspaces
        assert b"null" in L.mpcqp_last_error()
        bad = _swarm_struct(_lib)  # the swarm struct's checks are mpcqp_swarm_loop's
        bad.max_replans = -1
        assert call(None, None, ctypes.byref(f), ctypes.byref(bad), c) == E_ARG
        assert b"max_replans" in L.mpcqp_last_error()
    assert list(st) == [77, 77]


def test_mixed_swarm_kernel_resources():
    """k_swarm_loop_mixed<N> and k_swarm_loop_mixed_warm<N>, N = 1..32: two waves per SIMD, no AGPRs, no more
    LDS than the mixed fleet loop (cold) or the warm fleet loop (warm) of the same horizon, and that loop's
    scratch plus at most 64 bytes (the margin test_swarm_warm_host.py grants the live trigger)."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    for prefix, base in (("swarm_mixed:", "loop_mixed:"), ("swarm_mixed_warm:", "loop_warm:")):
        own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith(prefix)}
        assert sorted(own) == list(range(1, 33)), prefix
        for n, r in own.items():
            b = res[f"{base}{n}"]
            print(f"{prefix}{n}", r, "base", b)
            assert r["Occupancy"] >= 2, (prefix, n, r)
            assert r["AGPRs"] == 0, (prefix, n, r)
            assert r["LDS"] <= b["LDS"], (prefix, n, r, b)
            assert r["ScratchSize"] <= b["ScratchSize"] + 64, (prefix, n, r, b)
    # the new keys are not selected by the prefixes the tests before them use
    for k in res:
        if k.startswith("swarm_mixed"):
            assert not k.startswith(("pair:", "loop_pair:", "warm:", "loop_warm:", "loop:", "loop_warm_carry",
                                     "pair_warm:", "serve_warm:", "mixed:", "loop_mixed:", "swarm_warm")), k


class _Ctrl:
    """Stands in for a BatchedMPCController: records its set_classes calls."""

    def __init__(self):
        self.calls = []

    def set_classes(self, params_list, settings=None):
        self.calls.append((params_list, settings))


def _bare_swarm(N=15, fused=True, warm_start=False, dt=0.1):
    """A Swarm without planner or workspaces (no device here): what the argument checks read."""
    import torch
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker
    from mpcqp.pipeline.swarm import Swarm

    t = object.__new__(FleetTracker)
    t._torch = torch
    t.device = torch.device("cpu")
    t.mpc = MPCConfig(horizon=N, sim_steps=5, dt=dt)
    t.params = t.mpc.to_parameters(0.8)
    t._ref_dt = float(t.mpc.dt)
    t.horizon, t.max_vehicles, t.max_ref_len = N, 8, 64
    t.fused = False  # the swarm's tracker is built so
    t.num_classes, t._class_params = 0, None
    t._bufs = t._fleet = None
    t._nominal, t._relaxed = _Ctrl(), _Ctrl()
    sw = object.__new__(Swarm)
    sw.fleet, sw.mpc, sw.fused, sw.warm_start = t, t.mpc, fused, warm_start
    return sw


def test_swarm_set_classes_argument_checks():
    from mpcqp.pipeline.fleet import relaxed_parameters

    sw = _bare_swarm()
    base = sw.fleet.params
    with pytest.raises(ValueError, match="fused=True"):
        _bare_swarm(fused=False).set_classes([base])
    with pytest.raises(ValueError, match="horizon <= 32"):
        s40 = _bare_swarm(N=40)
        s40.set_classes([s40.fleet.params])
    import dataclasses

    with pytest.raises(ValueError, match="one dt"):
        sw.set_classes([base, dataclasses.replace(base, dt=0.05)])
    assert sw.fleet.num_classes == 0 and not sw.fleet._nominal.calls  # a refusal sets nothing
    # the two controllers are driven as FleetTracker.set_classes drives them, and the fleet knows its classes
    wide = dataclasses.replace(base, wheelbase_px=14.0)
    for warm in (False, True):  # combines with warm_start
        sw = _bare_swarm(warm_start=warm)
        sw.set_classes([base, wide], settings=[{}, dict(max_iter=7)])
        (nom, ns), = sw.fleet._nominal.calls
        (rel, rs), = sw.fleet._relaxed.calls
        assert nom == [base, wide] and ns == [{}, dict(max_iter=7)] and rs == ns
        for got, p in zip(rel, (base, wide)):
            want = relaxed_parameters(p)
            assert got.du_bounds == want.du_bounds and got.wheelbase_px == want.wheelbase_px
        assert sw.fleet.num_classes == 2 and sw.fleet._class_params == [base, wide]
        assert sw.fleet._class_indices(None, 3).tolist() == [0, 0, 0]
        assert sw.fleet._class_indices(np.array([1, 0, -1, 2]), 4).tolist() == [1, 0, -1, 2]
        # None / [] drops the tables
        sw.set_classes([] if warm else None)
        assert sw.fleet.num_classes == 0 and sw.fleet._class_params is None
        assert sw.fleet._nominal.calls[-1] == (None, None) and sw.fleet._relaxed.calls[-1] == (None, None)
    sw = _bare_swarm()
    sw.set_classes([base], relaxed_settings=dict(max_iter=9))
    assert sw.fleet._relaxed.calls[-1][1] == dict(max_iter=9) and sw.fleet._nominal.calls[-1][1] is None


def test_swarm_run_classes_without_a_table_is_refused():
    """classes= without set_classes: FleetTracker._class_indices' refusal, before the fleet is loaded."""
    sw = _bare_swarm()
    V = 3
    starts = np.array([[10.0 + v, 10.0] for v in range(V)])
    goals = starts + 50.0
    sw._plan = lambda s, g, seeds: (np.ones(V, bool), [[tuple(a), tuple(b)] for a, b in zip(s, g)], [None] * V)
    with pytest.raises(ValueError, match="set_classes"):
        sw.run(starts, goals, classes=np.zeros(V, np.int32))
    assert sw.fleet._bufs is None
    sw.set_classes([sw.fleet.params])
    with pytest.raises(ValueError, match="shape"):
        sw.run(starts, goals, classes=np.zeros(V + 1, np.int32))
    with pytest.raises(ValueError, match="integer"):
        sw.run(starts, goals, classes=np.zeros(V))


def test_run_swarm_sharded_cuts_classes_like_the_seeds():
    from mpcqp.pipeline.swarm import SwarmResult, run_swarm_sharded, shard_vehicles

    V, world = 10, 3
    starts = np.arange(2 * V, dtype=float).reshape(V, 2)
    goals = starts + 100.0
    cls = np.arange(V) % 4
    seen = []

    def run(s, g, seeds=None, **kw):
        seen.append(dict(seeds=np.asarray(seeds), kw=kw, n=len(s)))
        n = len(s)
        return SwarmResult(states=[np.zeros((1, 4))] * n, phase=np.zeros(n, int), steps=np.ones(n, int),
                           replans=np.zeros(n, int), planned=np.ones(n, bool))

    gather = lambda out, obj: out.__setitem__(0, obj)
    for r in range(world):
        lo, hi = shard_vehicles(V, world, r)
        run_swarm_sharded(run, starts, goals, np.arange(V) + 5, rank=r, world=world, all_gather_object=gather,
                          classes=cls, sim_steps=7)
        call = seen[-1]
        np.testing.assert_array_equal(call["seeds"], np.arange(lo, hi) + 5)
        assert set(call["kw"]) == {"classes", "sim_steps"} and call["kw"]["sim_steps"] == 7
        np.testing.assert_array_equal(call["kw"]["classes"], cls[lo:hi])
        assert call["n"] == hi - lo
    # without classes nothing new reaches run
    run_swarm_sharded(run, starts, goals, None, rank=0, world=world, all_gather_object=gather)
    assert seen[-1]["kw"] == {}
    run_swarm_sharded(run, starts, goals, None, rank=0, world=world, all_gather_object=gather, classes=None)
    assert seen[-1]["kw"] == {}
