"""CPU tests of the swarm on a changing map (``mpcqp_swarm_loop_map``, ``mpcqp_swarm_run_map``,
``k_swarm_loop_map<N>``, ``Swarm(grids=...)``): the entry points in the header and the library, the contract's
phrases, the struct's layout, the argument checks that come before any device call, ``Swarm``'s own checks,
the host arithmetic of ``SwarmResult.hits`` / ``replan_grid`` and the recorded resources of the new kernel.
No GPU calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
from host_helpers import E_ARG
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"


def test_header_declares_and_library_exports_the_map_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_swarm_run_map\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"const mpcqp_swarm\* s,\s+const mpcqp_swarm_map\* m, int steps, int use_graph, void\* stream\);",
                     text, re.M)
    assert re.search(r"^int mpcqp_swarm_loop_map\(mpcqp_ws\* nominal, mpcqp_ws\* relaxed, const mpcqp_fleet\* f, "
                     r"const mpcqp_swarm\* s,\s+const mpcqp_swarm_map\* m, void\* stream\);", text, re.M)
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())  # the header declares exactly what the binding binds
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("mpcqp_swarm_run_map", "mpcqp_swarm_loop_map"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M) and _lib.ABI_VERSION == 9  # additive
    # the tenth launch kind, and the causes
    assert re.search(r"^#define MPCQP_LAUNCH_LOOP_MAP \(MPCQP_LAUNCH_LOOP_MIXED_WARM \+ 1\)$", text, re.M)
    assert _lib.LAUNCH_LOOP_MAP == _lib.LAUNCH_LOOP_MIXED_WARM + 1 == 9 and _lib.LAUNCH_KINDS[9] == "loop_map"
    for name, value in (("ABORTED", 1), ("OFF_TRACK", 2), ("BLOCKED", 3)):
        assert re.search(rf"^#define MPCQP_REPLAN_{name} {value}$", text, re.M)
        assert getattr(_lib, f"REPLAN_{name}") == value
    assert re.search(r"^#define MPCQP_SWARM_MAP_MAX_LOOKAHEAD 64$", text, re.M) and _lib.SWARM_MAP_MAX_LOOKAHEAD == 64
    doc = text[text.index(" * The swarm on a changing map"):text.index("int mpcqp_swarm_run_map(")]
    for phrase in ("grid min(k / epoch_steps, T - 1)", "bit for bit", "lookahead", "MPCQP_E_ARG", "one vehicle per wave",
                   "not read", "MPCQP_LAUNCH_LOOP_MAP", "cold only", "no classes", "round half to even",
                   "replan_distance <= 0 switches off only the off-track test"):
        assert phrase in doc, phrase
    kinds_doc = text[text.index("/* What the last solver launch"):text.index("int mpcqp_launch_info(")]
    assert "mpcqp_swarm_loop_map" in kinds_doc


def test_map_struct_layout_matches_c(tmp_path):
    """ctypes' MpcqpSwarmMap == the C compiler's mpcqp_swarm_map (sizeof, offsets)."""
    _lib = _binding()
    fields = [f for f, _ in _lib.MpcqpSwarmMap._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcqp.h"\nint main(void){\n'
                   '  printf("%zu\\n", sizeof(mpcqp_swarm_map));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(mpcqp_swarm_map, {f}));\n' for f in fields)
                   + '  printf("%d\\n", MPCQP_LAUNCH_LOOP_MAP);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.MpcqpSwarmMap)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.MpcqpSwarmMap, f).offset == off, f
    assert vals[-1] == 9


def _swarm_struct(_lib):
    s = _lib.MpcqpSwarm()
    s.rrt.max_iterations, s.rrt.width, s.rrt.height = 10, 8, 8
    s.path_cap, s.horizon, s.dt, s.desired_speed = 16, 15, 0.1, 15.0
    return s


def test_map_calls_check_their_arguments_before_the_device():
    """Every MPCQP_E_ARG case of the map struct, on both calls, with null workspaces behind them: the map's checks
    come before the fleet's, and nothing is touched."""
    _lib = _binding()
    L = _lib.lib()
    st = (ctypes.c_int32 * 2)(77, 77)
    grid = (ctypes.c_uint8 * 64)(*([1] * 64))
    grid_of = (ctypes.c_int32 * 2)(77, 77)
    f = _lib.MpcqpFleet()
    f.status = ctypes.addressof(st)
    s = _swarm_struct(_lib)  # max_replans 0: no swarm buffer is needed, and occupancy stays NULL

    def a_map(**fields):
        m = _lib.MpcqpSwarmMap()
        m.grids, m.num_grids, m.epoch_steps, m.lookahead = ctypes.addressof(grid), 1, 10, 20
        m.grid_of = ctypes.addressof(grid_of)
        for k, v in fields.items():
            setattr(m, k, v)
        return m

    calls = (lambda s_, m: L.mpcqp_swarm_loop_map(None, None, ctypes.byref(f), s_, m, None),
             lambda s_, m: L.mpcqp_swarm_run_map(None, None, ctypes.byref(f), s_, m, 5, 0, None),
             lambda s_, m: L.mpcqp_swarm_run_map(None, None, ctypes.byref(f), s_, m, 5, 1, None))
    for call in calls:
        assert call(None, ctypes.byref(a_map())) == E_ARG and b"null swarm" in L.mpcqp_last_error()
        assert call(ctypes.byref(s), None) == E_ARG and b"null swarm map" in L.mpcqp_last_error()
        for fields, msg in ((dict(num_grids=0), b"num_grids"), (dict(epoch_steps=0), b"epoch_steps"),
                            (dict(lookahead=-1), b"lookahead"), (dict(lookahead=65), b"lookahead"),
                            (dict(grids=None), b"null grids")):
            assert call(ctypes.byref(s), ctypes.byref(a_map(**fields))) == E_ARG, fields
            assert msg in L.mpcqp_last_error(), (fields, L.mpcqp_last_error())
        # lookahead 0 and 64 are inside; the next refusal is the fleet's (null workspaces)
        for look in (0, 64):
            assert call(ctypes.byref(s), ctypes.byref(a_map(lookahead=look))) == E_ARG
            assert b"null argument" in L.mpcqp_last_error(), L.mpcqp_last_error()
        # grid_of may be NULL only without replans; with them the swarm's own buffers are checked first
        assert call(ctypes.byref(s), ctypes.byref(a_map(grid_of=None))) == E_ARG
        assert b"null argument" in L.mpcqp_last_error()
        bad = _swarm_struct(_lib)
        bad.max_replans = 1
        assert call(ctypes.byref(bad), ctypes.byref(a_map())) == E_ARG and b"null swarm buffer" in L.mpcqp_last_error()
        buf = (ctypes.c_double * 8)()
        for name, _ in _lib.MpcqpSwarm._fields_[13:]:  # every pointer of the swarm struct but occupancy
            setattr(bad, name, ctypes.addressof(buf))
        assert bad.occupancy is None
        assert call(ctypes.byref(bad), ctypes.byref(a_map(grid_of=None))) == E_ARG
        assert b"null grid_of" in L.mpcqp_last_error(), L.mpcqp_last_error()
        assert call(ctypes.byref(bad), ctypes.byref(a_map())) == E_ARG and b"null argument" in L.mpcqp_last_error()
    assert list(st) == [77, 77] and list(grid_of) == [77, 77]


def test_swarm_grids_argument_checks():
    """Swarm._check_grids: what the constructor refuses before it builds a planner or a workspace."""
    from mpcqp.pipeline.swarm import Swarm

    occ = np.ones((6, 8), np.uint8)
    occ[2, 3] = 0
    closed = occ.copy()
    closed[4] = 0
    check = Swarm._check_grids
    assert check(occ, None, None, 20, False) == (None, 1, 0)
    g, e, look = check(occ, np.stack([occ, closed]), 10, 20, False)
    assert g.dtype == np.uint8 and g.shape == (2, 6, 8) and (e, look) == (10, 20)
    assert check(occ, occ[None], None, 0, False)[1:] == (1, 0)  # one grid needs no epoch
    with pytest.raises(ValueError, match=r"grids\[0\] must equal occupancy"):
        check(occ, np.stack([closed, occ]), 10, 20, False)
    with pytest.raises(ValueError, match="shape"):
        check(occ, occ, 10, 20, False)
    with pytest.raises(ValueError, match="shape"):
        check(occ, np.ones((2, 8, 6), np.uint8), 10, 20, False)
    with pytest.raises(ValueError, match="warm_start"):
        check(occ, occ[None], 10, 20, True)
    with pytest.raises(ValueError, match="need epoch_steps"):
        check(occ, np.stack([occ, closed]), None, 20, False)
    with pytest.raises(ValueError, match="epoch_steps must be >= 1"):
        check(occ, np.stack([occ, closed]), 0, 20, False)
    with pytest.raises(ValueError, match="epoch_steps needs grids"):
        check(occ, None, 10, 20, False)
    for look in (-1, 65):
        with pytest.raises(ValueError, match="lookahead"):
            check(occ, occ[None], 1, look, False)
    # a swarm with grids takes no classes
    sw = object.__new__(Swarm)
    sw.grids, sw.fused, sw.fleet = occ[None], True, None
    with pytest.raises(ValueError, match="grids"):
        sw.set_classes([object()])


def test_hits_and_replan_grid_on_a_hand_made_result():
    from mpcqp.pipeline.swarm import grid_index, map_hits, replan_grids

    assert grid_index(np.array([0, 9, 10, 19, 20, 500]), 10, 2).tolist() == [0, 0, 1, 1, 1, 1]
    assert int(grid_index(7, 8, 3)) == 0 and int(grid_index(16, 8, 3)) == 2 and int(grid_index(1000, 8, 3)) == 2
    g0 = np.ones((4, 6), np.uint8)
    g1 = g0.copy()
    g1[1, 2] = 0  # the cell x = 2, y = 1 closes at step 3 (epoch_steps 3)
    grids = np.stack([g0, g1])
    # vehicle 0 stands on (2, 1) for five steps: free at k = 1, 2 (grid 0), occupied at k = 3, 4, 5 (grid 1);
    # 2.5 rounds half to even to 2, 1.5 to 2 (free row), and positions off the grid are clipped onto it
    states = [np.array([[2.0, 1.0, 0, 0]] * 5),
              np.array([[2.5, 0.5, 0, 0], [2.5, 1.5, 0, 0], [2.5, 0.5, 0, 0], [1.5, 1.4, 0, 0], [2.4, 0.6, 0, 0]]),
              np.array([[-7.0, 1.0, 0, 0]] * 4 + [[2.0, 99.0, 0, 0]]),
              np.zeros((0, 4))]
    assert map_hits(states, grids, 3).tolist() == [3, 2, 0, 0]
    assert map_hits(states, grids[:1], 3).tolist() == [0, 0, 0, 0]
    # replan_steps: steps where the replan gave a plan, -steps - 1 where it failed, 0 unused
    replans = np.array([0, 1, 2, 1])
    rsteps = np.array([[0, 0], [10, 0], [-17, 40], [-1, 0]])
    assert replan_grids(replans, rsteps, 8, 3).tolist() == [[-1, -1], [1, -1], [2, 2], [0, -1]]
    assert replan_grids(replans, rsteps, 10, 2).tolist() == [[-1, -1], [1, -1], [1, 1], [0, -1]]


def test_map_swarm_results_merge():
    """merge_swarm_results carries the three new per-vehicle fields, and leaves them None where no shard has them."""
    from mpcqp.pipeline.swarm import SwarmResult, merge_swarm_results

    def part(n, on_map):
        extra = dict(replan_cause=np.full((n, 1), 3), replan_grid=np.full((n, 1), 1), hits=np.arange(n)) if on_map else {}
        return SwarmResult(states=[np.zeros((1, 4))] * n, phase=np.zeros(n, int), steps=np.ones(n, int),
                           replans=np.ones(n, int), planned=np.ones(n, bool), **extra)

    got = merge_swarm_results([part(2, True), part(3, True)])
    assert got.replan_cause.shape == (5, 1) and got.replan_grid.shape == (5, 1) and got.hits.tolist() == [0, 1, 0, 1, 2]
    plain = merge_swarm_results([part(2, False), part(3, False)])
    assert plain.replan_cause is None and plain.replan_grid is None and plain.hits is None


def test_map_swarm_kernel_resources():
    """k_swarm_loop_map<N>, N = 1..32: two waves per SIMD, no AGPRs, no more LDS than the fused loop of the same
    horizon, and that loop's scratch plus at most 64 bytes (the margin this project grants a live trigger)."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith("swarm_map:")}
    assert sorted(own) == list(range(1, 33))
    for n, r in own.items():
        b = res[f"loop:{n}"]
        print(f"swarm_map:{n}", r, "loop", b)
        assert r["Occupancy"] >= 2, (n, r)
        assert r["AGPRs"] == 0, (n, r)
        assert r["LDS"] <= b["LDS"], (n, r, b)
        assert r["ScratchSize"] <= b["ScratchSize"] + 64, (n, r, b)
    for k in res:  # the new keys are not selected by the prefixes the tests before them use
        if k.startswith("swarm_map"):
            assert not k.startswith(("pair:", "loop_pair:", "warm:", "loop_warm:", "loop:", "loop_warm_carry",
                                     "pair_warm:", "serve_warm:", "mixed:", "loop_mixed:", "swarm_warm", "swarm_mixed",
                                     "pair_mixed:", "loop_pair_mixed:")), k
