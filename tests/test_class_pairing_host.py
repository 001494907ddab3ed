"""CPU tests of mixed launches at two per wave (``mpcqp_class_slots``, ``mpcqp_class_slot_waves``,
``mpcqp_set_class_pairing``; ``k_solve_pair_mixed``, ``k_fleet_loop_pair_mixed``): the entry points in the
header and the library, the argument checks that come before any device call, the grid formula, the recorded
resources of the new kernels, and the Python switches' own checks.  No GPU calls are made here."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path

import pytest
from host_helpers import E_ARG
from host_helpers import binding as _binding

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"
RESOURCES = ROOT / "build" / "kernel_resources.json"


def test_header_declares_and_library_exports_the_three_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_class_slots\(int V, int K, const int32_t\* cls, const int32_t\* seq, int32_t\* slots, "
                     r"void\* stream\);", text, re.M)
    assert re.search(r"^int mpcqp_class_slot_waves\(int V, int K\);", text, re.M)
    assert re.search(r"^int mpcqp_set_class_pairing\(mpcqp_ws\* ws, int on\);", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    assert _lib.ABI_VERSION == 9
    cap = re.search(r"^#define MPCQP_CLASS_SLOT_MAX_CLASSES (\d+)$", text, re.M)
    assert cap and int(cap.group(1)) == _lib.CLASS_SLOT_MAX_CLASSES
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("mpcqp_class_slots", "mpcqp_class_slot_waves", "mpcqp_set_class_pairing"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(mpcqp_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(_lib.exported_symbols())
    # no new launch kind: a class-paired launch records as the mixed launch it is
    kinds = dict(re.findall(r"^#define MPCQP_LAUNCH_([A-Z_]+) (\d+)\b", text, re.M))
    assert sorted(map(int, kinds.values())) == list(range(9))
    # the contract a caller has to know is in the header
    doc = text[text.index(" * Mixed launches at two per wave"):text.index("int mpcqp_set_class_pairing(")]
    doc = " ".join(doc.replace("\n *", " ").split())  # the comment's own line breaks and leaders aside
    for phrase in ("bit for bit", "exactly once", "-1 marks an empty half", "same class", "class by class",
                   "chunks of 1024", "stream capture", "MPCQP_E_ARG", "MPCQP_E_STATE", "(V + min(K + 1, V)) / 2",
                   "N <= 15", "mpcqp_set_pairing", "swarm", "warm call", "mpcqp_destroy"):
        assert phrase in doc, phrase
    # "never paired" now speaks of mpcqp_set_pairing alone and names the new switch beside it (the words
    # themselves stay: test_classes_host.py and test_fleet_classes_host.py look for them); the swarm's stands
    classes_doc = " ".join(text[text.index(" * Per-QP parameter classes"):text.index("#define MPCQP_BAD_CLASS")]
                           .replace("\n *", " ").split())
    assert "under mpcqp_set_pairing a mixed build never runs two QPs per wave" in classes_doc
    assert classes_doc.count("unless mpcqp_set_class_pairing") == 2
    loop_doc = " ".join(text[text.index("/* mpcqp_fleet_loop for a heterogeneous fleet"):
                             text.index("int mpcqp_fleet_loop_mixed(")].replace("\n *", " ").split())
    assert "Never paired by mpcqp_set_pairing" in loop_doc and "unless mpcqp_set_class_pairing" in loop_doc
    swarm_doc = text[text.index("/* mpcqp_swarm_loop for a heterogeneous swarm"):text.index("int mpcqp_swarm_loop_mixed(")]
    assert "Never paired" in swarm_doc


def test_calls_check_their_arguments_before_the_device():
    _lib = _binding()
    L = _lib.lib()
    assert L.mpcqp_set_class_pairing(None, 1) == E_ARG
    assert b"null ws" in L.mpcqp_last_error()
    assert L.mpcqp_set_class_pairing(None, 2) == E_ARG
    cls = (ctypes.c_int32 * 4)(0, 1, 0, 1)
    slots = (ctypes.c_int32 * 8)(*([77] * 8))
    a = ctypes.addressof
    assert L.mpcqp_class_slots(4, 2, None, None, a(slots), None) == E_ARG
    assert L.mpcqp_class_slots(4, 2, a(cls), None, None, None) == E_ARG
    assert L.mpcqp_class_slots(-1, 2, a(cls), None, a(slots), None) == E_ARG
    assert L.mpcqp_class_slots(4, 0, a(cls), None, a(slots), None) == E_ARG
    assert L.mpcqp_class_slots(4, _lib.CLASS_SLOT_MAX_CLASSES + 1, a(cls), None, a(slots), None) == E_ARG
    assert str(_lib.CLASS_SLOT_MAX_CLASSES).encode() in L.mpcqp_last_error()
    assert L.mpcqp_class_slots(0, 2, a(cls), None, a(slots), None) == 0  # nothing to pair, nothing launched
    assert list(slots) == [77] * 8


@pytest.mark.parametrize("K", [1, 3, 2000])
@pytest.mark.parametrize("V", [0, 1, 2, 3, 7, 1025])
def test_slot_waves_is_the_formula(V, K):
    """(V + min(K + 1, V)) / 2: at least the used waves whatever the classes' parities, never more than V."""
    L = _binding().lib()
    got = L.mpcqp_class_slot_waves(V, K)
    assert got == (V + min(K + 1, V)) // 2
    most_odd = min(K + 1, V)  # the most buckets that can be odd ...
    if (V - most_odd) % 2:    # ... with the parity of V
        most_odd -= 1
    assert (V + most_odd) // 2 <= got <= V


def test_class_pairing_kernel_resources():
    """k_solve_pair_mixed<N> and k_fleet_loop_pair_mixed<N>, N = 1..15, against records of the same build: two
    waves per SIMD, no AGPRs, no more LDS than the existing paired counterpart (k_solve_pair<N>,
    k_fleet_loop<N, true>).  Scratch: k_solve_pair_mixed<N> stays within the unpaired mixed counterpart's
    (k_solve_mixed<N>) plus the 64 bytes test_swarm_classes_host.py allows.  The paired loop does not hold to
    that line against k_fleet_loop_mixed<N> (N = 10: 96 bytes against 12): its spills are the pair layout's,
    which sits at 256 VGPRs -- k_fleet_loop<N, true> itself has 84 there -- so it is held to the paired plain
    loop's scratch plus those 64 bytes (DESIGN.md has the table)."""
    if not RESOURCES.exists():
        pytest.skip("no build record (build/kernel_resources.json)")
    res = json.loads(RESOURCES.read_text())
    for prefix, paired, scratch_base in (("pair_mixed:", "pair:", "mixed:"),
                                         ("loop_pair_mixed:", "loop_pair:", "loop_pair:")):
        own = {int(k.split(":")[1]): v for k, v in res.items() if k.startswith(prefix)}
        assert sorted(own) == list(range(1, 16)), prefix
        for n, r in own.items():
            p, u = res[f"{paired}{n}"], res[f"{scratch_base}{n}"]
            print(f"{prefix}{n}", r, "paired LDS", p["LDS"], f"{scratch_base}{n} scratch", u["ScratchSize"])
            assert r["Occupancy"] >= 2, (prefix, n, r)
            assert r["AGPRs"] == 0, (prefix, n, r)
            assert r["LDS"] <= p["LDS"], (prefix, n, r, p)
            assert r["ScratchSize"] <= u["ScratchSize"] + 64, (prefix, n, r, u)
    # the new keys are not selected by the prefixes the tests before them use
    for k in res:
        if k.startswith(("pair_mixed:", "loop_pair_mixed:")):
            assert not k.startswith(("pair:", "loop_pair:", "mixed:", "loop_mixed:", "pair_warm:", "loop:", "warm:",
                                     "loop_warm", "swarm_")), k


def test_python_switches_check_their_mode():
    """set_class_pairing refuses anything but "on" / "off" before it reaches the library, on a bare object."""
    from mpcqp.control.mpc_controller import BatchedMPCController

    _lib = _binding()
    assert _lib.CLASS_PAIRING_MODES == {"off": 0, "on": 1}
    c = object.__new__(BatchedMPCController)
    for bad in ("auto", "ON", 1, None):
        with pytest.raises(ValueError, match="class_pairing"):
            c.set_class_pairing(bad)
