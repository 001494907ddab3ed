"""CPU tests of the per-QP parameter classes (``mpcqp_set_classes`` / ``mpcqp_build_mixed``): the two
entry points in the header and the library, the host helper ``_lib.class_table`` against
``to_c_params`` field by field, and the argument checks that come before any device call.  No GPU
calls are made here."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
from host_helpers import E_ARG
from host_helpers import bare_controller as _bare_controller
from host_helpers import binding as _binding
from param_variants import VARIANTS, resolution, variant

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mpcqp.h"


def _variants(N):
    from mpcqp.config import MPCConfig

    return [variant(MPCConfig(horizon=N).to_parameters(resolution(name)), name) for name in VARIANTS]


def _fields(c):
    out = {}
    for name, _ in type(c)._fields_:
        v = getattr(c, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    return out


def test_header_declares_and_library_exports_the_class_calls():
    _lib = _binding()
    text = HEADER.read_text()
    assert re.search(r"^int mpcqp_set_classes\(mpcqp_ws\* ws, int K, const mpcqp_params\* blocks\);", text, re.M)
    assert re.search(r"^int mpcqp_build_mixed\(mpcqp_ws\* ws, int B, const double\* x0, const double\* ref, "
                     r"const double\* u_prev,\s+const int32_t\* cls, void\* stream\);", text, re.M)
    assert re.search(r"^#define MPCQP_BAD_CLASS \(-11\)", text, re.M)
    assert re.search(r"^#define MPCQP_ABI_VERSION 9$", text, re.M)  # additive: the ABI version stays
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("mpcqp_set_classes", "mpcqp_build_mixed"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.exported_symbols()
    assert _lib.BAD_CLASS == -11 and _lib.ABI_VERSION == 9
    assert _lib.STATUS_NAMES[_lib.BAD_CLASS] == "bad_class"
    # the limits a caller has to know are in the header
    assert "never runs two QPs per wave" in text and "keep using the workspace's own block" in text


def test_class_calls_check_their_arguments_before_the_device():
    """A null workspace or null pointers are refused before anything touches a device."""
    _lib = _binding()
    L = _lib.lib()
    assert L.mpcqp_set_classes(None, 0, None) == E_ARG
    assert b"null ws" in L.mpcqp_last_error()
    assert L.mpcqp_build_mixed(None, 1, None, None, None, None, None) == E_ARG


@pytest.mark.parametrize("N", [10, 20])
def test_class_table_fills_each_block_as_to_c_params(N):
    from mpcqp._lib import MpcqpParams, class_table, to_c_params

    plist = _variants(N)
    table = class_table(plist)
    assert len(table) == len(VARIANTS) and isinstance(table[0], MpcqpParams)
    assert ctypes.sizeof(table) == len(VARIANTS) * ctypes.sizeof(MpcqpParams)  # contiguous blocks, as the C array
    for k, p in enumerate(plist):
        assert _fields(table[k]) == _fields(to_c_params(p)), VARIANTS[k]
    # the classes really differ (dt, wheelbase, weights, bounds, slack weights)
    assert {table[k].dt for k in range(len(plist))} == {0.1, 0.05, 0.2}
    assert len({table[k].wheelbase_px for k in range(len(plist))}) == 2
    # one settings dict and one method for all classes
    table = class_table(plist, method="newton", settings=dict(max_iter=7, polish_from=0))
    for k, p in enumerate(plist):
        assert _fields(table[k]) == _fields(to_c_params(p, 1, max_iter=7, polish_from=0)), VARIANTS[k]
    # a list with one settings dict (and one method) per class
    per = [dict(max_iter=100 + k, rho=0.1 * (k + 1)) for k in range(len(plist))]
    methods = ["admm" if k % 2 == 0 else "newton" for k in range(len(plist))]
    table = class_table(plist, method=methods, settings=per)
    for k, p in enumerate(plist):
        assert _fields(table[k]) == _fields(to_c_params(p, k % 2, **per[k])), VARIANTS[k]
        assert table[k].max_iter == 100 + k and table[k].method == k % 2


def test_class_table_refuses_what_the_library_would():
    from mpcqp._lib import class_table
    from mpcqp.config import MPCConfig

    plist = _variants(10)
    with pytest.raises(ValueError, match="horizon"):
        class_table(plist + [MPCConfig(horizon=12).to_parameters(0.8)])
    with pytest.raises(ValueError, match="debug_state"):
        class_table(plist, settings=dict(debug_state=1))
    with pytest.raises(ValueError, match="debug_state"):
        class_table(plist[:2], settings=[{}, dict(debug_state=1)])
    with pytest.raises(ValueError, match="settings has 3 entries for 9 classes"):
        class_table(plist, settings=[{}, {}, {}])
    with pytest.raises(ValueError, match="method has 2 entries"):
        class_table(plist, method=["admm", "newton"])
    with pytest.raises(ValueError, match="method must be"):
        class_table(plist, method="simplex")
    with pytest.raises(ValueError, match="reproducible"):
        class_table(plist[:2], settings=[{}, dict(reproducible=1)])
    with pytest.raises(ValueError, match="at least one"):
        class_table([])


def test_solve_batch_classes_argument_checks():
    N, B = 10, 6
    x0, ref = np.zeros((B, 4)), np.zeros((B, N + 1, 4))
    # classes without a table: refused before any library call (the bare controller has no library)
    with pytest.raises(ValueError, match="set_classes"):
        _bare_controller(N).solve_batch(x0, ref, classes=np.zeros(B, np.int32))
    c = _bare_controller(N, num_classes=3)
    with pytest.raises(ValueError, match="shape"):
        c.solve_batch(x0, ref, classes=np.zeros(B + 1, np.int32))
    with pytest.raises(ValueError, match="shape"):
        c.solve_batch(x0, ref, classes=np.zeros((B, 1), np.int32))
    with pytest.raises(ValueError, match="integer"):
        c.solve_batch(x0, ref, classes=np.zeros(B))
    with pytest.raises(ValueError, match="max_batch"):
        c.solve_batch(np.zeros((9, 4)), np.zeros((9, N + 1, 4)), classes=np.zeros(9, np.int32))
    # the class indices reach the device as int32, whatever integer type they came in
    import torch

    for given in (np.array([0, 2, 1, -1, 3, 2**31 - 1], np.int64), [0, 2, 1, -1, 3, 2**31 - 1],
                  torch.tensor([0, 2, 1, -1, 3, 2**31 - 1], dtype=torch.int64)):
        t = c._class_input(given, B)
        assert t.dtype == torch.int32 and t.is_contiguous()
        assert t.tolist() == [0, 2, 1, -1, 3, 2**31 - 1]
    assert c._class_input(np.array([2**40, 1], np.int64), 2).tolist() == [-1, 1]  # no index: stays out of range
