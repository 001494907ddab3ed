"""What the host (CPU) test files share: the binding of the built library, a controller object without a
workspace, and the return codes of ``include/mpcqp.h``.  A plain module, imported like ``param_variants``."""
from __future__ import annotations

import ctypes

OK, E_ARG, E_HORIZON, E_BATCH, E_HIP, E_STATE, E_DEVICE = 0, -1, -2, -3, -4, -5, -6  # MPCQP_OK, MPCQP_E_*


def binding():
    """``mpcqp._lib`` over the tree's library (built first where it is missing)."""
    import __graft_entry__ as g

    if not g.LIB.exists():
        g.build_library()
    from mpcqp import _lib

    return _lib


def bare_controller(N=10, max_batch=8, num_classes=0):
    """A controller object without a workspace (no device here): what the argument checks read."""
    import torch
    from mpcqp.control.mpc_controller import BatchedMPCController

    c = object.__new__(BatchedMPCController)
    c._torch = torch
    c.device = torch.device("cpu")
    c.horizon, c.max_batch, c.num_classes = N, max_batch, num_classes
    c._ws = ctypes.c_void_p()  # null: close() / __del__ have nothing to destroy
    return c
