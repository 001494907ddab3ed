"""Linear time-varying MPC on MI355X: drop-in for ``src/control/mpc_controller.py``.

``MPCParameters`` and ``MPCController.solve`` keep the reference's names,
arguments, return values and failure behaviour (``mpc_controller.py:17-145``);
the QP that the reference assembles in cvxpy and hands to OSQP
(``:53-132``) is built and solved by the HIP kernels of ``libmpcqp.so``
(``csrc/mpcqp.hip``: K1 ``k_build`` = unwrap + linearize, K2 ``k_solve`` =
condense + OSQP-algorithm ADMM + polish).  ``BatchedMPCController`` is the
batched entry point that thousands of candidate trajectories go through at once.
"""
from __future__ import annotations

import ctypes
import logging
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import numpy as np

from .. import _lib

LOG = logging.getLogger(__name__)

FloatArray = np.ndarray


@dataclass
class MPCParameters:
    """Same fields and defaults as ``src/control/mpc_controller.py:17-30``."""

    wheelbase_px: float
    dt: float
    horizon: int
    q: FloatArray
    r: FloatArray
    q_terminal: FloatArray
    u_bounds: Tuple[Tuple[float, float], Tuple[float, float]]
    v_bounds: Tuple[float, float]
    du_bounds: Tuple[Tuple[float, float], Tuple[float, float]]
    slack_velocity: float = 1e3
    slack_input: float = 5e2
    slack_rate: float = 5e2


class BatchSolution(NamedTuple):
    """Device tensors of one ``solve_batch`` call (views into controller-owned buffers,
    valid until the next call on the same controller)."""

    u0: "object"  # (B, 2)      float64
    X: "object"  # (B, 4, N+1)  float64
    U: "object"  # (B, 2, N)    float64
    status: "object"  # (B,)    int32   (1 solved, 2 solved_inaccurate, -2 max_iter, -10 numerical)
    iters: "object"  # (B, 4)   int32   {ADMM its, polish its, KKT factorizations, line-search trials}
    active: "object"  # (B, 5N+1) uint8 {0 inactive, 1 lower, 2 upper} per soft row


def _arr_key(a) -> bytes:
    if type(a) is np.ndarray and a.dtype == np.float64 and a.flags.c_contiguous:
        return a.tobytes()
    return np.asarray(a, float).tobytes()


_NUM = (float, int, np.floating, np.integer)


def _tuple_key(a) -> tuple:
    """Value key of a bounds field: a flat tuple of floats whatever the container (a tuple of tuples
    of numbers takes the fast path; lists, arrays and tuples holding them are converted), so equal
    bounds share one workspace and an unhashable leaf never reaches the cache."""
    if type(a) is tuple:
        if all(type(r) is tuple and all(isinstance(v, _NUM) for v in r) for r in a):
            return tuple(float(v) for r in a for v in r)
        if all(isinstance(v, _NUM) for v in a):
            return tuple(float(v) for v in a)
    return tuple(np.asarray(a, float).ravel().tolist())


def _params_key(params, method: int, settings: dict) -> tuple:
    """Value key of a parameter block + solver settings (the B=1 controller cache; computed once per
    drop-in solve, so it avoids array conversions where the fields already are float64 arrays /
    tuples, as MPCConfig.to_parameters and dataclasses.replace produce them)."""
    return (
        params.horizon,
        params.wheelbase_px,
        params.dt,
        _arr_key(params.q),
        _arr_key(params.r),
        _arr_key(params.q_terminal),
        _tuple_key(params.u_bounds),
        _tuple_key(params.v_bounds),
        _tuple_key(params.du_bounds),
        getattr(params, "slack_velocity", 1e3),
        getattr(params, "slack_input", 5e2),
        getattr(params, "slack_rate", 5e2),
        int(method),
        tuple(sorted(settings.items())),
    )


def class_input(torch, device, classes, B):
    """Class indices (int array or integer tensor) as an int32 tensor of shape (B,) on ``device``; a
    tensor of that type and place is used as it is.  Shared by ``solve_batch(classes=...)`` and
    ``FleetTracker``."""
    if isinstance(classes, torch.Tensor):
        if classes.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"classes must be an integer tensor, got {classes.dtype}")
        t = classes
    else:
        a = np.asarray(classes)
        if a.dtype.kind not in "iu":
            raise ValueError(f"classes must be an integer array, got dtype {a.dtype}")
        # values outside int32 are no class indices: kept out of range (the device reports them per QP)
        a = np.where((a < 0) | (a > 2**31 - 1), -1, a).astype(np.int32)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if tuple(t.shape) != (B,):
        raise ValueError(f"classes must have shape ({B},), got {tuple(t.shape)}")
    if t.device != device or t.dtype != torch.int32:
        t = t.to(device=device, dtype=torch.int32)
    return t.contiguous()


class BatchedMPCController:
    """Solve B independent MPC QPs per call on one GPU.

    ``solve_batch(x0[B,4], ref[B,N+1,4], u_prev[B,2])`` runs K1 + K2 asynchronously on
    the current torch stream (or ``stream``).  Inputs may be numpy arrays (copied to the
    device) or float64 device tensors (used in place).

    ``pairing`` ("auto", "on", "off"): two QPs per wave for horizons N <= 15 (``mpcqp_set_pairing``;
    the same results bit for bit).  "auto" pairs a launch with more QPs than the GPU has wave slots;
    a warm launch (``solve_batch(..., U_guess=...)``, the warm fleet loops) pairs under "on" only.
    ``launch_info()`` tells what the last launch did.

    Mixed batches: ``set_classes([params_0, ..., params_{K-1}])`` gives the workspace a table of K
    parameter blocks of this horizon, and ``solve_batch(..., classes=cls)`` solves QP b under block
    ``cls[b]`` in the same single launch (``mpcqp_build_mixed``).  A mixed launch ignores ``pairing`` and
    runs one QP per wave unless ``class_pairing="on"`` (``mpcqp_set_class_pairing``): then two QPs of the
    same class share a wave for N <= 15, the same results bit for bit, and ``launch_info()`` reports
    ``per_wave == 2``.  ``solve_one``, the fleet and the swarm keep using the controller's own block.
    """

    def __init__(self, params, max_batch: int, *, device=None, method: str = "admm", pairing: str = "auto",
                 class_pairing: str = "off", **settings) -> None:
        import torch

        if method not in ("admm", "newton"):
            raise ValueError("method must be 'admm' or 'newton'")
        if not torch.cuda.is_available():
            raise _lib.LibraryError("BatchedMPCController needs a ROCm GPU; there is no CPU fallback")
        self._torch = torch
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.params = params
        self.method = _lib.METHOD_ADMM if method == "admm" else _lib.METHOD_NEWTON
        self.settings = dict(settings)
        self.horizon = int(params.horizon)
        self.max_batch = int(max_batch)
        L = _lib.lib()
        self._L = L
        self._cparams = _lib.to_c_params(params, self.method, **self.settings)
        ws = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.mpcqp_create(ctypes.byref(self._cparams), self.max_batch, self.device.index, ctypes.byref(ws)),
                       "mpcqp_create")
        self._ws = ws
        self.num_classes = 0
        self.set_pairing(pairing)
        self.class_pairing = "off"
        if class_pairing != "off":
            self.set_class_pairing(class_pairing)
        N, B = self.horizon, self.max_batch
        kw = dict(device=self.device)
        self._u0 = torch.empty((B, 2), dtype=torch.float64, **kw)
        self._X = torch.empty((B, 4, N + 1), dtype=torch.float64, **kw)
        self._U = torch.empty((B, 2, N), dtype=torch.float64, **kw)
        self._status = torch.empty((B,), dtype=torch.int32, **kw)
        self._iters = torch.empty((B, 4), dtype=torch.int32, **kw)
        self._active = torch.empty((B, 5 * N + 1), dtype=torch.uint8, **kw)

    # ------------------------------------------------------------------
    def set_params(self, params) -> None:
        """Swap the parameter block (same horizon); stream-ordered."""
        self._cparams = _lib.to_c_params(params, self.method, **self.settings)
        _lib.check(self._L.mpcqp_set_params(self._ws, ctypes.byref(self._cparams)), "mpcqp_set_params")
        self.params = params

    def set_pairing(self, mode: str) -> None:
        """Two QPs per wave for N <= 15: "auto" (default), "on" or "off" (mpcqp_set_pairing)."""
        if mode not in _lib.PAIRING_MODES:
            raise ValueError(f"pairing must be one of {sorted(_lib.PAIRING_MODES)}")
        _lib.check(self._L.mpcqp_set_pairing(self._ws, _lib.PAIRING_MODES[mode]), "mpcqp_set_pairing")
        self.pairing = mode

    def set_class_pairing(self, mode: str) -> None:
        """Mixed launches at two per wave: "on" pairs QPs (in ``FleetTracker``'s nominal controller: vehicles)
        of the same class for N <= 15, "off" (default) keeps a mixed launch at one per wave
        (``mpcqp_set_class_pairing``; synchronous the first time it is "on": it allocates the slot table)."""
        if mode not in _lib.CLASS_PAIRING_MODES:
            raise ValueError(f"class_pairing must be one of {sorted(_lib.CLASS_PAIRING_MODES)}")
        with self._torch.cuda.device(self.device):
            _lib.check(self._L.mpcqp_set_class_pairing(self._ws, _lib.CLASS_PAIRING_MODES[mode]),
                       "mpcqp_set_class_pairing")
        self.class_pairing = mode

    def launch_info(self) -> dict:
        """What the last solver launch recorded on this controller's workspace did (``mpcqp_launch_info``;
        no device call): ``{"kind": _lib.LAUNCH_*, "name", "per_wave": 1 or 2, "workgroups", "count": B or V}``.
        ``kind`` is ``_lib.LAUNCH_NONE`` before any launch and after ``set_params``."""
        return _lib.launch_info(self._ws)

    def set_classes(self, params_list, settings=None, *, method=None) -> None:
        """The parameter blocks ("classes") of mixed batches: ``params_list[k]`` is block k
        (``mpcqp_set_classes``; synchronous).  ``settings``: one dict of solver settings for all
        classes or a list with one dict per class, on top of the controller's own settings;
        ``method``: the controller's by default, or "admm" / "newton", or a list with one per class.
        ``None`` or an empty list drops the table.  Every block has the controller's horizon."""
        if not params_list:
            _lib.check(self._L.mpcqp_set_classes(self._ws, 0, None), "mpcqp_set_classes")
            self.num_classes = 0
            return
        params_list = list(params_list)
        K = len(params_list)
        if isinstance(settings, (list, tuple)):
            if len(settings) != K:
                raise ValueError(f"settings has {len(settings)} entries for {K} classes")
            merged = [{**self.settings, **(st or {})} for st in settings]
        else:
            merged = {**self.settings, **(settings or {})}
        table = _lib.class_table(params_list, self.method if method is None else method, merged)
        if table[0].horizon != self.horizon:
            raise ValueError(f"the classes have horizon {table[0].horizon}, the controller {self.horizon}")
        with self._torch.cuda.device(self.device):
            _lib.check(self._L.mpcqp_set_classes(self._ws, K, table), "mpcqp_set_classes")
        self.num_classes = K

    def _class_input(self, classes, B):
        """``classes`` as an int32 device tensor of shape (B,) (a device tensor of that type is used in place)."""
        return class_input(self._torch, self.device, classes, B)

    def _device_input(self, a, shape, name):
        torch = self._torch
        if isinstance(a, torch.Tensor):
            t = a
            if t.device != self.device or t.dtype != torch.float64:
                t = t.to(device=self.device, dtype=torch.float64)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device, non_blocking=False)
        t = t.contiguous()
        if tuple(t.shape) != tuple(shape):
            t = t.reshape(shape)
        return t

    def solve_batch(self, x0, ref, u_prev=None, *, stream=None, classes=None, U_guess=None,
                    guess_passes=None) -> BatchSolution:
        """``classes`` (int array or int32 device tensor of shape (B,)): QP b is solved under block
        ``classes[b]`` of ``set_classes``; a QP whose index lies outside the table reports status
        ``_lib.BAD_CLASS`` and none of its other outputs is written.  ``None``: the controller's block.

        ``U_guess`` (tensor or array of shape (B, 2, N), the layout of ``U``): warm start
        (``mpcqp_solve_warm``) -- each QP first gets one polish attempt of at most ``guess_passes``
        passes (default ``_lib.DEFAULT_GUESS_PASSES``) from its guess; a hit returns the exact optimum
        with ``iters[:, 0] == 0``, a miss or an unusable guess (a non-finite entry, ``guess_passes <= 0``)
        runs the cold solve unchanged.  The previous ``U`` shifted one step is the usual guess; the
        returned ``U`` tensor itself may be passed.  Not with ``classes``; horizons <= 32 in fast mode.
        Under ``pairing="on"`` (N <= 15) the guess pairs too: two QPs per wave, each half with its own
        attempt, the results those of ``pairing="off"`` bit for bit; ``"auto"`` keeps a warm launch at
        one QP per wave."""
        torch = self._torch
        N = self.horizon
        B = int(x0.shape[0])
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        if classes is not None and not self.num_classes:
            raise ValueError("solve_batch(classes=...) needs a class table: call set_classes first")
        if U_guess is not None and classes is not None:
            raise ValueError("solve_batch(U_guess=...) does not take classes: the warm start solves a plain batch")
        if U_guess is None and guess_passes is not None:
            raise ValueError("solve_batch(guess_passes=...) needs U_guess")
        if U_guess is not None and tuple(U_guess.shape) != (B, 2, N):
            raise ValueError(f"U_guess must have shape ({B}, 2, {N}), got {tuple(U_guess.shape)}")
        cls_t = None if classes is None else self._class_input(classes, B)
        x0_t = self._device_input(x0, (B, 4), "x0")
        if len(ref.shape) == 3 and ref.shape[1] > N + 1:  # rows past N are never read (see solve)
            ref = ref[:, : N + 1]
        ref_t = self._device_input(ref, (B, N + 1, 4), "ref")
        up_t = None if u_prev is None else self._device_input(u_prev, (B, 2), "u_prev")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        ug_t = None if U_guess is None else self._device_input(U_guess, (B, 2, N), "U_guess")
        self._keep = (x0_t, ref_t, up_t, cls_t, ug_t)  # keep inputs alive until the kernels have consumed them
        self.solve_raw(B, x0_t, ref_t, up_t, stream, classes=cls_t, U_guess=ug_t, guess_passes=guess_passes)
        return BatchSolution(self._u0[:B], self._X[:B], self._U[:B], self._status[:B], self._iters[:B],
                             self._active[:B])

    def solve_raw(self, B, x0, ref, u_prev, stream, *, classes=None, U_guess=None, guess_passes=None,
                  after_build=None) -> None:
        """The two library calls of one batch solve, on tensors as the C-ABI reads them: ``mpcqp_build`` (with
        ``classes`` ``mpcqp_build_mixed``), then ``mpcqp_solve`` (with ``U_guess`` ``mpcqp_solve_warm``), enqueued
        on ``stream`` (a torch stream) into the controller's own output tensors (``_u0``, ``_X``, ``_U``,
        ``_status``, ``_iters``, ``_active``; rows ``[:B]``).  Contiguous device tensors: ``x0`` (B, 4), ``ref``
        (B, N+1, 4) and ``U_guess`` (B, 2, N) float64, ``u_prev`` (B, 2) float64 or None, ``classes`` (B,) int32.
        Nothing is converted, checked or kept alive here: ``solve_batch`` does that and then calls this; the
        measuring tools call it directly.  ``after_build``: called between the two enqueues (an event record)."""
        s = ctypes.c_void_p(stream.cuda_stream)
        up = None if u_prev is None else u_prev.data_ptr()
        if classes is None:
            _lib.check(self._L.mpcqp_build(self._ws, B, x0.data_ptr(), ref.data_ptr(), up, s), "mpcqp_build")
        else:
            _lib.check(self._L.mpcqp_build_mixed(self._ws, B, x0.data_ptr(), ref.data_ptr(), up, classes.data_ptr(), s),
                       "mpcqp_build_mixed")
        if after_build is not None:
            after_build()
        outs = (self._u0.data_ptr(), self._X.data_ptr(), self._U.data_ptr(), self._status.data_ptr(),
                self._iters.data_ptr(), self._active.data_ptr())
        if U_guess is not None:
            passes = _lib.DEFAULT_GUESS_PASSES if guess_passes is None else int(guess_passes)
            _lib.check(self._L.mpcqp_solve_warm(self._ws, B, U_guess.data_ptr(), passes, *outs, s), "mpcqp_solve_warm")
        else:
            _lib.check(self._L.mpcqp_solve(self._ws, B, *outs, s), "mpcqp_solve")

    def solve_one(self, x0, ref, u_prev=None, *, U_guess=None, guess_passes=None):
        """One QP for the sequential closed loop of ``TrajectoryTracker.track``, where host overhead
        dominates a B=1 step.  The workspace's own blocks of pinned, device-mapped host memory hold
        the inputs and outputs, which the kernels read and write in place (``mpcqp_stage`` /
        ``mpcqp_solve_served``, include/mpcqp.h): the inputs are written into the block, then ONE
        library call hands the QP to the workspace's resident solver wave (started by the first
        call, gone after 2 ms idle) and waits for its answer -- no kernel launch per step.
        ``x0`` (4,), ``ref`` (>= N+1, 4) -- rows 0..N are used --, ``u_prev`` (2,) host arrays.
        Returns host numpy ``(status, u0, X, U)``; X (4, N+1) and U (2, N) are fresh arrays;
        ``last_iters`` holds a copy of the solve's four counters.
        A fault that surfaces at the synchronisation raises ``_lib.DeviceError``.

        ``U_guess`` (2, N), the layout of ``U``: warm start under ``mpcqp_solve_warm``'s contract
        (``mpcqp_solve_served_warm`` / ``mpcqp_solve_staged_warm``): the guess is written into the
        workspace's guess block and the QP first gets one polish attempt of at most ``guess_passes``
        passes (default ``_lib.DEFAULT_GUESS_PASSES``) from it; a hit has ``last_iters[0] == 0``, a miss
        or an unusable guess runs the cold solve unchanged.  Horizons <= 32 in fast mode; others raise
        ``_lib.LibraryError``.  Without ``U_guess`` the call is the cold one exactly."""
        if U_guess is None and guess_passes is not None:
            raise ValueError("solve_one(guess_passes=...) needs U_guess")
        io = self._one
        if io is None:
            io = self._one = self._stage()
        solve1 = self._solve1
        if U_guess is not None:
            g = np.asarray(U_guess, dtype=float)
            if g.shape != (2, self.horizon):
                raise ValueError(f"U_guess must have shape (2, {self.horizon}), got {g.shape}")
            warm1 = self._solve1_warm
            if warm1 is None:
                raise _lib.LibraryError("this libmpcqp build has no warm B = 1 calls (mpcqp_solve_served_warm)")
            if "guess" not in io:
                io["guess"] = self._stage_guess()
            io["guess"][:] = g
            passes = _lib.DEFAULT_GUESS_PASSES if guess_passes is None else int(guess_passes)
            solve1 = lambda ws: warm1(ws, passes)  # noqa: E731
        io["x0"][:] = x0
        io["ref"][:] = ref[: self.horizon + 1]
        if u_prev is None:
            io["up"][:] = 0.0
        else:
            io["up"][:] = u_prev
        rc = solve1(self._ws)
        if rc != 0:
            _lib.raise_failed(rc, "B=1 solve", sync_fault=True)
        return int(io["status"][0]), io["u0"].copy(), io["X"].copy(), io["U"].copy()

    _one = None

    @property
    def last_iters(self):
        """A copy of the four counters of the last ``solve_one`` (ADMM iterations, polish passes,
        factorizations, line-search trials), read from the output block when asked for: the cold call pays
        nothing for it.  None before the first solve."""
        io = self._one
        return None if io is None else io["iters"].copy()

    def _stage_guess(self):
        """numpy view (2, N) of the workspace's guess block (mpcqp_stage_guess: NaN until written)."""
        hg = ctypes.c_void_p()
        with self._torch.cuda.device(self.device):
            rc = self._L.mpcqp_stage_guess(self._ws, ctypes.byref(hg))
        if rc != 0:
            _lib.raise_failed(rc, "mpcqp_stage_guess", _lib.DeviceError)
        N = self.horizon
        return np.frombuffer((ctypes.c_double * (2 * N)).from_address(hg.value), np.float64).reshape(2, N)

    def _stage(self) -> dict:
        """numpy views of the workspace's B=1 staging blocks (allocated by the first mpcqp_stage;
        an allocation failure raises DeviceError)."""
        N = self.horizon
        # the resident B=1 server (mpcqp_solve_served: no launch per call) unless MPCQP_B1_SERVER=0
        # asks for a launch per call (mpcqp_solve_staged)
        launched = os.environ.get("MPCQP_B1_SERVER", "1") == "0"
        self._solve1 = self._L.mpcqp_solve_staged if launched else self._L.mpcqp_solve_served
        # (None: an older library loaded under MPCQP_ABI_ANY has no warm B = 1 calls; solve_one(U_guess=...) raises)
        self._solve1_warm = getattr(self._L, "mpcqp_solve_staged_warm" if launched else "mpcqp_solve_served_warm", None)
        hin, hout = ctypes.c_void_p(), ctypes.c_void_p()
        offs = (ctypes.c_int32 * 6)()
        with self._torch.cuda.device(self.device):
            rc = self._L.mpcqp_stage(self._ws, ctypes.byref(hin), ctypes.byref(hout), offs)
        if rc != 0:
            _lib.raise_failed(rc, "mpcqp_stage", _lib.DeviceError)
        nin = 4 + 4 * (N + 1) + 2
        nout = offs[5] + 5 * N + 1
        fin = np.frombuffer((ctypes.c_double * nin).from_address(hin.value), np.float64)
        fout = np.frombuffer((ctypes.c_uint8 * nout).from_address(hout.value), np.uint8)
        return dict(
            x0=fin[0:4], ref=fin[4:4 + 4 * (N + 1)].reshape(N + 1, 4), up=fin[4 + 4 * (N + 1):],
            u0=fout[offs[0]:offs[0] + 16].view(np.float64),
            X=fout[offs[1]:offs[1] + 32 * (N + 1)].view(np.float64).reshape(4, N + 1),
            U=fout[offs[2]:offs[2] + 16 * N].view(np.float64).reshape(2, N),
            status=fout[offs[3]:offs[3] + 4].view(np.int32),
            iters=fout[offs[4]:offs[4] + 16].view(np.int32),
            active=fout[offs[5]:offs[5] + 5 * N + 1],
        )

    @property
    def closed(self) -> bool:
        return getattr(self, "_ws", None) is None or not self._ws.value

    def close(self) -> None:
        # the staging blocks belong to the workspace: mpcqp_destroy syncs its stream and frees them
        self._one = None
        if getattr(self, "_ws", None) is not None and self._ws.value:
            self._L.mpcqp_destroy(self._ws)
            self._ws = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


_CACHE: "OrderedDict[tuple, BatchedMPCController]" = OrderedDict()
_CACHE_SIZE = 8


def latency_settings(horizon: int) -> dict:
    """Polish schedule of the latency-bound B=1 drop-in (the reference's sequential loop, one QP
    per call).  The library default (`polish_from` 75 with near-tolerance attempts) is tuned for a
    batch, whose time is its slowest QP; one QP's own cost is lower with an attempt at every
    termination check.  Measured on one vehicle's closed loop with the default single Ruiz pass
    (profiles/r03_s14_schedule_single.json): `polish_from` 25 is the fastest schedule
    at N = 10, 15, 20 and 30.  The horizons past the one-wave kernel keep the default (unmeasured).
    Every schedule ends at the exact optimum; the counters match the C restatement under each
    (tests/test_gpu_parity.py)."""
    return {"polish_from": 25} if horizon <= 32 else {}


# OSQP's default Ruiz pass count (this build's default is 1: DESIGN.md §5)
OSQP_SCALING = 10


def _unpolished_fallback(ctrl: BatchedMPCController) -> bool:
    """The drop-in re-solves a QP its polish did not finish under OSQP's 10 Ruiz passes: with a
    polished exact optimum the scaling only changes the work, never the result; without one the
    returned ADMM iterate depends on it.  Method newton has no ADMM iterate."""
    c = ctrl._cparams
    return c.scaling != OSQP_SCALING and c.method == _lib.METHOD_ADMM


def _single_controller(params, method: str = "admm", **settings) -> BatchedMPCController:
    settings = {**latency_settings(int(params.horizon)), **settings}  # the caller's settings win
    key = _params_key(params, 0 if method == "admm" else 1, settings)
    ctrl = _CACHE.get(key)
    if ctrl is not None and ctrl.closed:
        ctrl = None
    if ctrl is None:
        ctrl = BatchedMPCController(params, 1, method=method, **settings)
        _CACHE[key] = ctrl
        while len(_CACHE) > _CACHE_SIZE:
            _CACHE.popitem(last=False)[1].close()
    else:
        _CACHE.move_to_end(key)
    return ctrl


class MPCController:
    """Quadratic-cost MPC controller with soft bounds and rate limits (``mpc_controller.py:33-145``)."""

    def __init__(self, params: MPCParameters, warm_start: bool = False, guess_passes: Optional[int] = None,
                 **settings) -> None:
        # ``settings``: optional solver settings of ``mpcqp_params`` (rho, max_iter, polish, ...);
        # the reference's constructor takes ``params`` alone and so does every caller of it.
        # ``warm_start``: ``solve(..., u_init=G)`` starts from G ((N, 2), the reference's layout) with one
        # polish attempt of at most ``guess_passes`` passes (``BatchedMPCController.solve_one``); neither
        # is a solver setting, and neither reaches the controller cache's key.
        if warm_start and int(params.horizon) > _lib.WIDE_MIN_HORIZON - 1:
            raise ValueError(f"warm_start needs horizon <= {_lib.WIDE_MIN_HORIZON - 1} (the one-wave kernel), "
                             f"got {int(params.horizon)}")
        self._params = params
        self._settings = dict(settings)
        self.warm_start = bool(warm_start)
        self.guess_passes = guess_passes
        self.last_iters = None  # the four counters of the last solve (None: it never reached the device)

    def solve(
        self,
        x0: FloatArray,
        ref_traj: FloatArray,
        *,
        u_init: Optional[FloatArray] = None,
        u_prev: Optional[FloatArray] = None,
    ) -> Tuple[Optional[FloatArray], Optional[FloatArray], Optional[FloatArray]]:
        # u_init is accepted and ignored, as in the reference (mpc_controller.py:50-51), unless the
        # controller was made with warm_start: then it is the guess, (N, 2) as the reference lays it out.
        N = int(self._params.horizon)
        warm = {}
        if self.warm_start and u_init is not None:
            g = np.asarray(u_init, dtype=float)
            if g.shape != (N, 2):
                raise ValueError(f"u_init must have shape ({N}, 2), got {g.shape}")
            warm = dict(U_guess=np.ascontiguousarray(g.T), guess_passes=self.guess_passes)
        self.last_iters = None
        x0 = np.asarray(x0, dtype=float)
        ref = np.asarray(ref_traj, dtype=float)
        # The reference reads rows 0..N of ref_traj (mpc_controller.py:68,111) after unwrapping
        # the whole yaw column (:59-60); np.unwrap is a prefix operation, so the first N+1 rows
        # unwrap identically on their own.  Fewer rows fail there (ref[N]) and here.
        if ref.ndim != 2 or ref.shape[1] != 4 or ref.shape[0] < N + 1:
            raise ValueError(f"ref_traj must have shape (>= {N + 1}, 4), got {ref.shape}")
        if x0.size != 4:
            raise ValueError(f"x0 must have 4 entries, got shape {x0.shape}")
        x0 = x0.reshape(4)
        up = None if u_prev is None else np.asarray(u_prev, dtype=float).reshape(2)
        # A missing library or device, or a failed allocation, fails loudly here (no CPU fallback
        # exists) ...
        settings = self._settings
        if "scaling" not in settings and not settings.get("polish", 1):
            # no polish: the result is the ADMM iterate, which depends on the scaling -> OSQP's own
            settings = {**settings, "scaling": OSQP_SCALING}
        ctrl = _single_controller(self._params, **settings)
        try:
            status, _, X, U = ctrl.solve_one(x0, ref, up, **warm)
            self.last_iters = getattr(ctrl, "last_iters", None)
        except _lib.LibraryError:
            # ... while a refused or failed launch of the solve maps to (None, None, None), as the
            # reference maps cp.SolverError (mpc_controller.py:133-135).  A fault that surfaces at
            # the stream sync is a DeviceError and propagates.
            LOG.exception("GPU failed during MPC solve")
            return None, None, None
        if status != _lib.SOLVED and _unpolished_fallback(ctrl):
            # Not the polished exact optimum (the solution then no longer depends on the scaling):
            # solve again under OSQP's own 10 Ruiz passes, so the returned unpolished iterate and
            # status are those of the reference's OSQP settings (mpc_controller.py:119-132).  (The
            # converse -- one pass polishes a QP that ten passes would leave unpolished -- returns
            # the exact optimum; it needs a max_iter far below the reference's 60000.)
            ctrl = _single_controller(self._params, **{**settings, "scaling": OSQP_SCALING})
            try:
                status, _, X, U = ctrl.solve_one(x0, ref, up, **warm)
                self.last_iters = getattr(ctrl, "last_iters", None)
            except _lib.LibraryError:
                LOG.exception("GPU failed during MPC solve")
                return None, None, None
        if status == _lib.NUMERICAL_ERROR:
            LOG.error("MPC solve failed with a numerical error")
            return None, None, None
        if status not in (_lib.SOLVED, _lib.SOLVED_INACCURATE):
            LOG.warning("MPC solve returned status %s", _lib.STATUS_NAMES.get(status, status))
            return None, None, None
        return U[:, 0].copy(), X, U

    @property
    def params(self) -> MPCParameters:
        return self._params


__all__ = ["MPCParameters", "MPCController", "BatchedMPCController", "BatchSolution", "latency_settings"]
