"""Closed-loop tracking for a fleet of vehicles, resident on the GPU.

``FleetTracker`` runs the loop body of the reference's ``TrajectoryTracker.track``
(``src/pipeline/control_stage.py:100-150``) for V vehicles at once through
``mpcqp_fleet_run`` (``csrc/mpcqp_fleet.hip``): per step, a masked batched MPC solve
with the reference's relaxation retry (``:33-56``), the plant ``f_discrete`` (``:127``),
the ``path_idx`` advance (``:141-145``) and the goal test (``:147-150``), all on the
device.  The host only checks every ``check_every`` steps whether any vehicle still runs.
``fused=True`` runs the whole loop in ONE launch instead (``mpcqp_fleet_loop``,
``k_fleet_loop`` in ``csrc/mpcqp_solve.h``): each vehicle's wave loops over its own steps, with
no kernel boundary per step, and leaves the loop at its goal -- the same operations, so the
traces are bit-identical to the stepped path.

A heterogeneous fleet (several wheelbases, limits, weights or a per-vehicle ``dt``) runs in the same
single launch: ``set_classes([params_0, ...])`` loads K parameter blocks and ``reset(..., classes=cls)``
gives vehicle ``v`` block ``cls[v]`` (``mpcqp_fleet_loop_mixed``, fused loop only); its buffers equal a
homogeneous fused fleet's under that block bit for bit.

Each vehicle follows exactly the reference's single-vehicle semantics, so vehicle ``v``
reproduces ``TrajectoryTracker.track`` on its own plan (tests/test_gpu_fleet.py).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, replace
from typing import List, Optional, Sequence

import numpy as np

from .. import _lib
from ..control.ref_builder import PackedPaths, build_reference, build_reference_batch
from .control_stage import TrackingResult

PHASE_NAMES = {
    _lib.FLEET_RUNNING: "running",
    _lib.FLEET_GOAL: "goal_reached",
    _lib.FLEET_ABORTED: "aborted",
    _lib.FLEET_OUT_OF_STEPS: "out_of_steps",
}


def relaxed_parameters(base_params):
    """The retry parameters of ``control_stage.py:50-56`` (du_bounds widened by (5, 0.05))."""
    return replace(
        base_params,
        du_bounds=(
            (base_params.du_bounds[0][0] - 5.0, base_params.du_bounds[0][1] + 5.0),
            (base_params.du_bounds[1][0] - 0.05, base_params.du_bounds[1][1] + 0.05),
        ),
    )


def initial_state(path: Sequence, start) -> np.ndarray:
    """``control_stage.py:74-79``: start position, heading of the first path segment, 5 px/s."""
    if len(path) > 1:
        yaw0 = float(np.arctan2(path[1][1] - path[0][1], path[1][0] - path[0][0]))
    else:
        yaw0 = 0.0
    return np.array([start[0], start[1], yaw0, 5.0], dtype=float)


def initial_states(paths: Sequence, starts, packed: Optional[PackedPaths] = None) -> np.ndarray:
    """``initial_state`` of every vehicle, (V, 4): the first segments' headings by one elementwise
    ``np.arctan2`` over all vehicles (the same float64 differences and ufunc as per path), read
    from the packed polylines (``packed``: the pass ``build_reference_batch`` shares)."""
    pk = packed if packed is not None else PackedPaths(paths)
    V = pk.V
    if V and pk.counts.min() == 0:
        raise RuntimeError("Planner returned an empty path")
    many = pk.counts > 1
    i0 = pk.off[:-1].astype(np.int64)
    i1 = np.where(many, i0 + 1, i0)
    p0, p1 = pk.pts[np.minimum(i0, len(pk.pts) - 1)], pk.pts[np.minimum(i1, len(pk.pts) - 1)]
    out = np.empty((V, 4))
    out[:, :2] = np.asarray(starts, dtype=float).reshape(V, 2)
    out[:, 2] = np.where(many, np.arctan2(p1[:, 1] - p0[:, 1], p1[:, 0] - p0[:, 0]), 0.0)
    out[:, 3] = 5.0
    return out


@dataclass
class FleetResult:
    """Per-vehicle outcome of a fleet run (host copies)."""

    states: List[np.ndarray]  # vehicle v: (steps[v], 4) states after each step (TrackingResult.states)
    inputs: List[np.ndarray]  # vehicle v: (steps[v], 2) applied u0
    phase: np.ndarray  # (V,) int32: 0 running, 1 goal reached, 2 aborted, 3 out of steps
    steps: np.ndarray  # (V,) int32
    path_idx: np.ndarray  # (V,) int32

    def tracking_results(self) -> List[TrackingResult]:
        return [TrackingResult(states=[s.copy() for s in st]) for st in self.states]


def closed_loop_settings(horizon: int) -> dict:
    """Polish schedule of the device closed loops (FleetTracker, Swarm).  A fleet's run is the sum
    of each vehicle's step costs, so an attempt at every termination check pays, where the library
    default (`polish_from` 75) is tuned for a one-shot batch's slowest QP.  Measured with the fused
    loop at N = 15 and the default single Ruiz pass (DESIGN.md §9,
    profiles/r03_s14_schedule_fleets.json): `polish_from` 25 against 75 gives -9 / -7 / -10 % at
    100 / 1024 / 4096 vehicles and -5 % on the config-5 swarm.  Past the one-wave kernel the default
    stays (unmeasured)."""
    return {"polish_from": 25} if horizon <= 32 else {}


class FleetTracker:
    """V vehicles in closed loop on one GPU; every loop step runs on the device.

    ``mpc`` is an ``MPCConfig`` (reference or ``mpcqp.config``); the solver parameters
    are ``mpc.to_parameters(map_resolution)`` as in ``control_stage.py:73``, or ``params`` (an
    ``MPCParameters`` of the same horizon) where given: blocks an ``MPCConfig`` cannot express, such as
    a non-diagonal Q.

    ``warm_start=True`` (with ``fused=True``, without classes): inside a launch each vehicle's solves
    start from the ``U`` of its step before, shifted one step (``mpcqp_fleet_loop_warm``): one polish
    attempt of at most ``guess_passes`` passes (default ``_lib.DEFAULT_GUESS_PASSES``) before ADMM, which
    a hit skips; a miss runs the cold solve unchanged.  Results equal the cold loop's to rounding.
    A vehicle's first step of every launch is cold, so a tracker stepped in short launches loses the guess
    each time.  ``carry_guess=True`` (with ``warm_start=True``) keeps it: the tracker owns a ``U_carry``
    tensor (``max_vehicles x 2 x N``, ``buffers()["U_carry"]``, NaN-filled for the loaded vehicles by every
    reset) and ``step`` calls ``mpcqp_fleet_loop_warm_carry``, so a run split into launches of any sizes
    equals the same run in one warm launch bit for bit.  Off by default: a split run's results then differ
    from the uncarried ones at rounding level.

    ``pairing`` ("auto", "on", "off"; passed on to both controllers): two vehicles per wave for N <= 15 in
    the fused loops, the same buffers bit for bit.  The warm loops pair under "on" only; "auto" leaves
    them at one vehicle per wave.  A fleet with classes (``set_classes``) ignores it and runs one vehicle
    per wave unless ``class_pairing="on"`` (handed to the nominal controller, ``mpcqp_set_class_pairing``):
    then two vehicles of the same class share a wave for N <= 15, the same buffers bit for bit.
    """

    warm_start = False
    carry_guess = False
    _carry = None
    guess_passes = _lib.DEFAULT_GUESS_PASSES

    def __init__(self, mpc, *, map_resolution: float, max_vehicles: int, max_ref_len: int,
                 device=None, use_graph: bool = True, fused: bool = False,
                 relaxed_settings: Optional[dict] = None, params=None, warm_start: bool = False,
                 guess_passes: Optional[int] = None, carry_guess: bool = False, class_pairing: str = "off",
                 **settings) -> None:
        import torch

        from ..control.mpc_controller import BatchedMPCController

        # warm start (mpcqp_fleet_loop_warm): inside a launch every solve starts from the step before
        if warm_start and not fused:
            raise ValueError("warm_start needs fused=True: only the fused loop carries a guess from step to step")
        if guess_passes is not None and not warm_start:
            raise ValueError("guess_passes needs warm_start=True")
        if carry_guess and not warm_start:
            raise ValueError("carry_guess needs warm_start=True: the carried guess belongs to the warm loop")
        self.warm_start = bool(warm_start)
        self.carry_guess = bool(carry_guess)
        self.guess_passes = _lib.DEFAULT_GUESS_PASSES if guess_passes is None else int(guess_passes)
        self._torch = torch
        self.mpc = mpc
        self.params = mpc.to_parameters(map_resolution) if params is None else params
        self._ref_dt = float(mpc.dt if params is None else params.dt)  # reset_from_plans builds references with it
        self.horizon = int(self.params.horizon)
        self.max_vehicles = int(max_vehicles)
        self.max_ref_len = int(max_ref_len)
        self.use_graph = bool(use_graph)
        self.fused = bool(fused)
        # a closed loop pays every vehicle's step costs, not a batch's slowest QP: the polish schedule
        # defaults to closed_loop_settings (the caller's settings win)
        loop = closed_loop_settings(self.horizon)
        settings = {**loop, **settings}
        self._nominal = BatchedMPCController(self.params, self.max_vehicles, device=device,
                                             class_pairing=class_pairing, **settings)
        # the retry's solver settings default to the nominal ones (control_stage.py:50-56 changes
        # only du_bounds and the reference speed)
        rs = settings if relaxed_settings is None else {**loop, **relaxed_settings}
        self._relaxed = BatchedMPCController(relaxed_parameters(self.params), self.max_vehicles,
                                             device=self._nominal.device, **rs)
        self.device = self._nominal.device
        self._L = _lib.lib()
        # the guess carried across launches (mpcqp_fleet_loop_warm_carry): NaN = none yet, a cold first step
        self._carry = (torch.full((self.max_vehicles, 2, self.horizon), float("nan"), dtype=torch.float64,
                                  device=self.device) if self.carry_guess else None)
        self._bufs = None
        self._fleet = None
        self.vehicles = 0
        self.num_classes = 0
        self._class_params = None

    # ------------------------------------------------------------------
    def set_classes(self, params_list, settings=None, relaxed_settings=None) -> None:
        """Per-vehicle parameter classes for the fused loop: block k of the nominal controller is
        ``params_list[k]``, block k of the retry ``relaxed_parameters(params_list[k])`` (both through
        ``BatchedMPCController.set_classes``: ``settings`` / ``relaxed_settings`` are one dict for all
        classes or a list with one per class, on top of the controller's own; the retry's default to
        the nominal ones, as in the constructor).  ``reset(..., classes=cls)`` then gives vehicle v
        block ``cls[v]`` (class 0 without ``classes``), and ``step`` / ``run`` call
        ``mpcqp_fleet_loop_mixed``.  ``None`` or ``[]`` drops the tables: the tracker is homogeneous
        again.  Needs ``fused=True`` and a horizon of at most 32 (the stepped loop has no classes)."""
        if params_list:
            if not self.fused:
                raise ValueError("set_classes needs fused=True: only the fused loop runs per-vehicle classes")
            if self.warm_start:
                raise ValueError("set_classes does not combine with warm_start: the warm loop runs one parameter block")
            if self.horizon > 32:
                raise ValueError(f"set_classes needs a horizon <= 32 (the fused loop), got {self.horizon}")
        self._load_classes(params_list, settings, relaxed_settings)

    def _load_classes(self, params_list, settings=None, relaxed_settings=None) -> None:
        """Load the class tables on both controllers and record them (``None`` or ``[]``: drop them), unchecked:
        what ``set_classes`` and ``Swarm.set_classes`` do after their own checks."""
        if not params_list:
            self._nominal.set_classes(None)
            self._relaxed.set_classes(None)
            self.num_classes = 0
            self._class_params = None
            return
        params_list = list(params_list)
        self._nominal.set_classes(params_list, settings)
        self._relaxed.set_classes([relaxed_parameters(p) for p in params_list],
                                  settings if relaxed_settings is None else relaxed_settings)
        self.num_classes = len(params_list)
        self._class_params = params_list

    def _class_indices(self, classes, V: int):
        """``classes`` as the int32 device tensor ``mpcqp_fleet_loop_mixed`` reads (None without a table)."""
        from ..control.mpc_controller import class_input

        if classes is None:
            if not self.num_classes:
                return None
            return self._torch.zeros((max(V, 1),), dtype=self._torch.int32, device=self.device)
        if not self.num_classes:
            raise ValueError("classes=... needs a class table: call set_classes first")
        t = class_input(self._torch, self.device, classes, V)
        return t if V else self._torch.zeros((1,), dtype=self._torch.int32, device=self.device)

    def _class_dts(self, cls, V: int) -> np.ndarray:
        """dt of each vehicle's class (the tracker's own where the index is out of range: that
        vehicle is aborted before it reads its reference)."""
        dts = np.array([float(p.dt) for p in self._class_params])
        c = cls[:V].cpu().numpy().astype(np.int64)
        ok = (c >= 0) & (c < len(dts))
        return np.where(ok, dts[np.where(ok, c, 0)], float(self.params.dt))

    # ------------------------------------------------------------------
    def reset(self, ref_globals: Sequence[np.ndarray], states0: np.ndarray, goals: np.ndarray,
              max_steps: Optional[int] = None, *, classes=None) -> None:
        """Load V references (each ``(M_v, 4)``, ``build_reference`` output), start states and goals.
        ``classes`` (int array or int32 device tensor, shape ``(V,)``): vehicle v's block of
        ``set_classes``; an index outside the table aborts that vehicle with status ``BAD_CLASS``."""
        V = len(ref_globals)
        if V > self.max_vehicles:
            raise ValueError(f"{V} vehicles exceed max_vehicles {self.max_vehicles}")
        cls = self._class_indices(classes, V)
        start = self._start_inputs(V, states0, goals, max_steps)
        lens = np.array([len(r) for r in ref_globals], dtype=np.int32)
        if V and (lens.min() < 1 or lens.max() > self.max_ref_len):
            raise ValueError(f"reference lengths must be in [1, {self.max_ref_len}]")
        M = self.max_ref_len
        ref = np.zeros((max(V, 1), M, 4))
        for v, r in enumerate(ref_globals):
            r = np.asarray(r, dtype=float)
            if r.ndim != 2 or r.shape[1] != 4:
                raise ValueError("each reference must have shape (M, 4)")
            ref[v, : len(r)] = r
        self._load(V, ref, lens, *start, cls)

    def _start_inputs(self, V: int, states0, goals, max_steps: Optional[int]):
        """``(states0 (V, 4), goals (V, 2), max_steps)`` as ``_load`` takes them (``max_steps`` None: the
        config's ``sim_steps``)."""
        states0 = np.asarray(states0, dtype=float).reshape(V, 4)
        goals = np.asarray(goals, dtype=float).reshape(V, 2)
        max_steps = int(self.mpc.sim_steps if max_steps is None else max_steps)
        if max_steps < 1:
            raise ValueError("max_steps must be >= 1")
        return states0, goals, max_steps

    def _load(self, V: int, ref: Optional[np.ndarray], lens: np.ndarray, states0: np.ndarray, goals: np.ndarray,
              max_steps: int, cls=None) -> None:
        """The fleet's device buffers for V vehicles (the inputs as ``_start_inputs`` returns them);
        ``ref`` None: the references are copied in on the device afterwards (reset_device), so no host
        copy of them is built or uploaded."""
        torch = self._torch
        M = self.max_ref_len
        N = self.horizon
        dev = dict(device=self.device)
        f64 = torch.float64
        i32 = torch.int32
        b = {
            "ref_global": (torch.from_numpy(ref).to(**dev) if ref is not None
                           else torch.zeros((max(V, 1), M, 4), dtype=f64, **dev)),
            "ref_len": torch.from_numpy(np.maximum(lens, 1) if V else np.ones(1, np.int32)).to(**dev),
            "goal": torch.from_numpy(goals if V else np.zeros((1, 2))).to(**dev),
            "state": torch.from_numpy(states0 if V else np.zeros((1, 4))).to(**dev),
            "u_prev": torch.zeros((max(V, 1), 2), dtype=f64, **dev),
            "path_idx": torch.zeros((max(V, 1),), dtype=i32, **dev),
            "phase": torch.zeros((max(V, 1),), dtype=i32, **dev),
            "steps": torch.zeros((max(V, 1),), dtype=i32, **dev),
            "mask": torch.zeros((2, max(V, 1)), dtype=torch.uint8, **dev),
            "status": torch.zeros((2, max(V, 1)), dtype=i32, **dev),
            "u0": torch.zeros((2, max(V, 1), 2), dtype=f64, **dev),
            "X": torch.zeros((max(V, 1), 4, N + 1), dtype=f64, **dev),
            "trace": torch.zeros((max(V, 1), max_steps, 4), dtype=f64, **dev),
            "u_trace": torch.zeros((max(V, 1), max_steps, 2), dtype=f64, **dev),
        }
        f = _lib.MpcqpFleet()
        f.vehicles = V
        f.ref_stride = M
        f.max_steps = max_steps
        for name, t in b.items():
            setattr(f, name, t.data_ptr())
        # the vehicles' class indices (mpcqp_fleet_loop_mixed's argument, not a member of mpcqp_fleet)
        b["cls"] = cls if cls is not None else torch.zeros((max(V, 1),), dtype=i32, **dev)
        if self._carry is not None:  # a new run starts without a guess
            self._carry[:V].fill_(float("nan"))
            b["U_carry"] = self._carry
        self._bufs = b
        self._fleet = f
        self.vehicles = V
        self.max_steps = max_steps

    def reset_from_plans(self, paths: Sequence, starts: np.ndarray, goals: np.ndarray,
                         max_steps: Optional[int] = None, *, device_reference: bool = False, classes=None):
        """``control_stage.py:69-87`` per vehicle: references from the planned paths, start states.
        With ``classes`` vehicle v's reference is built with its class's ``dt`` (host path; the batched
        device builder takes one ``dt``, so ``device_reference=True`` needs classes that share it).

        ``device_reference=True`` builds the references with the batched GPU ``build_reference``
        (``mpcqp_build_reference``) straight into the fleet's buffers; otherwise on the host.
        Returns the host references (or ``(ref, ref_len)`` device tensors)."""
        V = len(paths)
        cls = self._class_indices(classes, V)
        cls = None if cls is None else cls[:V]
        dts = np.full(V, self._ref_dt) if cls is None else self._class_dts(cls, V)
        if device_reference and cls is not None and len(set(float(p.dt) for p in self._class_params)) > 1:
            raise ValueError("device_reference=True builds every reference with one dt, the classes have several: "
                             "build the references on the host (device_reference=False)")
        packed = PackedPaths(paths)
        states0 = initial_states(paths, starts, packed)
        if device_reference:
            ref, ref_len = build_reference_batch(paths, self.mpc.v_px_s, self.horizon, float(dts[0]) if V else self._ref_dt,
                                                 device=self.device, ref_stride=self.max_ref_len, packed=packed)
            self.reset_device(ref, ref_len, states0, goals, max_steps, classes=cls)
            return ref, ref_len
        refs = [build_reference(path, self.mpc.v_px_s, self.horizon, float(dts[v])) for v, path in enumerate(paths)]
        self.reset(refs, states0, goals, max_steps, classes=cls)
        return refs

    def reset_device(self, ref, ref_len, states0: np.ndarray, goals: np.ndarray,
                     max_steps: Optional[int] = None, *, classes=None) -> None:
        """Load references already on the device: ``ref`` (V, max_ref_len, 4) float64 and
        ``ref_len`` (V,) int32 as produced by ``build_reference_batch``.  ``classes``: as ``reset``."""
        torch = self._torch
        V = int(ref.shape[0])
        if V > self.max_vehicles:
            raise ValueError(f"{V} vehicles exceed max_vehicles {self.max_vehicles}")
        cls = self._class_indices(classes, V)
        if int(ref.shape[1]) != self.max_ref_len:
            raise ValueError(f"ref rows {int(ref.shape[1])} != max_ref_len {self.max_ref_len}")
        lens = ref_len.cpu().numpy()
        if V and (lens.min() < 1 or lens.max() > self.max_ref_len):
            raise ValueError(f"reference lengths must be in [1, {self.max_ref_len}] (build_reference_batch "
                             f"reports overflow as negative lengths)")
        self._load(V, None, lens.astype(np.int32), *self._start_inputs(V, states0, goals, max_steps), cls)
        self._bufs["ref_global"][:V].copy_(ref)
        self._bufs["ref_len"][:V].copy_(ref_len.to(torch.int32))

    # ------------------------------------------------------------------
    def step(self, steps: int = 1, stream=None) -> None:
        """Enqueue ``steps`` closed-loop steps (asynchronous on the current torch stream)."""
        if self._fleet is None:
            raise RuntimeError("reset() the fleet first")
        torch = self._torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        s = ctypes.c_void_p(stream.cuda_stream)
        if self.num_classes:  # a class per vehicle (set_classes: fused only)
            call, args = "mpcqp_fleet_loop_mixed", (self._bufs["cls"].data_ptr(), int(steps))
        elif self.carry_guess:  # warm, and the first step of this launch from the last step of the launch before
            call, args = "mpcqp_fleet_loop_warm_carry", (int(steps), self.guess_passes, self._carry.data_ptr())
        elif self.warm_start:  # fused, each step's solves started from the step before (cold at every launch)
            call, args = "mpcqp_fleet_loop_warm", (int(steps), self.guess_passes)
        elif self.fused:
            call, args = "mpcqp_fleet_loop", (int(steps),)
        else:
            call, args = "mpcqp_fleet_run", (int(steps), int(self.use_graph))
        _lib.check(getattr(self._L, call)(*self.loop_args(), *args, s), call)

    def loop_args(self) -> tuple:
        """The three leading arguments of every loop call (``step``'s and ``Swarm.run``'s): the two workspaces and
        the loaded fleet."""
        return self._nominal._ws, self._relaxed._ws, ctypes.byref(self._fleet)

    def launch_info(self) -> dict:
        """What the last loop launch did: the nominal controller's ``launch_info()``."""
        return self._nominal.launch_info()

    def running(self) -> int:
        return int((self._bufs["phase"][: self.vehicles] == _lib.FLEET_RUNNING).sum().item())

    def run(self, sim_steps: Optional[int] = None, check_every: int = 16) -> FleetResult:
        """Step until every vehicle has left the RUNNING phase (or ``sim_steps`` steps)."""
        total = self.max_steps if sim_steps is None else min(int(sim_steps), self.max_steps)
        if self.fused:  # one launch: every vehicle leaves the loop by itself
            if self.vehicles:
                self.step(total)
            return self.result()
        done = 0
        while done < total and self.vehicles:
            k = min(check_every, total - done)
            self.step(k)
            done += k
            if self.running() == 0:
                break
        return self.result()

    def result(self) -> FleetResult:
        b = self._bufs
        V = self.vehicles
        self._torch.cuda.synchronize(self.device)
        steps = b["steps"][:V].cpu().numpy().copy()
        trace = b["trace"][:V].cpu().numpy()
        utr = b["u_trace"][:V].cpu().numpy()
        return FleetResult(
            states=[trace[v, : steps[v]].copy() for v in range(V)],
            inputs=[utr[v, : steps[v]].copy() for v in range(V)],
            phase=b["phase"][:V].cpu().numpy().copy(),
            steps=steps,
            path_idx=b["path_idx"][:V].cpu().numpy().copy(),
        )

    def buffers(self) -> dict:
        """The device tensors behind the fleet state (views; for inspection and tests)."""
        return self._bufs

    def close(self) -> None:
        self._nominal.close()
        self._relaxed.close()


__all__ = ["FleetTracker", "FleetResult", "relaxed_parameters", "initial_state", "initial_states", "closed_loop_settings",
           "PHASE_NAMES"]
