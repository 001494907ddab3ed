"""BASELINE config 5: a swarm of vehicles on one inflated grid, planned, tracked and re-planned
on the GPU with a per-step replan trigger.

``Swarm.run`` chains the batched stages for V vehicles:
  1. plan    -- ``BatchedRRTStarPlanner.paths_batch``: one RRT* tree per vehicle, path extraction,
               shortcut pruning and Catmull-Rom smoothing on the device (``rrt_star.py:201-289``);
  2. refs    -- ``build_reference_batch`` (GPU) straight into the fleet's buffers;
  3. track + replan -- ``mpcqp_swarm_run`` (``csrc/mpcqp_swarm.hip``), every step on the device:
               the fleet closed-loop step (``control_stage.py:100-150``), then the trigger the
               reference lists as roadmap (``README.md:146-148``) -- a vehicle farther than
               ``replan_distance`` from ``ref[path_idx]`` after its step, or one whose QP stayed
               unsolved after relaxation (aborted) -- and, in the same step, its replanning from
               where it stands (RRT* with its next seed ``seed + 7919 (r + 1)``, pruning,
               smoothing, build_reference); pose, speed and u_prev carry over, path_idx restarts at
               0.  At most ``max_replans`` per vehicle.  The whole step is one hipGraph replay; the
               host only polls every ``check_every`` steps whether any vehicle still runs.  With
               ``fused=True``: ``mpcqp_swarm_loop``, the fused fleet loop with the trigger inside
               (max_replans + 1 launches, the replanning kernels between them).  With
               ``warm_start=True`` as well: ``mpcqp_swarm_loop_warm``, the same launches with each
               vehicle's solves started from its step before (cold at the first step of a launch, so
               a replanned vehicle starts its new reference cold).  After
               ``Swarm.set_classes`` (``fused=True``): ``mpcqp_swarm_loop_mixed`` /
               ``mpcqp_swarm_loop_mixed_warm``, the same launches with a parameter class per vehicle
               (``run(..., classes=)``).  With ``grids=`` (a map that changes with time):
               ``mpcqp_swarm_loop_map`` (``fused=True``) or ``mpcqp_swarm_run_map`` -- a vehicle that has
               taken k steps lives on grid ``min(k // epoch_steps, T - 1)``, the trigger also fires when
               one of the next ``lookahead`` reference rows lies on an occupied cell of that grid, and
               the replanning plans on it.
Every vehicle between replans follows the reference's single-vehicle loop exactly.
"""
from __future__ import annotations

import ctypes
import time
from dataclasses import dataclass, field, fields
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from ..planning.rrt_star import BatchedRRTStarPlanner, PlannerParameters, pcg64_states
from .fleet import FleetTracker

# (fused, map, mixed, warm) -> the C call of Swarm.run and what it takes between the swarm struct and the
# stepped calls' (steps, use_graph).  A combination that is not here is refused before run gets this far
# (__init__, set_classes, the fleet tracker's check of classes without a table, run's own of classes on a map).
_CALLS = {
    (True, False, False, False): ("mpcqp_swarm_loop", ()),
    (True, False, False, True): ("mpcqp_swarm_loop_warm", ("passes",)),
    (True, False, True, False): ("mpcqp_swarm_loop_mixed", ("cls",)),
    (True, False, True, True): ("mpcqp_swarm_loop_mixed_warm", ("cls", "passes")),
    (True, True, False, False): ("mpcqp_swarm_loop_map", ("map",)),
    (False, False, False, False): ("mpcqp_swarm_run", ()),
    (False, True, False, False): ("mpcqp_swarm_run_map", ("map",)),
}

REPLAN_SEED_STRIDE = 7919  # replan r of vehicle v draws from default_rng(seed_v + 7919 (r + 1))


def replan_seed(seed: int, r: int) -> int:
    return int(seed) + REPLAN_SEED_STRIDE * (int(r) + 1)


def grid_index(k, epoch_steps: int, num_grids: int):
    """The grid a vehicle that has taken ``k`` steps lives on: ``min(k // epoch_steps, T - 1)`` (array or int)."""
    return np.minimum(np.asarray(k) // int(epoch_steps), int(num_grids) - 1)


def replan_grids(replans, replan_steps, epoch_steps: int, num_grids: int) -> np.ndarray:
    """``(V, R)``: the grid each replan planned on -- ``grid_index`` of the step count recorded in
    ``replan_steps`` (``steps`` where the replan gave a plan, ``-steps - 1`` where it failed) -- and -1 where no
    replan happened."""
    rs = np.asarray(replan_steps).astype(np.int64)
    k = np.where(rs >= 0, rs, -rs - 1)
    happened = np.arange(rs.shape[1])[None, :] < np.asarray(replans).reshape(-1, 1)
    return np.where(happened, grid_index(k, epoch_steps, num_grids), -1).astype(np.int64)


def map_hits(states, grids: np.ndarray, epoch_steps: int) -> np.ndarray:
    """Per vehicle, the number of steps after which the vehicle's own cell (the planner's lookup: round half to
    even, clipped) was occupied in the grid of that moment: ``states[v][i]`` is the state after step ``i + 1``."""
    T, H, W = grids.shape
    hits = np.zeros(len(states), dtype=np.int64)
    for v, st in enumerate(states):
        st = np.asarray(st, dtype=float).reshape(-1, 4)
        if not len(st):
            continue
        g = grid_index(np.arange(1, len(st) + 1), epoch_steps, T)
        xi = np.clip(np.rint(st[:, 0]), 0, W - 1).astype(np.int64)
        yi = np.clip(np.rint(st[:, 1]), 0, H - 1).astype(np.int64)
        hits[v] = int((grids[g, yi, xi] == 0).sum())
    return hits


@dataclass
class SwarmResult:
    states: List[np.ndarray]  # per vehicle: states after each step, across replans
    phase: np.ndarray  # final MPCQP_FLEET_* phase
    steps: np.ndarray  # closed-loop steps per vehicle
    replans: np.ndarray  # replan attempts per vehicle
    planned: np.ndarray  # initial plan succeeded
    paths: List[Optional[list]] = field(default_factory=list)  # initial plan per vehicle (None: no plan)
    replan_steps: Optional[np.ndarray] = None  # (V, max_replans): steps[v] at replan r, -steps-1 failed, 0 unused
    last_replan_start: Optional[np.ndarray] = None  # (V, 2): where the last replan started
    last_replan_path: List[Optional[np.ndarray]] = field(default_factory=list)  # its final path (None: failed/none)
    # the last replan failed because its smoothed path exceeded path_cap (not an RRT* failure)
    replan_over_capacity: Optional[np.ndarray] = None
    inputs: List[np.ndarray] = field(default_factory=list)  # per vehicle: applied u0 per step
    timings: Dict[str, float] = field(default_factory=dict)
    # a swarm on a changing map (Swarm(grids=...)); None otherwise
    replan_cause: Optional[np.ndarray] = None  # (V, max_replans): _lib.REPLAN_ABORTED / _OFF_TRACK / _BLOCKED, 0 unused
    replan_grid: Optional[np.ndarray] = None  # (V, max_replans): the grid each replan planned on, -1 unused
    hits: Optional[np.ndarray] = None  # (V,): steps after which the vehicle stood on an occupied cell of its grid


class Swarm:
    warm_start = False
    guess_passes = _lib.DEFAULT_GUESS_PASSES

    def __init__(self, occupancy: np.ndarray, mpc, planner: PlannerParameters, *, map_resolution: float,
                 max_vehicles: int, max_ref_len: int = 512, device=None, replan_distance: float = 15.0,
                 max_replans: int = 2, path_cap: int = 6144, use_graph: bool = True, fused: bool = False,
                 warm_start: bool = False, guess_passes: Optional[int] = None, grids: Optional[np.ndarray] = None,
                 epoch_steps: Optional[int] = None, lookahead: int = 20, **settings) -> None:
        # warm start (mpcqp_swarm_loop_warm): opt-in, the fused swarm only.  Results equal the cold swarm's
        # to rounding, so a replanned vehicle's new plan may differ from the cold swarm's (RRT* decisions
        # sit on knife edges); guess_passes <= 0 is the cold swarm bit for bit.
        if warm_start and not fused:
            raise ValueError("warm_start needs fused=True: only the fused swarm loop carries a guess from step to step")
        if guess_passes is not None and not warm_start:
            raise ValueError("guess_passes needs warm_start=True")
        # a map that changes with time (mpcqp_swarm_loop_map / mpcqp_swarm_run_map): grids (T, H, W), grids[0] the
        # grid the initial plans are made on; a vehicle that has taken k steps lives on grid
        # min(k // epoch_steps, T - 1); lookahead: reference rows ahead of path_idx tested for occupied cells
        self.grids, self.epoch_steps, self.lookahead = self._check_grids(occupancy, grids, epoch_steps, lookahead,
                                                                         warm_start)
        self.warm_start = bool(warm_start)
        self.guess_passes = _lib.DEFAULT_GUESS_PASSES if guess_passes is None else int(guess_passes)
        # path_cap: smoothed points a replan may produce.  The default is the most that the device
        # reference builder stages (kRefCap, csrc/mpcqp_swarm.hip), so a replanned path is never cut
        # shorter than a reference could be built from; capacity failures are reported apart from
        # RRT* failures (SwarmResult.replan_over_capacity).
        self.occupancy = np.ascontiguousarray(occupancy, dtype=np.uint8)
        self.mpc = mpc
        self.planner = BatchedRRTStarPlanner(self.occupancy, planner, device=device)
        # settings: solver settings of the vehicles' QPs (mpcqp_params names), as FleetTracker's
        self.fleet = FleetTracker(mpc, map_resolution=map_resolution, max_vehicles=max_vehicles,
                                  max_ref_len=max_ref_len, device=self.planner.device, **settings)
        self.device = self.planner.device
        self.replan_distance = float(replan_distance)
        self.max_replans = int(max_replans)
        self.path_cap = int(path_cap)
        self.use_graph = bool(use_graph)
        # fused: the run as max_replans + 1 launches of the fused fleet loop with the trigger inside
        # (mpcqp_swarm_loop) instead of one graph-replayed launch sequence per step
        self.fused = bool(fused)
        self._L = _lib.lib()

    grids = None  # class defaults: a swarm on one grid
    epoch_steps, lookahead = 1, 0

    @staticmethod
    def _check_grids(occupancy, grids, epoch_steps, lookahead, warm_start):
        if grids is None:
            if epoch_steps is not None:
                raise ValueError("epoch_steps needs grids=")
            return None, 1, 0
        grids = np.ascontiguousarray(grids, dtype=np.uint8)
        occupancy = np.asarray(occupancy)
        if grids.ndim != 3 or grids.shape[0] < 1 or grids.shape[1:] != occupancy.shape:
            raise ValueError(f"grids must have shape (T, {occupancy.shape[0]}, {occupancy.shape[1]}) with T >= 1, "
                             f"got {grids.shape}")
        if not np.array_equal(grids[0], occupancy):
            raise ValueError("grids[0] must equal occupancy: the initial plans are made on it")
        if warm_start:
            raise ValueError("grids with warm_start=True: the changing map runs the cold swarm only")
        if epoch_steps is None:
            if grids.shape[0] > 1:
                raise ValueError("grids with more than one grid need epoch_steps")
            epoch_steps = 1
        if int(epoch_steps) < 1:
            raise ValueError(f"epoch_steps must be >= 1, got {epoch_steps}")
        if not 0 <= int(lookahead) <= _lib.SWARM_MAP_MAX_LOOKAHEAD:
            raise ValueError(f"lookahead must lie in [0, {_lib.SWARM_MAP_MAX_LOOKAHEAD}], got {lookahead}")
        return grids, int(epoch_steps), int(lookahead)

    def set_classes(self, params_list, settings=None, relaxed_settings=None) -> None:
        """Per-vehicle parameter classes for the fused swarm (``mpcqp_swarm_loop_mixed``, with
        ``warm_start=True`` ``mpcqp_swarm_loop_mixed_warm``): block k of the nominal controller is
        ``params_list[k]``, block k of the retry ``relaxed_parameters(params_list[k])``; ``settings`` /
        ``relaxed_settings`` as ``FleetTracker.set_classes`` takes them.  ``run(..., classes=cls)`` then
        runs vehicle v under block ``cls[v]`` (class 0 without ``classes``).  ``None`` or ``[]`` drops the
        tables: the swarm is homogeneous again.  Needs ``fused=True`` and a horizon of at most 32 (the
        stepped swarm has no classes), and one dt: the replanning builds every vehicle's new reference
        with the swarm's ``mpc.dt``, so every class must have it."""
        if params_list:
            if self.grids is not None:
                raise ValueError("set_classes on a swarm with grids: the changing map runs one parameter block")
            if not self.fused:
                raise ValueError("set_classes needs fused=True: only the fused swarm loop runs per-vehicle classes")
            if self.fleet.horizon > 32:
                raise ValueError(f"set_classes needs a horizon <= 32 (the fused loop), got {self.fleet.horizon}")
            params_list = list(params_list)
            for k, p in enumerate(params_list):
                if float(p.dt) != float(self.mpc.dt):
                    raise ValueError(f"the swarm runs one dt: class {k} has dt {float(p.dt)}, the swarm's replanning "
                                     f"builds references with mpc.dt = {float(self.mpc.dt)}")
        # not through FleetTracker.set_classes: the swarm's tracker is built with fused=False (the swarm
        # issues the fused calls itself) and would refuse
        self.fleet._load_classes(params_list, settings, relaxed_settings)

    def _plan(self, starts, goals, seeds):
        """Final paths of every problem (growth, extraction, pruning and smoothing on the device);
        returns (success mask, paths with the start alone where no plan was found)."""
        found = self.planner.paths_batch(starts, goals, seeds, smoothing="device")
        ok = np.array([p is not None for p in found], dtype=bool)
        paths = [p if p is not None else [tuple(s)] for p, s in zip(found, starts)]
        return ok, paths, found

    def _swarm_struct(self, V: int, seeds, planned) -> tuple:
        torch = self.fleet._torch
        dev = dict(device=self.device)
        R = max(self.max_replans, 1)
        M = int(self.planner.params.max_iterations) + 2
        S = self.fleet.max_ref_len
        table = np.zeros((max(V, 1), R, 4), dtype=np.uint64)
        if self.max_replans:
            for v in range(V):
                table[v] = pcg64_states([replan_seed(seeds[v], r) for r in range(self.max_replans)])
        f64, i32 = torch.float64, torch.int32
        n = max(V, 1)
        b = {
            "rng_table": torch.from_numpy(table).to(**dev),
            # vehicles without an initial plan never replan (the reference raises, control_stage.py:69-72)
            "replans": torch.from_numpy(np.where(planned, 0, self.max_replans).astype(np.int32)
                                        if V else np.zeros(1, np.int32)).to(**dev),
            "replan_step": torch.zeros((n, R), dtype=i32, **dev),
            "start_goal": torch.zeros((n, 4), dtype=f64, **dev),
            "nodes": torch.zeros((n, M, 4), dtype=f64, **dev),
            "count": torch.zeros((n,), dtype=i32, **dev),
            "meta": torch.zeros((n, 2), dtype=i32, **dev),
            "raw": torch.zeros((n, M, 2), dtype=f64, **dev),
            "raw_len": torch.zeros((n,), dtype=i32, **dev),
            "pruned": torch.zeros((n, M, 2), dtype=f64, **dev),
            "pruned_len": torch.zeros((n,), dtype=i32, **dev),
            "smooth": torch.zeros((n, self.path_cap, 2), dtype=f64, **dev),
            "smooth_len": torch.zeros((n,), dtype=i32, **dev),
            "new_ref": torch.zeros((n, S, 4), dtype=f64, **dev),
            "new_len": torch.zeros((n,), dtype=i32, **dev),
        }
        occ = torch.from_numpy(self.occupancy).to(**dev)
        s = _lib.MpcqpSwarm()
        s.rrt = self.planner._c
        s.occupancy = occ.data_ptr()
        pp = self.planner.params
        s.prune = int(bool(pp.prune_path))
        s.spline_samples = int(pp.spline_samples)
        s.spline_alpha = float(pp.spline_alpha)
        s.dedupe_tol = float(pp.dedupe_tolerance)
        s.desired_speed = float(self.mpc.v_px_s)
        s.dt = float(self.mpc.dt)
        s.horizon = int(self.fleet.horizon)
        s.max_replans = self.max_replans
        s.replan_distance = self.replan_distance
        s.path_cap = self.path_cap
        for k, t in b.items():
            setattr(s, k, t.data_ptr())
        b["occupancy"] = occ
        return s, b

    def _map_struct(self, V: int) -> tuple:
        """``mpcqp_swarm_map`` of this swarm's grids and its device buffers (grids, grid_of, replan_cause)."""
        torch = self.fleet._torch
        n, R = max(V, 1), max(self.max_replans, 1)
        b = {"grids": torch.from_numpy(self.grids).to(device=self.device),
             "grid_of": torch.zeros((n,), dtype=torch.int32, device=self.device),
             "replan_cause": torch.zeros((n, R), dtype=torch.uint8, device=self.device)}
        m = _lib.MpcqpSwarmMap()
        m.num_grids, m.epoch_steps, m.lookahead = int(self.grids.shape[0]), self.epoch_steps, self.lookahead
        for k, t in b.items():
            setattr(m, k, t.data_ptr())
        return m, b

    def run(self, starts: np.ndarray, goals: np.ndarray, seeds=None, *, sim_steps: Optional[int] = None,
            check_every: int = 10, classes=None, before_launch: Optional[Callable[[dict], None]] = None) -> SwarmResult:
        """``classes`` (int array or int32 device tensor, shape ``(V,)``; after ``set_classes``): vehicle
        v's block; an index outside the table aborts that vehicle with status ``BAD_CLASS`` and it never
        replans.  Without ``classes`` a swarm with a table runs every vehicle under class 0.
        ``before_launch``: called with the fleet's buffers once the plans and references are on the device,
        before the first launch (a replan overwrites a vehicle's reference rows; this is where to copy them)."""
        torch = self.fleet._torch
        starts = np.asarray(starts, dtype=float).reshape(-1, 2)
        goals = np.asarray(goals, dtype=float).reshape(-1, 2)
        V = len(starts)
        seeds = np.arange(V) if seeds is None else np.asarray(seeds)
        total = int(self.mpc.sim_steps if sim_steps is None else sim_steps)
        t = {}
        t0 = time.perf_counter()
        planned, paths, found = self._plan(starts, goals, seeds)
        t["plan_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        mixed = classes is not None or bool(self.fleet.num_classes)  # classes without a table: refused below
        ckw = dict(classes=self.fleet._class_indices(classes, V)) if mixed else {}
        self.fleet.reset_from_plans(paths, starts, goals, max_steps=total, device_reference=True, **ckw)
        fb = self.fleet.buffers()
        if (~planned).any():  # no plan: the vehicle never starts (the reference raises, :69-72)
            fb["phase"][torch.from_numpy(np.flatnonzero(~planned)).to(self.device)] = _lib.FLEET_ABORTED
        sw, sb = self._swarm_struct(V, seeds, planned)
        on_map = self.grids is not None
        if on_map and mixed:
            raise ValueError("classes on a swarm with grids: the changing map runs one parameter block")
        mp, mb = self._map_struct(V) if on_map else (None, None)
        self._map_buffers = mb  # kept for inspection (grid_of)
        if before_launch is not None:
            before_launch(fb)
        torch.cuda.synchronize(self.device)
        t["refs_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        stream = torch.cuda.current_stream(self.device)
        call, names = _CALLS[(bool(self.fused), on_map, mixed, bool(self.warm_start))]
        given = {"map": lambda: ctypes.byref(mp), "cls": lambda: fb["cls"].data_ptr(),
                 "passes": lambda: self.guess_passes}
        args = tuple(given[n]() for n in names)

        def launch(*tail):
            _lib.check(getattr(self._L, call)(*self.fleet.loop_args(), ctypes.byref(sw), *args, *tail,
                                              ctypes.c_void_p(stream.cuda_stream)), call)

        done = 0
        if self.fused and V:
            launch()
            done = total
        while done < total and V:
            k = min(check_every, total - done)
            launch(int(k), int(self.use_graph))
            done += k
            if not self.fleet.running():
                break
        torch.cuda.synchronize(self.device)
        t["track_replan_s"] = time.perf_counter() - t0
        return self._result(V, planned, found, sb, mb, t)

    def _result(self, V: int, planned, found, sb: dict, mb: Optional[dict], t: dict) -> SwarmResult:
        """The finished run on the host: the fleet's result, and from the swarm's buffers ``sb`` (and the map's
        ``mb``, None off a map) the replans, their steps, the last replanned paths and the map extras."""
        r = self.fleet.result()
        replans = sb["replans"][:V].cpu().numpy().astype(np.int64)
        replans = np.where(planned, replans, 0)
        rsteps = sb["replan_step"][:V, : max(self.max_replans, 1)].cpu().numpy()
        sg = sb["start_goal"][:V].cpu().numpy()
        sl = sb["smooth_len"][:V].cpu().numpy()
        smooth = sb["smooth"][:V].cpu().numpy()
        last_paths = []
        over_cap = np.zeros(V, dtype=bool)
        for v in range(V):
            over_cap[v] = bool(replans[v] and rsteps[v, replans[v] - 1] < 0 and sl[v] == -1)
            if replans[v] and rsteps[v, replans[v] - 1] >= 0 and sl[v] >= 1:
                last_paths.append(smooth[v, : sl[v]].copy())
            else:
                last_paths.append(None)
        extra = {}
        if mb is not None:  # causes from the device; the grids of the replans and the hits are host arithmetic on the result
            cause = mb["replan_cause"][:V, : max(self.max_replans, 1)].cpu().numpy()
            extra = dict(replan_cause=np.where(np.arange(cause.shape[1])[None, :] < replans[:, None], cause, 0),
                         replan_grid=replan_grids(replans, rsteps, self.epoch_steps, self.grids.shape[0]),
                         hits=map_hits(r.states, self.grids, self.epoch_steps))
        return SwarmResult(states=r.states, phase=r.phase, steps=r.steps, replans=replans, planned=planned,
                           paths=found, replan_steps=rsteps, last_replan_start=sg[:, :2].copy(),
                           last_replan_path=last_paths, inputs=r.inputs, timings=t,
                           replan_over_capacity=over_cap, **extra)

    def launch_info(self) -> dict:
        """What the last fused-loop launch did (``FleetTracker.launch_info``)."""
        return self.fleet.launch_info()

    def close(self) -> None:
        """Free the two controllers' workspaces; a second call does nothing."""
        self.fleet.close()


# ------------------------------------------------------------------ multi-GPU: vehicles sharded over ranks
# The vehicles of the swarm are independent (the reference tracks each one alone,
# control_stage.py:100-150; nothing couples two vehicles), so config 5 on G GPUs gives each rank a
# contiguous block of vehicles -- with the vehicles' own seeds, so every vehicle does exactly what it
# does in a one-GPU run -- and the only collective is the gather of the per-vehicle results at the end
# (no data-path exchange: weak scaling in the vehicles, strong scaling of a fixed swarm).

def shard_vehicles(V: int, world: int, rank: int) -> Tuple[int, int]:
    """[lo, hi) of rank's contiguous block; block sizes differ by at most one (bench.shard_bounds)."""
    base, extra = divmod(int(V), int(world))
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


_PER_VEHICLE_ARRAYS = ("phase", "steps", "replans", "planned", "replan_steps", "last_replan_start",
                       "replan_over_capacity", "replan_cause", "replan_grid", "hits")
_PER_VEHICLE_LISTS = ("states", "paths", "last_replan_path", "inputs")


def merge_swarm_results(parts: Sequence[SwarmResult]) -> SwarmResult:
    """Rank-ordered shard results -> the swarm's result in vehicle order; timings: max over ranks
    (the ranks run concurrently, the slowest one sets the swarm's wall time)."""
    parts = [p for p in parts if p is not None]
    kw = {}
    for f in fields(SwarmResult):
        vals = [getattr(p, f.name) for p in parts]
        if f.name in _PER_VEHICLE_ARRAYS:
            vals = [v for v in vals if v is not None and len(v)]
            kw[f.name] = np.concatenate(vals) if vals else None
        elif f.name in _PER_VEHICLE_LISTS:
            kw[f.name] = [x for v in vals for x in v]
        elif f.name == "timings":
            keys = sorted({k for v in vals for k in v})
            kw[f.name] = {k: max(v.get(k, 0.0) for v in vals) for k in keys}
    return SwarmResult(**kw)


def run_swarm_sharded(run: Callable[..., SwarmResult], starts, goals, seeds, *, rank: int, world: int,
                      all_gather_object: Callable[[list, object], None], classes=None, **kwargs) -> SwarmResult:
    """Run rank's block of the swarm with ``run`` (``Swarm.run`` of this rank's device) and gather
    every rank's result: each rank returns the whole swarm's result, in vehicle order.  ``classes``
    (``(V,)``, a mixed swarm) is cut like the seeds; None passes nothing to ``run``."""
    starts = np.asarray(starts, dtype=float).reshape(-1, 2)
    goals = np.asarray(goals, dtype=float).reshape(-1, 2)
    V = len(starts)
    seeds = np.arange(V) if seeds is None else np.asarray(seeds)
    lo, hi = shard_vehicles(V, world, rank)
    if classes is not None:
        kwargs["classes"] = classes[lo:hi]
    local = run(starts[lo:hi], goals[lo:hi], seeds=seeds[lo:hi], **kwargs) if hi > lo else None
    parts: list = [None] * world
    all_gather_object(parts, local)
    return merge_swarm_results(parts)


__all__ = ["Swarm", "SwarmResult", "replan_seed", "REPLAN_SEED_STRIDE", "shard_vehicles", "merge_swarm_results",
           "run_swarm_sharded", "grid_index", "replan_grids", "map_hits"]
