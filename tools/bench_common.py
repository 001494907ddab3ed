"""How the tools measure, and the inputs they share.  A plain module: it imports neither
torch nor the library until a function that needs one is called, so the measuring rule is tested on the host
(tests/test_bench_common.py).  Tools import from here and from ``mpcqp``, never from each other.

The rule: the sides ("legs") of a comparison run in one process and alternate within each repeat, the order
rotating from repeat to repeat; repeat 0 warms up and is dropped; medians are reported with min and max."""
from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT / "rrt-mpc_amd") not in sys.path:
    sys.path.insert(0, str(ROOT / "rrt-mpc_amd"))


# ---------------------------------------------------------------------- the measuring rule
def interleaved(legs: dict, reps: int, setup=None, *, rotate: bool = True, warmup: bool = True, value=None):
    """Run the named ``legs`` (callables without arguments) ``reps`` times each, taking turns within every
    repeat: repeat r visits them in the order ``names[r % n:] + names[:r % n]`` (``rotate=False``: always as
    given), after ``setup()`` where one is given.  With ``warmup`` a repeat 0 runs first and what its legs
    return is dropped.  Returns ``(values, last)``: per leg the returns of the timed repeats in repeat order
    (``value(ret)`` of each where ``value`` is given), and per leg its last return whole.  Nothing is caught:
    an exception from a leg or from ``setup`` ends the run there, and no further leg is started."""
    names = list(legs)
    values = {k: [] for k in names}
    last = {}
    for r in range(reps + 1 if warmup else reps):
        if setup is not None:
            setup()
        shift = r % len(names) if rotate else 0
        for k in names[shift:] + names[:shift]:
            last[k] = legs[k]()
            if r or not warmup:
                values[k].append(last[k] if value is None else value(last[k]))
    return values, last


def timed(fn, sync, clock):
    """``(seconds, fn())`` of the window synchronise, clock, ``fn()``, synchronise, clock.  The tools pass
    ``torch.cuda.synchronize`` and ``time.perf_counter``."""
    sync()
    t0 = clock()
    out = fn()
    sync()
    return clock() - t0, out


def summary(ts) -> dict:
    """Median, min, max and every value of a list of times, in the order given."""
    return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "all": list(ts)}


# ---------------------------------------------------------------------- shared inputs
@lru_cache(maxsize=None)
def default_grid() -> np.ndarray:
    """The default plan's inflated occupancy grid (80 x 80, 1 = free), loaded once; not to be written to."""
    from mpcqp import scenarios

    return scenarios.load_default_plan()["occupancy"]


def class_blocks(base, K):
    """K parameter blocks of one horizon and dt: the base, then other wheelbases, limits and weights."""
    from dataclasses import replace

    pool = [
        base,
        replace(base, wheelbase_px=base.wheelbase_px * 4.0),  # the wheelbase at map_resolution 0.2
        replace(base, u_bounds=((-5.0, 4.0), (-0.3, 0.25)), v_bounds=(2.0, 18.0), du_bounds=((-3.0, 2.5), (-0.05, 0.04))),
        replace(base, q=np.array(base.q) * 2.0, q_terminal=np.array(base.q_terminal) * 2.0),
        replace(base, r=np.array(base.r) * 4.0),
        replace(base, v_bounds=(0.0, 12.0)),
        replace(base, wheelbase_px=base.wheelbase_px * 2.0, du_bounds=((-8.0, 8.0), (-0.1, 0.1))),
        replace(base, slack_velocity=1e4, slack_input=5e3, slack_rate=5e3),
    ]
    if not 1 <= K <= len(pool):
        raise SystemExit(f"--classes takes 1..{len(pool)}")
    return pool[:K]


def track_args(path, start, goal) -> tuple:
    """``(planning, maps)`` as ``TrajectoryTracker.track`` reads them, for one planned path."""
    planning = SimpleNamespace(plan=SimpleNamespace(success=True, path=[tuple(map(float, q)) for q in path]))
    return planning, SimpleNamespace(start=tuple(start), goal=tuple(goal))


def default_track_args() -> tuple:
    """``track_args`` of the default (config-1) plan."""
    from mpcqp import scenarios

    plan = scenarios.load_default_plan()
    return track_args(plan["path"], plan["start"], plan["goal"])


_COUNTS = {"vehicle_steps": lambda r: int(r.steps.sum()), "goal_reached": lambda r: int((r.phase == 1).sum()),
           "aborted": lambda r: int((r.phase == 2).sum()), "replans": lambda r: int(r.replans.sum())}


def loop_counts(res, keys=("vehicle_steps", "goal_reached", "aborted")) -> dict:
    """The closed-loop counts a leg reports of its ``FleetResult`` or ``SwarmResult`` (``replans``: a swarm's)."""
    return {k: _COUNTS[k](res) for k in keys}
