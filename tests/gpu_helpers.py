"""What the GPU test files share: the tolerances of the project's contract with its oracle, parameter
blocks, controllers and their outputs, the exact-oracle yardstick, device reads, plans, fleets and cached
cases.  A plain module, imported like ``host_helpers`` and ``param_variants``; test files import from it
and never from each other.  Everything here is a function or a constant: which inputs a test uses and
what it asserts stays written in the test."""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import warm_newton as wn
from host_helpers import E_ARG, E_HORIZON, E_STATE  # noqa: F401  (the return codes, for the test files)
from mpcqp._lib import BAD_CLASS  # noqa: F401  (MPCQP_BAD_CLASS; the binding loads the library lazily)
from mpcqp.scenarios import pairs  # noqa: F401  (the swarm's trips; the swarm test files import it from here)
from param_variants import VARIANTS, resolution, variant

# ---------------------------------------------------------------------- 1. constants
# U, X and u0 of a solved QP against the exact oracle (mpc_oracle.solve_exact), relative as ``rel`` scales:
# tighter than the north star's 1e-5, and about 9x over the two CPU references' own spread
# (test_gpu_params_long.py).  The active codes beside it must be equal.
REL_TOL = 1e-8
# px: closed-loop states against the golden loop / the oracle's loop over the whole run (the QPs match
# to REL_TOL; the plant's sin / cos / tan may differ from glibc by an ulp)
ATOL = 1e-7
OUTS = ("u0", "X", "U", "status", "iters", "active")  # BatchSolution's fields
# every buffer the fleet loop owns; the masks are scratch (the stepped path clears them for vehicles that
# no longer run, the fused loop leaves each vehicle's last-step masks), so stepped-against-fused
# comparisons leave them out
LOOP_BUFFERS = ("state", "u_prev", "path_idx", "phase", "steps", "trace", "u_trace", "X", "status", "u0")
LOOP_BUFFERS_MASK = LOOP_BUFFERS + ("mask",)
TWO_SLOT = ("status", "u0", "mask")  # a nominal and a relaxed slot: vehicles along axis 1
FAIL_NOMINAL = dict(max_iter=1, polish=0, polish_from=0, polish_near=0.0)  # status max_iter on every QP
SWARM_HORIZON = 15


# ---------------------------------------------------------------------- 2. parameter blocks
def base_params(N, res=0.8):
    from mpcqp.config import MPCConfig

    return MPCConfig(horizon=N).to_parameters(res)


def variant_params(name, N):
    """Variant ``name`` of ``param_variants`` at its own resolution; "default" is the block at 0.8."""
    return base_params(N) if name == "default" else variant(base_params(N, resolution(name)), name)


def variant_blocks(N, names=VARIANTS):
    """The named variants as a class table (all nine: dt 0.05 / 0.2 and the 14 px wheelbase among them)."""
    return [variant_params(name, N) for name in names]


def oracle_variant_params(name, N):
    """``variant_params`` on the oracle's own parameter type."""
    import mpc_oracle as mo

    return mo.default_params(N, 0.8) if name == "default" else variant(mo.default_params(N, resolution(name)), name)


# ---------------------------------------------------------------------- 3. controllers and outputs
def controller(params, B, **kw):
    from mpcqp.control.mpc_controller import BatchedMPCController

    return BatchedMPCController(params, B, device="cuda:0", **kw)


def take(sol, names=OUTS):
    import torch

    torch.cuda.synchronize()  # raises if a kernel of the launch faulted
    return {k: getattr(sol, k).cpu().numpy().copy() for k in names}


def solve(params, x0, ref=None, u_prev=None, **kw):
    """The outputs of one batch on a controller of its own: create, solve_batch, take, close.  ``x0`` may
    be a ``scenarios`` batch in place of the three arrays; ``kw`` (method, pairing, solver settings) goes
    to the controller."""
    if hasattr(x0, "x0"):
        x0, ref, u_prev = x0.x0, x0.ref, x0.u_prev
    ctrl = controller(params, max(1, len(x0)), **kw)
    out = take(ctrl.solve_batch(x0, ref, u_prev))
    ctrl.close()
    return out


def solve_with_model(params, x0, ref, u_prev, **settings):
    """``solve`` and the LTV model K1 left in the workspace (None where the solve builds it on chip)."""
    from mpcqp import _lib

    N = int(params.horizon)
    B = len(x0)
    ctrl = controller(params, B, **settings)
    out = take(ctrl.solve_batch(x0, ref, u_prev))
    L = _lib.lib()
    ptr = L.mpcqp_model_buffer(ctrl._ws)
    model = None  # the fused one-wave solve builds its model on chip: no model buffer
    if ptr:
        model = d2h(ptr, np.zeros((B, L.mpcqp_model_stride(N))))
    ctrl.close()
    return out, model


# ---------------------------------------------------------------------- 4. yardsticks
def rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def assert_exact(out, b, exact, what, solved=False):
    """QP ``b`` of ``out`` (``b`` None: ``out`` holds one QP) against one ``solve_exact`` result: U, X and
    u0 within REL_TOL, equal active codes, and with ``solved`` status 1.  Returns the relative error."""
    got = {k: out[k] if b is None else out[k][b] for k in ("U", "X", "u0", "active", "status")}
    if solved:
        assert np.ravel(got["status"])[0] == 1, f"{what} QP {b}: status {got['status']}"
    e = max(rel(got["U"], exact.Umat), rel(got["X"], exact.X), rel(got["u0"], exact.Umat[:, 0]))
    assert e <= REL_TOL, f"{what} QP {b}: rel err {e:.3e}"
    assert np.array_equal(got["active"], exact.active), \
        f"{what} QP {b}: active set differs in rows {np.flatnonzero(got['active'] != exact.active)[:10]}"
    return e


def check_against_oracle(params, x0, ref, u_prev, out, idx, what=""):
    """The QPs ``idx`` of ``out`` against the exact oracle under ``params``; returns the worst error."""
    import mpc_oracle as mo

    worst = 0.0
    for b in idx:
        ex = mo.solve_exact(params, x0[b], ref[b], None if u_prev is None else u_prev[b])
        assert ex.converged, f"{what} QP {b}: the oracle did not converge"
        worst = max(worst, assert_exact(out, b, ex, what))
    return worst


def assert_same(got, want, what, names=OUTS):
    """The named outputs bit for bit."""
    for k in names:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


# ---------------------------------------------------------------------- 5. device access
@lru_cache(maxsize=None)
def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def d2h(ptr, host):
    """Device memory at ``ptr`` into the numpy array ``host`` (after a device synchronize); returns it."""
    _hip().hipDeviceSynchronize()
    assert _hip().hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0  # device -> host
    return host


def is_live(ctrl) -> bool:
    """Whether the workspace's B = 1 server wave is resident."""
    return ctrl._L.mpcqp_debug_serve_fault(ctrl._ws, 3) == 1


# ---------------------------------------------------------------------- 6. plans and fleets
def default_plan(golden):
    g = golden("default_plan.npz")
    return g, [tuple(map(float, p)) for p in g["path"]]


def branches(golden):
    """The RRT* branch splines of the BASELINE config-3 generator (branches.npz)."""
    br = golden("branches.npz")
    off = br["spline_off"]
    return [br["spline"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def varied_fleet(golden, V, seed):
    """V vehicles cycling through the 13 plans (12 branches and the default plan), starts off the path's
    first point by up to 3 px: (default_plan.npz, paths, starts, goals)."""
    g, path = default_plan(golden)
    paths = branches(golden) + [np.asarray(path)]
    rng = np.random.default_rng(seed)
    chosen = [paths[i % len(paths)] for i in range(V)]
    starts = np.array([p[0] for p in chosen]) + rng.uniform(-3, 3, size=(V, 2))
    goals = np.array([p[-1] for p in chosen])
    return g, chosen, starts, goals


def fleet_tracker(N, V, M, sim_steps, map_resolution=0.8, use_graph=True, fused=False, params=None, **settings):
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.fleet import FleetTracker

    return FleetTracker(MPCConfig(horizon=N, sim_steps=sim_steps), map_resolution=map_resolution, max_vehicles=V,
                        max_ref_len=M, device="cuda:0", use_graph=use_graph, fused=fused, params=params, **settings)


def loop_buffers(ft, names=LOOP_BUFFERS):
    """The tracker's named device buffers, whole, on the host."""
    return {k: ft.buffers()[k].cpu().numpy().copy() for k in names}


def snap(ft, names=LOOP_BUFFERS_MASK):
    """``loop_buffers`` cut to the tracker's vehicles (axis 1 of the two-slot buffers)."""
    import torch

    torch.cuda.synchronize()
    V = ft.vehicles
    b = ft.buffers()
    return {k: (b[k][:, :V] if k in TWO_SLOT else b[k][:V]).cpu().numpy().copy() for k in names}


def run_loop(ft, paths, starts, goals, steps=None):
    """Reset, run to the end (or ``steps`` steps), read every loop buffer, close: (result, buffers)."""
    ft.reset_from_plans(paths, starts, goals)
    res = ft.run() if steps is None else (ft.step(steps), ft.result())[1]
    bufs = loop_buffers(ft, LOOP_BUFFERS_MASK)
    ft.close()
    return res, bufs


def planner_params(seed=13):
    from mpcqp.planning.rrt_star import default_planner_parameters

    return default_planner_parameters(max_iterations=1500, random_seed=int(seed))


def swarm(occ, V, sim_steps, **kw):
    from mpcqp.config import MPCConfig
    from mpcqp.pipeline.swarm import Swarm

    return Swarm(occ, MPCConfig(horizon=SWARM_HORIZON, sim_steps=sim_steps), planner_params(),
                 map_resolution=0.8, max_vehicles=V, device="cuda:0", **kw)


def oracle_plan(occ, start, goal, seed, cr=False):
    """RRTStarPlanner.plan (rrt_star.py:201-283) on the host: oracle/rrt_oracle.grow_tree fed the
    seed's own sample stream (draw_samples), oracle extraction and shortcut pruning, then the
    Catmull-Rom smoothing of the host restatement (pinned by branches.npz).  cr: the steer's
    trig correctly rounded (the device's) instead of glibc's."""
    import rrt_oracle as ro
    from mpcqp.common.geometry import catmull_rom_spline
    from mpcqp.planning.rrt_star import draw_samples

    prm = planner_params(seed)
    smp = draw_samples(int(seed), goal, occ.shape, prm.goal_sample_rate, prm.max_iterations)
    nodes, _, gi = ro.grow_tree(occ, start, goal, smp, step=prm.step, goal_radius=prm.goal_radius,
                                rewire_radius=prm.rewire_radius, collision_step=prm.collision_step,
                                trig=ro.CR_TRIG if cr else ro.LIBM_TRIG)
    if gi < 0:
        return None
    path = ro.extract_path(nodes, gi)
    if prm.prune_path and len(path) >= 2:
        pruned = ro.shortcut_prune(occ, path, prm.collision_step)
        if len(pruned) >= 2:
            path = pruned
    if len(path) >= 2 and prm.spline_samples > 1:
        spline = catmull_rom_spline(path, samples_per_segment=prm.spline_samples, alpha=prm.spline_alpha,
                                    dedupe_tol=prm.dedupe_tolerance)
        if len(spline) >= 2:
            path = [tuple(map(float, q)) for q in spline]
    return path


# ---------------------------------------------------------------------- 7. cases
_CASES: dict = {}


def config3_case(N, B, seed, margins=False):
    """B QPs of the config-3 generator at horizon N with their exact optima, each optimum also the case's
    guess, and with ``margins`` their margins (computed once per argument tuple).
    The slack weights put an active row a few 1e-6 outside its bound, so a QP now and then has a row
    within MARGIN of one; with the seeds 5200 + N the oracle finds at most one such QP in 16 at every
    horizon test_gpu_warm.py uses (a property of the inputs alone)."""
    import mpc_oracle as mo
    from mpcqp import scenarios

    key = ("config3", N, B, seed, margins)
    if key not in _CASES:
        params = base_params(N)
        batch = scenarios.config3(B, horizon=N, seed=seed)
        exact = [mo.solve_exact(params, batch.x0[b], batch.ref[b], batch.u_prev[b]) for b in range(B)]
        assert all(e.converged for e in exact)
        case = dict(params=params, x0=batch.x0, ref=batch.ref, u_prev=batch.u_prev, exact=exact,
                    guesses=np.stack([e.Umat for e in exact]))
        if margins:
            case["margins"] = np.array([wn.margin(mo.condense(params, batch.x0[b], batch.ref[b], batch.u_prev[b]),
                                                  exact[b].U) for b in range(B)])
        _CASES[key] = case
    return _CASES[key]


def golden_case(golden, N):
    """The windows of the reference's closed loop at horizon N (``warm_newton.golden_windows``) as a case:
    ``guesses`` are the exact optima, ``shifted`` the guesses a closed loop carries (window k from window
    k - 1's optimum, shifted one step) and ``shifted_runs`` the host model's runs from them."""
    key = ("golden", N)
    if key not in _CASES:
        params = base_params(N, float(golden("default_plan.npz")["map_resolution"]))
        w = wn.golden_windows(golden("closed_loop.npz"), params, N)
        _CASES[key] = dict(params=params, x0=w["x0"], ref=w["window"], u_prev=w["u_prev"], exact=w["exact"],
                           margins=w["margins"], guesses=np.stack([e.Umat for e in w["exact"]]),
                           shifted=w["guesses"], shifted_runs=w["shifted_runs"])
    return _CASES[key]
