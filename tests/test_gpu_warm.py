"""GPU tests of the warm start (``mpcqp_solve_warm`` / ``k_solve_warm``, ``mpcqp_fleet_loop_warm`` /
``k_fleet_loop_warm``): one polish attempt from a caller's guess before ADMM.

The contract (include/mpcqp.h): a hit returns the exact optimum with ``iters[0] == 0``; a miss, and an
unusable guess, run the cold solve unchanged -- u0, X, U, status and active bit for bit, ``iters[0]`` the
cold value, ``iters[1..3]`` the cold values plus the attempt's.  So every QP here is held either to the
exact oracle (``mpc_oracle.solve_exact``: <= 1e-8 relative, equal active codes, as test_gpu_params.py)
or to a cold ``mpcqp_solve`` of the same build, and where the host model (``warm_newton``) says the
guess's active set is the optimum's, with every row clear of its bounds, to the hit itself.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import warm_newton as wn
from gpu_helpers import (ATOL, E_ARG, E_HORIZON, E_STATE, LOOP_BUFFERS_MASK, OUTS, assert_exact, base_params, config3_case,
                         controller, default_plan, fleet_tracker, golden_case, loop_buffers, run_loop, take, varied_fleet)

pytestmark = pytest.mark.gpu

_SAME = ("u0", "X", "U", "status", "active")


def _assert_miss(warm, cold, b, passes, what):
    """The miss clause: the cold solve's answer bit for bit, its ADMM count, its polish counters plus
    the attempt's (1..passes passes, at most one factorization per pass, any number of line-search trials)."""
    for k in _SAME:
        np.testing.assert_array_equal(warm[k][b], cold[k][b], err_msg=f"{what} QP {b}: {k}")
    wi, ci = warm["iters"][b], cold["iters"][b]
    assert wi[0] == ci[0], (what, b, wi, ci)
    assert 1 <= wi[1] - ci[1] <= passes, (what, b, wi, ci)
    assert 0 <= wi[2] - ci[2] <= wi[1] - ci[1], (what, b, wi, ci)
    assert wi[3] >= ci[3], (what, b, wi, ci)


def _solve_pair(case, guesses, passes=None, rows=None):
    """(warm, cold) outputs of one controller on the case's QPs (`rows`: a subset)."""
    rows = np.arange(len(case["x0"])) if rows is None else np.asarray(rows)
    ctrl = controller(case["params"], len(rows))
    args = (case["x0"][rows], case["ref"][rows], case["u_prev"][rows])
    warm = take(ctrl.solve_batch(*args, U_guess=np.asarray(guesses)[rows], guess_passes=passes))
    cold = take(ctrl.solve_batch(*args))
    ctrl.close()
    return warm, cold


# ---------------------------------------------------------------------- 1. the exact guess
@pytest.mark.parametrize("N", [1, 2, 10, 15, 16, 23, 24, 29, 32])
def test_exact_guess_hits(cuda, golden, N):
    """From the optimum itself the attempt converges at once: N = 1 (nothing to shift), 15 / 16 (the
    pair limit), 23 / 24 (kept model, packed Pbar), 29 (the spill range), 32 (every lane a column)."""
    cases = [("config3", config3_case(N, 16, 5200 + N, margins=True))]
    if N in (10, 15):
        cases.append(("golden", golden_case(golden, N)))
    for name, case in cases:
        B = len(case["x0"])
        warm, _ = _solve_pair(case, case["guesses"], passes=2)
        clear = case["margins"] > wn.MARGIN
        print(f"N={N} {name}: {int(clear.sum())} of {B} clear of their bounds; iters {warm['iters'].tolist()}")
        assert (~clear).sum() <= (0 if name == "golden" else B // 10)
        for b in range(B):
            assert_exact(warm, b, case["exact"][b], f"N={N} {name}", solved=True)
            if clear[b]:
                assert warm["iters"][b, 0] == 0, (N, name, b, warm["iters"][b])
                assert 1 <= warm["iters"][b, 1] <= 2, (N, name, b, warm["iters"][b])


# ---------------------------------------------------------------------- 2. the shifted guess
@pytest.mark.parametrize("N", [10, 15])
def test_shifted_guess_along_the_golden_loop(cuda, golden, N):
    """What a closed loop carries: window k starts from window k - 1's optimum, shifted one step."""
    from mpcqp import _lib

    case = golden_case(golden, N)
    rows = np.arange(1, len(case["x0"]))
    warm, cold = _solve_pair(case, case["shifted"], rows=rows)
    hits = warm["iters"][:, 0] == 0
    expected = np.array([r.passes == 1 and r.margin > wn.MARGIN for r in case["shifted_runs"][1:]])
    print(f"N={N}: {int(hits.sum())} hits of {len(rows)}, {int(expected.sum())} expected from the host model; "
          f"attempt passes of the hits {warm['iters'][hits, 1].tolist()}")
    assert expected.sum() >= 25
    for i in range(len(rows)):
        assert_exact(warm, i, case["exact"][rows[i]], f"N={N} window {rows[i]}", solved=True)
        if expected[i]:
            assert hits[i], (N, rows[i], warm["iters"][i])
        if not hits[i]:
            _assert_miss(warm, cold, i, _lib.DEFAULT_GUESS_PASSES, f"N={N} window {rows[i]}")


# ---------------------------------------------------------------------- 3. unusable guesses
@pytest.mark.parametrize("how", ["nan", "inf", "passes0"])
def test_unusable_guess_is_the_cold_solve_bit_for_bit(cuda, how):
    N = 10
    case = config3_case(N, 16, 5200 + N, margins=True)
    B = len(case["x0"])
    g = case["guesses"].copy()
    odd = np.arange(B) % 2 == 1
    if how == "nan":
        g[odd, 0, N - 1] = np.nan  # one entry each: the last acceleration
    elif how == "inf":
        g[odd, 1, 0] = -np.inf  # the first steering angle
    warm, cold = _solve_pair(case, g, passes=0 if how == "passes0" else None)
    unusable = np.ones(B, bool) if how == "passes0" else odd
    for k in OUTS:  # iters included
        np.testing.assert_array_equal(warm[k][unusable], cold[k][unusable], err_msg=k)
    clear = case["margins"] > wn.MARGIN
    for b in np.flatnonzero(~unusable):
        assert_exact(warm, b, case["exact"][b], how, solved=True)
        if clear[b]:
            assert warm["iters"][b, 0] == 0, (how, b, warm["iters"][b])
    assert (~unusable & clear).sum() >= (0 if how == "passes0" else B // 2 - 1)


# ---------------------------------------------------------------------- 4. poor guesses
@pytest.mark.parametrize("N", [10, 20, 32])
@pytest.mark.parametrize("kind", ["zeros", "uniform", "huge"])
def test_poor_guess_never_changes_an_answer(cuda, kind, N):
    """A guess far from the optimum costs its attempt and nothing else: every QP either hits (the exact
    optimum, no ADMM) or returns the cold solve's answer."""
    from mpcqp import _lib

    case = config3_case(N, 16, 5200 + N, margins=True)
    B = len(case["x0"])
    p = case["params"]
    if kind == "zeros":
        g = np.zeros((B, 2, N))
    elif kind == "huge":
        g = np.full((B, 2, N), 1e12)
    else:
        rng = np.random.default_rng(7 + N)
        ub = np.asarray(p.u_bounds, dtype=float)  # (2, 2): (lo, hi) per input
        g = rng.uniform(3.0 * ub[:, 0][None, :, None], 3.0 * ub[:, 1][None, :, None], size=(B, 2, N))
    warm, cold = _solve_pair(case, g)
    hits = warm["iters"][:, 0] == 0
    print(f"{kind} N={N}: {int(hits.sum())} hits of {B}; warm iters {warm['iters'].tolist()}")
    for b in range(B):
        if hits[b]:
            assert_exact(warm, b, case["exact"][b], f"{kind} N={N}", solved=True)
        else:
            _assert_miss(warm, cold, b, _lib.DEFAULT_GUESS_PASSES, f"{kind} N={N}")


# ---------------------------------------------------------------------- 5. errors
def _raw_warm(ctrl, B, guess, status, passes=2):
    import torch

    s = ctypes.c_void_p(torch.cuda.current_stream(ctrl.device).cuda_stream)
    return ctrl._L.mpcqp_solve_warm(ctrl._ws, B, None if guess is None else guess.data_ptr(), passes, None, None, None,
                                    status.data_ptr(), None, None, s)


@pytest.mark.parametrize("how", ["null_guess", "n40", "reproducible", "after_mixed", "no_build"])
def test_warm_solve_errors_write_nothing(cuda, how):
    import torch
    from mpcqp import scenarios

    N = 40 if how == "n40" else 10
    B = 4
    batch = scenarios.config3(B, horizon=N, seed=9)
    params = base_params(N)
    ctrl = controller(params, B, **({"reproducible": 1} if how == "reproducible" else {}))
    if how == "after_mixed":
        ctrl.set_classes([params, params])
        ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=np.zeros(B, np.int32))
    elif how != "no_build":
        ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev)
    status = torch.full((B,), 77, dtype=torch.int32, device="cuda:0")
    guess = torch.zeros((B, 2, N), dtype=torch.float64, device="cuda:0")
    rc = _raw_warm(ctrl, B, None if how == "null_guess" else guess, status)
    torch.cuda.synchronize()
    want = {"null_guess": E_ARG, "n40": E_HORIZON, "reproducible": E_HORIZON, "after_mixed": E_STATE,
            "no_build": E_STATE}[how]
    assert rc == want, (how, rc, ctrl._L.mpcqp_last_error())
    assert (status.cpu().numpy() == 77).all()
    if how == "null_guess":  # the build is still there: the call with a guess solves it
        assert _raw_warm(ctrl, B, guess, status) == 0
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 1).all()
    ctrl.close()


def test_guess_may_be_the_output_buffer(cuda):
    """U_guess aliasing U: each wave reads its row before it writes it."""
    N = 10
    case = config3_case(N, 16, 5200 + N, margins=True)
    B = len(case["x0"])
    ctrl = controller(case["params"], B)
    args = (case["x0"], case["ref"], case["u_prev"])
    first = ctrl.solve_batch(*args)
    again = take(ctrl.solve_batch(*args, U_guess=first.U))  # the controller's own U tensor
    ctrl.close()
    clear = case["margins"] > wn.MARGIN
    for b in range(B):
        assert_exact(again, b, case["exact"][b], "aliased", solved=True)
        if clear[b]:
            assert again["iters"][b, 0] == 0, (b, again["iters"][b])


# ---------------------------------------------------------------------- 6. the fleet
@pytest.mark.parametrize("N,steps", [(10, None), (1, 6), (32, 6)])
def test_warm_loop_without_passes_is_the_cold_loop_bit_for_bit(cuda, golden, N, steps):
    """guess_passes = 0: every solve is cold, every buffer is mpcqp_fleet_loop's (one vehicle per wave)."""
    V = 4
    if N == 10:  # the golden plan, to its goal
        g, path = default_plan(golden)
        plans = ([path] * V, np.tile(g["start"], (V, 1)), np.tile(g["goal"], (V, 1)))
        kw = dict(sim_steps=100, map_resolution=float(g["map_resolution"]))
    else:
        plans = varied_fleet(golden, V, seed=31 + N)[1:]
        kw = dict(sim_steps=steps)
    _, cold = run_loop(fleet_tracker(N, V, 128, fused=True, pairing="off", **kw), *plans, steps=steps)
    _, warm = run_loop(fleet_tracker(N, V, 128, fused=True, warm_start=True, guess_passes=0, **kw), *plans, steps=steps)
    for k in LOOP_BUFFERS_MASK:
        np.testing.assert_array_equal(warm[k], cold[k], err_msg=k)
    assert (cold["steps"][:V] > 0).all()


@pytest.mark.parametrize("N,sim_steps", [(10, 100), (15, 300)])
def test_warm_loop_reproduces_the_reference_closed_loop(cuda, golden, N, sim_steps):
    """Each step's optimum is the cold loop's to rounding, so the warm loop follows the reference's own
    loop (closed_loop.npz) within the cold loop's tolerances, and the cold fused loop itself closely."""
    from mpcqp import _lib

    g, path = default_plan(golden)
    loop = golden("closed_loop.npz")
    V = 4
    plans = ([path] * V, np.tile(g["start"], (V, 1)), np.tile(g["goal"], (V, 1)))
    kw = dict(sim_steps=sim_steps, map_resolution=float(g["map_resolution"]))
    rc, cold = run_loop(fleet_tracker(N, V, 64, fused=True, pairing="off", **kw), *plans)
    rw, warm = run_loop(fleet_tracker(N, V, 64, fused=True, warm_start=True, **kw), *plans)
    ref_states = loop[f"N{N}_states"]
    assert (rw.phase == _lib.FLEET_GOAL).all() and (rw.steps == len(ref_states)).all()
    for v in range(V):
        np.testing.assert_allclose(rw.states[v], ref_states, rtol=0, atol=ATOL)
        np.testing.assert_allclose(rw.inputs[v], loop[f"N{N}_u0"], rtol=0, atol=1e-6)
    for k in ("phase", "steps", "path_idx"):
        np.testing.assert_array_equal(warm[k], cold[k], err_msg=k)
    print(f"N={N}: max |trace - cold trace| {np.abs(warm['trace'] - cold['trace']).max():.3e}")
    np.testing.assert_allclose(warm["trace"], cold["trace"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(warm["u_trace"], cold["u_trace"], rtol=0, atol=1e-7)


def test_warm_loop_relaxation_branches(cuda, golden):
    """test_gpu_fleet.py's relaxation scenario for the fused loop (a vehicle whose QP is non-finite is
    retried relaxed and aborts alone) under warm start: the same phases and the same accepted branch."""
    from mpcqp import _lib

    N, steps, V = 10, 20, 6
    g, path = default_plan(golden)
    out = []
    for kw in (dict(pairing="off"), dict(warm_start=True)):
        ft = fleet_tracker(N, V, 64, steps, float(g["map_resolution"]), fused=True, **kw)
        ft.reset_from_plans([path] * V, np.tile(g["start"], (V, 1)), np.tile(g["goal"], (V, 1)))
        ft.buffers()["state"][2, 0] = float("nan")
        res = ft.run()
        out.append((res, loop_buffers(ft, ("mask", "status", "phase", "steps"))))
        ft.close()
    (rc, cold), (rw, warm) = out
    for k in ("mask", "status", "phase", "steps"):
        np.testing.assert_array_equal(warm[k], cold[k], err_msg=k)
    assert warm["mask"][:, 2].tolist() == [1, 1]  # nominal solve, then the relaxed retry
    assert (warm["status"][:, 2] == _lib.NUMERICAL_ERROR).all()
    assert rw.phase[2] == _lib.FLEET_ABORTED and rw.steps[2] == 0
    others = [v for v in range(V) if v != 2]
    assert (rw.phase[others] == _lib.FLEET_OUT_OF_STEPS).all() and (rw.steps[others] == steps).all()
    assert warm["mask"][1, others].sum() == 0  # nobody else retried: the nominal branch every step
    loop = golden("closed_loop.npz")
    for v in others:
        np.testing.assert_allclose(rw.states[v], loop["N10_states"][:steps], rtol=0, atol=ATOL)


def test_warm_loop_longest_first_dispatch_order(cuda, golden):
    """More vehicles than wave slots (8 per CU): the warm loop dispatches through the order table as the
    plain loop does.  Without passes every step is cold (include/mpcqp.h): the plain fused loop's buffers bit
    for bit; with the default passes the same phases, step counts and path indices."""
    import torch
    from mpcqp.control.ref_builder import build_reference
    from mpcqp.pipeline.fleet import initial_states

    N, steps = 3, 4
    V = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    _, paths, starts, goals = varied_fleet(golden, V, seed=6)
    s0 = initial_states(paths, starts)
    out, refs = [], None
    for kw in ({}, dict(warm_start=True, guess_passes=0), dict(warm_start=True)):
        ft = fleet_tracker(N, V, 128, steps, fused=True, **kw)
        if refs is None:  # varied_fleet cycles through 13 plans: one reference per plan, built once
            distinct = [build_reference(paths[i], ft.mpc.v_px_s, N, ft.mpc.dt) for i in range(13)]
            assert all(paths[v] is paths[v - 13] for v in range(13, 26))
            refs = [distinct[v % 13] for v in range(V)]
        ft.reset(refs, s0, goals)
        ft.run()
        out.append(loop_buffers(ft, LOOP_BUFFERS_MASK))
        ft.close()
    plain, cold, warm = out
    assert (plain["steps"] == steps).any()
    for k in LOOP_BUFFERS_MASK:
        np.testing.assert_array_equal(cold[k], plain[k], err_msg=k)
    for k in ("phase", "steps", "path_idx"):
        np.testing.assert_array_equal(warm[k], plain[k], err_msg=k)
