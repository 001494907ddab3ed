"""GPU parity: libmpcqp.so (K1 + K2 on the MI355X) against the oracle.

Tolerances (north star: "<= 1e-5 rel-err, bit-exact active set"):
  * K1 LTV model vs the C restatement:           <= 1e-12 relative (sin/cos ulps only)
  * K1 unwrapped yaw vs numpy:                   bit-exact
  * K2 U/X vs the exact oracle (mpc_oracle.py):  <= 1e-8 relative  (tighter than the 1e-5 target)
  * active-set codes vs the exact oracle:        identical
"""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import OUTS, REL_TOL, base_params, check_against_oracle, controller, d2h, rel, solve, take

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("cfg", ["config2", "config3", "config4"])
def test_batches_match_exact_oracle(cuda, cfg):
    from mpcqp import scenarios

    batch = {"config2": lambda: scenarios.config2(1024), "config3": lambda: scenarios.config3(512),
             "config4": lambda: scenarios.config4(512)}[cfg]()
    params = base_params(batch.horizon)
    out = solve(params, batch.x0, batch.ref, batch.u_prev)
    assert (out["status"] == 1).all(), np.unique(out["status"], return_counts=True)
    check_against_oracle(params, batch.x0, batch.ref, batch.u_prev, out, range(0, batch.size, 7))


def test_newton_method_matches(cuda):
    from mpcqp import scenarios

    batch = scenarios.config3(256)
    params = base_params(20)
    out = solve(params, batch.x0, batch.ref, batch.u_prev, method="newton")
    assert (out["status"] == 1).all()
    assert (out["iters"][:, 0] == 0).all()
    check_against_oracle(params, batch.x0, batch.ref, batch.u_prev, out, range(0, 256, 5))


@pytest.mark.parametrize("cfg,N,B", [("config2", 20, 1024), ("config3", 4, 1024), ("config3", 8, 1024),
                                     ("config3", 10, 1024), ("config3", 16, 1024), ("config3", 24, 1024),
                                     ("config3", 31, 1024), ("config3", 32, 1024), ("config4", 30, 4096)])
def test_iteration_indexing_bit_exact_on_product_path(cuda, cfg, N, B):
    """The product kernel (fast mode) against the C restatement on whole batches: all four counters
    (ADMM iterations, polish passes, factorizations, line-search trials), statuses and active sets
    identical on every QP -- the north star's bit-exact iteration / active-set indexing.  N = 4 / 8 / 16
    run the whole-wave kernel's short broadcasts (no lane moves at 2N <= 16, one permlane16 stage at
    2N <= 32; batches below the pairing threshold)."""
    import cpu_solver
    from mpcqp import scenarios

    batch = {"config2": lambda: scenarios.config2(B),
             "config3": lambda: scenarios.config3(B, horizon=N, seed=5000 + N),
             "config4": lambda: scenarios.config4(B)}[cfg]()
    params = base_params(batch.horizon)
    out = solve(params, batch.x0, batch.ref, batch.u_prev)
    ref = cpu_solver.cpu_solve(params, batch.x0, batch.ref, batch.u_prev)
    same = (out["iters"] == ref["iters"]).all(axis=1)
    assert same.all(), f"QPs {np.flatnonzero(~same)[:10]} disagree on iteration counts"
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["active"], ref["active"])
    assert rel(out["U"], ref["U"]) <= REL_TOL


@pytest.mark.parametrize("schedule", [
    {},                                       # the default schedule (one Ruiz pass, early + near-tolerance polish)
    {"polish_near": 0.0},                     # early polish from iteration polish_from (75) only
    {"polish_from": 0, "polish_near": 0.0},   # OSQP's order: polish only after ADMM stops
    {"polish_from": 25},                      # an attempt at every check (latency-bound loops)
    {"polish_from": 50},
    {"scaling": 10, "polish_from": 150},      # OSQP's 10 Ruiz passes (the round-2 defaults)
])
def test_iteration_counts_match_cpu_restatement(cuda, schedule):
    """ADMM / polish iteration counts of the GPU against the C restatement (same algorithm),
    under each polish schedule; the solutions are the exact optimum in every case."""
    import cpu_solver
    from mpcqp import scenarios

    batch = scenarios.config3(512)
    params = base_params(20)
    out = solve(params, batch.x0, batch.ref, batch.u_prev, **schedule)
    ref = cpu_solver.cpu_solve(params, batch.x0, batch.ref, batch.u_prev, **schedule)
    assert (out["status"] == 1).all()
    same = (out["iters"] == ref["iters"]).all(axis=1)
    # bit-exact iteration indexing on the product path: the wavefront tree reductions round
    # differently from the C code's sequential sums, but no counter decision flips on these QPs
    # (profiles/r03_s16_iters_agreement.json: 100 % over 52,224 QPs of configs 2/3/4 and N = 1..63)
    assert same.all(), f"QPs {np.flatnonzero(~same)[:10]} disagree on iteration counts"
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["active"], ref["active"])
    assert rel(out["U"], ref["U"]) <= REL_TOL


def test_k1_model_matches_restatement(cuda):
    """K1 (unwrap + linearize) against the C restatement and numpy's unwrap."""
    import cpu_solver
    import torch
    from mpcqp import _lib, scenarios

    batch = scenarios.config3(256)
    # inject 2pi yaw jumps so np.unwrap has work to do
    ref = batch.ref.copy()
    ref[::3, 7:, 2] += 2 * np.pi
    ref[1::3, 12:, 2] -= 4 * np.pi
    params = base_params(20)
    # debug_state: K1 runs as its own kernel and leaves the model in the workspace (otherwise it
    # is fused into the solve and never leaves the CU)
    ctrl = controller(params, 256, debug_state=1)
    ctrl.solve_batch(batch.x0, ref, batch.u_prev)
    torch.cuda.synchronize()
    S = _lib.lib().mpcqp_model_stride(20)
    host = d2h(_lib.lib().mpcqp_model_buffer(ctrl._ws), np.zeros((256, S)))
    cpu = cpu_solver.cpu_solve(params, batch.x0, ref, batch.u_prev, want_model=True)["model"]
    N = 20
    yaw_gpu = host[:, 7 * N + 2: 11 * N + 4: 4]
    yaw_np = np.unwrap(ref[:, :, 2], axis=1)
    assert np.array_equal(yaw_gpu, yaw_np)
    assert rel(host[:, : 11 * N + 10], cpu[:, : 11 * N + 10]) <= 1e-12
    ctrl.close()


def test_k1_unwrap_golden_exact_pi(cuda, golden):
    """The reference-generated np.unwrap fixtures (unwrap.npz: exact +-pi jumps, whose sign rule
    is numpy's `ddmod == -pi and dd > 0`) through K1 on the GPU, bit for bit."""
    import torch
    from mpcqp import _lib

    g = golden("unwrap.npz")
    for case in range(len(g["lens"])):
        n = int(g["lens"][case])
        N = n - 1
        ref = np.zeros((2, n, 4))
        ref[:, :, 0] = np.arange(n)
        ref[:, :, 2] = g["p"][case, :n]
        ref[:, :, 3] = 10.0
        ctrl = controller(base_params(N), 2, debug_state=1)
        ctrl.solve_batch(np.zeros((2, 4)), ref, np.zeros((2, 2)))
        torch.cuda.synchronize()
        S = _lib.lib().mpcqp_model_stride(N)
        host = d2h(_lib.lib().mpcqp_model_buffer(ctrl._ws), np.zeros((2, S)))
        yaw = host[:, 7 * N + 2: 11 * N + 4: 4]
        assert np.array_equal(yaw[0], g["unwrapped"][case, :n]), case
        assert np.array_equal(yaw[1], g["unwrapped"][case, :n]), case
        ctrl.close()


def test_fused_k1_equals_separate_k1(cuda):
    """K1 fused into k_solve (the default: the model never leaves the CU) and K1 as its own kernel
    through the model buffer (debug_state) give the same bits for every output."""
    from mpcqp import scenarios

    batch = scenarios.config3(256)
    params = base_params(20)
    a = solve(params, batch.x0, batch.ref, batch.u_prev)
    b = solve(params, batch.x0, batch.ref, batch.u_prev, debug_state=1)
    for k in OUTS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("N", [3, 20])
def test_debug_scalars_of_the_solve_driver(cuda, N):
    """The debug scalars that k_solve's driver writes (debug_state): slot 4 = the wave's cycles,
    5 / 6 = the polish's factorizations from scratch / rank-1 updates, 7 = its start time.  A polish
    pass always begins with a factorization from scratch, and the debug state changes no output bit.
    For one-wave horizons only: from MPCQP_WIDE_MIN_HORIZON on the state slice has the wide layout."""
    from mpcqp import _lib, scenarios

    B = 8
    batch = scenarios.config3(B, horizon=N)
    params = base_params(N)
    plain = solve(params, batch.x0, batch.ref, batch.u_prev)
    ctrl = controller(params, B, debug_state=1)
    out = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev))
    L = _lib.lib()
    SS = L.mpcqp_state_stride(N)
    sc = SS - 8  # the eight scalars close a QP's slice
    if N == 20:
        assert sc == (4 * 20 * 20 + 7) // 8 * 8 + 15 * 64  # where tools/qp_cycles.py reads them
    st = d2h(L.mpcqp_state_buffer(ctrl._ws), np.zeros((B, SS)))
    ctrl.close()
    cycles, n_full, n_r1, start = (st[:, sc + k] for k in (4, 5, 6, 7))
    print(f"N={N}: cycles {cycles}, n_full {n_full}, n_r1 {n_r1}, start {start}, iters {out['iters'].tolist()}")
    for v in (cycles, start):
        assert np.isfinite(v).all() and (v > 0).all()
    for v in (n_full, n_r1):
        assert np.array_equal(v, np.round(v)) and (v >= 0).all()
    polished = out["iters"][:, 1] >= 1
    assert (n_full[polished] >= 1).all()
    for k in OUTS:
        assert np.array_equal(plain[k], out[k]), k


@pytest.mark.parametrize("N", [1, 2, 5, 10, 15, 31])
def test_horizons(cuda, N):
    from mpcqp import scenarios
    from mpcqp.control.ref_builder import build_reference

    plan = scenarios.load_default_plan()
    ref_g = build_reference(plan["path"], 15.0, N, 0.1)
    rng = np.random.default_rng(N)
    B = 64
    offs = rng.integers(0, len(ref_g), B)
    ref = np.stack([scenarios.window(ref_g, int(o), N) for o in offs])
    x0 = ref[:, 0] + rng.normal(0, 1, (B, 4)) * [2, 2, 0.3, 2]
    u_prev = rng.normal(0, 1, (B, 2)) * [3, 0.05]
    params = base_params(N)
    out = solve(params, x0, ref, u_prev)
    assert (out["status"] == 1).all()
    check_against_oracle(params, x0, ref, u_prev, out, range(0, B, 3))


def test_edge_cases(cuda):
    """Speeds outside [v_lo, v_hi] (constant v0 row active), saturated inputs, u_prev outside
    the rate band, u_prev omitted, and a heading window wrapping through +-pi."""
    import mpc_oracle as mo
    from mpcqp import scenarios

    N = 15
    params = base_params(N)
    batch = scenarios.config3(16, horizon=N)
    x0 = batch.x0.copy()
    ref = batch.ref.copy()
    x0[0, 3] = -3.0       # below v_lo
    x0[1, 3] = 120.0      # above v_hi
    ref[2, :, 3] = 200.0  # reference speed far above v_hi
    ref[3, :, 2] = np.linspace(3.0, 3.4, N + 1)
    ref[3, 5:, 2] -= 2 * np.pi  # wraps through pi
    up = batch.u_prev.copy()
    up[4] = [60.0, 1.0]   # outside the input box and the rate band
    out = solve(params, x0, ref, up)
    assert (out["status"] == 1).all()
    check_against_oracle(params, x0, ref, up, out, range(16))
    assert out["active"][0, 0] == 1 and out["active"][1, 0] == 2  # constant v0 row
    out2 = solve(params, x0, ref, None)
    assert (out2["status"] == 1).all()
    ex = mo.solve_exact(params, x0[5], ref[5], None)
    assert rel(out2["U"][5], ex.Umat) <= REL_TOL


def test_empty_batch_and_errors(cuda):
    import ctypes

    import torch
    from mpcqp import _lib

    params = base_params(10)
    ctrl = controller(params, 4)
    L = _lib.lib()
    st = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    x0 = torch.zeros((4, 4), dtype=torch.float64, device="cuda:0")
    ref = torch.zeros((4, 11, 4), dtype=torch.float64, device="cuda:0")
    assert L.mpcqp_build(ctrl._ws, 0, x0.data_ptr(), ref.data_ptr(), None, None) == 0
    assert L.mpcqp_solve(ctrl._ws, 0, None, None, None, st.data_ptr(), None, None, None) == 0
    assert L.mpcqp_build(ctrl._ws, 5, x0.data_ptr(), ref.data_ptr(), None, None) == -3  # > max_batch
    assert L.mpcqp_solve(ctrl._ws, 3, None, None, None, st.data_ptr(), None, None, None) == -5  # B != built
    bad = _lib.to_c_params(params)
    bad.horizon = 1025  # past MPCQP_MAX_HORIZON
    ws = ctypes.c_void_p()
    assert L.mpcqp_create(ctypes.byref(bad), 4, 0, ctypes.byref(ws)) == -2
    assert b"horizon" in L.mpcqp_last_error()
    # new parameters invalidate the last build: solving it would mix two parameter blocks
    assert L.mpcqp_build(ctrl._ws, 2, x0.data_ptr(), ref.data_ptr(), None, None) == 0
    assert L.mpcqp_set_params(ctrl._ws, ctypes.byref(_lib.to_c_params(params))) == 0
    assert L.mpcqp_solve(ctrl._ws, 2, None, None, None, st.data_ptr(), None, None, None) == -5
    assert L.mpcqp_build(ctrl._ws, 2, x0.data_ptr(), ref.data_ptr(), None, None) == 0
    assert L.mpcqp_solve(ctrl._ws, 2, None, None, None, st.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    ctrl.close()


def test_full_size_config3_properties(cuda):
    """BASELINE config 3 at its full size (B=4096, N=20): every QP solved, deterministic, and
    a strided sample matches the exact oracle."""
    from mpcqp import scenarios

    batch = scenarios.config3(4096)
    params = base_params(20)
    a = solve(params, batch.x0, batch.ref, batch.u_prev)
    b = solve(params, batch.x0, batch.ref, batch.u_prev)
    assert (a["status"] == 1).all()
    for k in ("U", "X", "active", "iters"):
        assert np.array_equal(a[k], b[k]), f"non-deterministic {k}"
    check_against_oracle(params, batch.x0, batch.ref, batch.u_prev, a, range(0, 4096, 97))


def test_full_size_config4_properties(cuda):
    """Config 4 at full size (B=16384, N=30): solved, first-order optimality (oracle gradient)
    on a sample, v rows consistent with X."""
    import mpc_oracle as mo
    from mpcqp import scenarios

    batch = scenarios.config4(16384)
    params = base_params(30)
    out = solve(params, batch.x0, batch.ref, batch.u_prev)
    assert (out["status"] == 1).all()
    for b in range(0, 16384, 331):
        qp = mo.condense(params, batch.x0[b], batch.ref[b], batch.u_prev[b])
        U = out["U"][b].T.reshape(-1)
        g = mo.gradient(qp, U)
        assert np.abs(g).max() <= 1e-6 * max(1.0, np.abs(qp.g).max()), f"QP {b}: gradient {np.abs(g).max():.2e}"
        v = out["X"][b, 3]
        lo, hi = params.v_bounds
        codes = np.where(v > hi, 2, np.where(v < lo, 1, 0))
        assert np.array_equal(codes, out["active"][b, :31])


def test_wave_primitives(cuda):
    """The DPP wavefront scans / reductions / shifts used by every kernel."""
    import torch
    from mpcqp import _lib

    rng = np.random.default_rng(3)
    v = rng.normal(size=64)
    x = torch.from_numpy(v).to(cuda)
    out = torch.zeros(10 * 64, dtype=torch.float64, device=cuda)
    assert _lib.lib().mpcqp_debug_wave_ops(x.data_ptr(), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(10, 64)
    a = np.abs(v)
    np.testing.assert_allclose(o[0], np.cumsum(v), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(o[1], np.cumsum(v[::-1])[::-1], rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(o[2], np.maximum.accumulate(a))
    np.testing.assert_array_equal(o[3], np.maximum.accumulate(a[::-1])[::-1])
    np.testing.assert_allclose(o[4], np.full(64, v.sum()), rtol=1e-13)
    np.testing.assert_array_equal(o[5], np.full(64, a.max()))
    np.testing.assert_array_equal(o[6], np.concatenate([[0, 0], v[:-2]]))
    np.testing.assert_array_equal(o[7], np.concatenate([v[2:], [0, 0]]))
    np.testing.assert_array_equal(o[8], np.concatenate([[0], v[:-1]]))
    np.testing.assert_array_equal(o[9], np.full(64, v[37]))


@pytest.mark.parametrize("N", [5, 20, 30])
def test_setup_state_matches_restatement(cuda, N):
    """K2a (condensing + Ruiz scaling) against the C restatement, field by field."""
    import cpu_solver
    import torch
    from mpcqp import _lib, scenarios

    batch = scenarios.config3(64, horizon=N)
    params = base_params(N)
    ctrl = controller(params, 64, debug_state=1)  # write the state buffer
    ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev)
    torch.cuda.synchronize()
    L = _lib.lib()
    SS, MS = L.mpcqp_state_stride(N), L.mpcqp_model_stride(N)
    st = d2h(L.mpcqp_state_buffer(ctrl._ws), np.zeros((64, SS)))
    model = d2h(L.mpcqp_model_buffer(ctrl._ws), np.zeros((64, MS)))
    ref = cpu_solver.cpu_state(params, model, SS)
    n = 2 * N
    lane_off = (4 * N * N + 7) // 8 * 8
    P_gpu, P_cpu = st[:, : n * n], ref[:, : n * n]
    assert rel(P_gpu, P_cpu) <= 1e-12
    for f, name in enumerate(["q", "D", "x", "E0", "E1", "E2", "lo0", "lo1", "lo2", "hi0", "hi1", "hi2",
                              "w0", "w1", "w2"]):
        if name == "x":
            continue
        g = st[:, lane_off + 64 * f: lane_off + 64 * (f + 1)]
        c = ref[:, lane_off + 64 * f: lane_off + 64 * (f + 1)]
        assert rel(g, c) <= 1e-12, name
    assert rel(st[:, lane_off + 15 * 64], ref[:, lane_off + 15 * 64]) <= 1e-12
    ctrl.close()


def test_admm_iterate_matches_restatement(cuda):
    """K2b alone (polish off): the ADMM iterate and its iteration counts against the C code."""
    import cpu_solver
    from mpcqp import scenarios

    batch = scenarios.config3(256)
    params = base_params(20)
    out = solve(params, batch.x0, batch.ref, batch.u_prev, polish=0)
    ref = cpu_solver.cpu_solve(params, batch.x0, batch.ref, batch.u_prev, polish=0)
    same = out["iters"][:, 0] == ref["iters"][:, 0]
    assert same.mean() >= 0.95, same.mean()
    # the ADMM iterate is only eps_abs = eps_rel = 1e-3 accurate by construction and ~100
    # iterations amplify the rounding differences of tree vs sequential sums to ~1e-6
    assert rel(out["U"][same], ref["U"][same]) <= 1e-4
