"""The polish's rank-1 path (Ctx::rank1, the line search, the pass control) against the C restatement.

Per horizon one batch that spends most of its polish passes beyond the first one, where the inverse
is updated by rank-1 changes instead of factorized again:

  * N = 3, 8, 9: the first block boundary of the inverse-column selection at small n;
  * N = 8 / 16: the register broadcasts with no lane move (n = 16) and one permlane16 stage (n = 32);
  * N = 17: the first horizon whose rank-1 update goes through LDS (n = 34 > 32);
  * N = 20: the headline horizon; N = 23 / 24: the last full and the first packed Pbar;
  * N = 32: n = 64, no padding lane;
  * N = 2 (perturbed inputs: config 3 almost never polishes twice there).

Asserted per horizon, with debug_state=1: status, active set and all four counters (ADMM iterations,
polish passes, factorizations, line-search trials) equal the C restatement's on every QP, U within
test_gpu_parity.py's 1e-8 relative of it, and the batch really is on the rank-1 path (share of QPs
with two or more passes, summed rank-1 counter).
"""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import REL_TOL, base_params, controller, d2h, rel, take

pytestmark = pytest.mark.gpu

B = 256


def _solve_debug(N, x0, ref, u_prev):
    """(outputs, summed rank-1 counter) of one debug_state solve; the C restatement of the same batch."""
    import cpu_solver
    from mpcqp import _lib

    params = base_params(N)
    n = len(x0)
    ctrl = controller(params, n, debug_state=1)
    out = take(ctrl.solve_batch(x0, ref, u_prev))
    L = _lib.lib()
    SS = L.mpcqp_state_stride(N)
    st = d2h(L.mpcqp_state_buffer(ctrl._ws), np.zeros((n, SS)))
    ctrl.close()
    n_r1 = st[:, SS - 8 + 6]  # debug scalar 6: the polish's rank-1 updates
    assert np.array_equal(n_r1, np.round(n_r1)) and (n_r1 >= 0).all()
    cpu = cpu_solver.cpu_solve(params, x0, ref, u_prev)
    return out, float(n_r1.sum()), cpu


def _assert_same_as_restatement(out, cpu):
    same = (out["iters"] == cpu["iters"]).all(axis=1)
    assert same.all(), f"QPs {np.flatnonzero(~same)[:10]} disagree on the counters"
    assert np.array_equal(out["status"], cpu["status"])
    assert np.array_equal(out["active"], cpu["active"])
    assert rel(out["U"], cpu["U"]) <= REL_TOL


@pytest.mark.parametrize("N", [3, 8, 9, 16, 17, 20, 23, 24, 32])
def test_rank1_path_matches_restatement(cuda, N):
    from mpcqp import scenarios

    batch = scenarios.config3(B, horizon=N)
    out, n_r1, cpu = _solve_debug(N, batch.x0, batch.ref, batch.u_prev)
    twice = float((out["iters"][:, 1] >= 2).mean())
    print(f"N={N}: {twice:.0%} of the QPs with two or more passes, "
          f"{int(np.maximum(out['iters'][:, 1] - 1, 0).sum())} passes beyond the first, {int(n_r1)} rank-1 updates")
    _assert_same_as_restatement(out, cpu)
    assert twice >= 0.40
    assert n_r1 >= 100


def test_rank1_path_at_two_steps(cuda):
    """N = 2 (n = 4: one leaf pair per half of the selection, every index clamp in play).  The inputs
    of test_horizons with three times its perturbation: the C restatement takes two or more passes on
    49 of the 256 QPs (config 3: 1 %)."""
    from mpcqp import scenarios
    from mpcqp.control.ref_builder import build_reference

    N = 2
    plan = scenarios.load_default_plan()
    ref_g = build_reference(plan["path"], 15.0, N, 0.1)
    rng = np.random.default_rng(N)
    offs = rng.integers(0, len(ref_g), B)
    ref = np.stack([scenarios.window(ref_g, int(o), N) for o in offs])
    x0 = ref[:, 0] + rng.normal(0, 1, (B, 4)) * [6, 6, 0.9, 6]
    u_prev = rng.normal(0, 1, (B, 2)) * [9, 0.15]
    out, n_r1, cpu = _solve_debug(N, x0, ref, u_prev)
    twice = int((out["iters"][:, 1] >= 2).sum())
    print(f"N=2: {twice} QPs with two or more passes, {int(n_r1)} rank-1 updates")
    assert int((cpu["iters"][:, 1] >= 2).sum()) >= 8
    _assert_same_as_restatement(out, cpu)
    assert twice >= 8
    # a pass beyond the first updates by rank 1 unless more than n / 2 = 2 soft rows changed
    assert n_r1 >= 1
