"""The ADMM termination check (admm_run: residual norms, the four-at-once wave maxima, the scalings'
reciprocals kept from setup, the adaptive-rho decision) on the product path against the C restatement.

One batch per case, scenarios.config3(256, horizon=N), no debug_state, with two QPs per wave on and
off where the horizon allows it (N <= 15):

  * default settings at N = 2, 8, 9, 16, 17, 20, 24, 32: no broadcast, one permlane stage, LDS, packed
    Pbar, no padding lane;
  * rho = 1.0 and rho = 0.005 at N = 9 and 20: the check's adaptive-rho decision asks for another ADMM
    factorization on most QPs (asserted on the restatement first);
  * max_iter = 40: the last check falls at an iteration that is no multiple of check_termination, and
    ends as solved_inaccurate on 20 or more QPs of the restatement;
  * polish off, with max_iter = 60 (the checks at 25, 50 and 60) and alone (up to seven checks per QP at
    N = 20, convergence by the test itself); the restatement's check counts are asserted first.

Polished results: status, active set and all four counters equal the restatement's on every QP, U within
test_gpu_parity.py's 1e-8 relative of it.  Unpolished results (max_iter = 40, polish off) follow
test_gpu_params.py::test_max_iter_status_follows_osqp: the statuses agree on 99 % of the QPs (unpolished
iterates round differently in the wave reductions), and the counters are equal wherever they do.
"""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import REL_TOL, base_params, rel, solve

pytestmark = pytest.mark.gpu

# an unpolished ADMM iterate against the restatement's (tests/test_gpu_parity.py: the iterate is only
# eps = 1e-3 accurate and ~100 iterations amplify the rounding of tree vs sequential sums to ~1e-6)
REL_TOL_UNPOLISHED = 1e-4
B = 256
PAIR_MAX = 15  # two QPs per wave up to this horizon

_cache: dict = {}


def _pairings(N):
    return ("on", "off") if N <= PAIR_MAX else ("auto",)


def _restatement(N, **settings):
    """The batch and the C restatement's result for it, computed once per (N, settings)."""
    import cpu_solver
    from mpcqp import scenarios

    key = (N, tuple(sorted(settings.items())))
    if key not in _cache:
        batch = scenarios.config3(B, horizon=N)
        params = base_params(N)
        cpu = cpu_solver.cpu_solve(params, batch.x0, batch.ref, batch.u_prev, **settings)
        for v in cpu.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = (batch, params, cpu)
    return _cache[key]


def _assert_same(out, cpu, what):
    same = (out["iters"] == cpu["iters"]).all(axis=1)
    print(f"{what}: counters equal on {int(same.sum())} of {len(same)} QPs, "
          f"status equal on {int((out['status'] == cpu['status']).sum())}, rel U {rel(out['U'], cpu['U']):.2e}")
    assert same.all(), f"{what}: QPs {np.flatnonzero(~same)[:10]} disagree on the counters"
    assert np.array_equal(out["status"], cpu["status"]), what
    assert np.array_equal(out["active"], cpu["active"]), what
    assert rel(out["U"], cpu["U"]) <= REL_TOL, what


def _assert_unpolished_rule(out, cpu, what, polished_exact):
    agree = out["status"] == cpu["status"]
    same = (out["iters"] == cpu["iters"]).all(axis=1)
    print(f"{what}: status equal on {agree.mean():.4f} of the QPs, counters equal on {int(same.sum())} of {len(same)}, "
          f"on {int(same[agree].sum())} of the {int(agree.sum())} with equal status")
    assert agree.mean() >= 0.99, (what, float(agree.mean()))
    assert same[agree].all(), f"{what}: QPs {np.flatnonzero(agree & ~same)[:10]} disagree on the counters"
    if polished_exact:  # solved = converged and polished: the exact optimum
        sel = agree & (cpu["status"] == 1)
        assert np.array_equal(out["active"][sel], cpu["active"][sel]), what
        assert rel(out["U"][sel], cpu["U"][sel]) <= REL_TOL, what
    assert rel(out["U"][agree], cpu["U"][agree]) <= REL_TOL_UNPOLISHED, what


@pytest.mark.parametrize("N", [2, 8, 9, 16, 17, 20, 24, 32])
def test_check_default_settings(cuda, N):
    batch, params, cpu = _restatement(N)
    assert (cpu["status"] == 1).all()
    for pairing in _pairings(N):
        _assert_same(solve(params, batch, pairing=pairing), cpu, f"N={N} pairing={pairing}")


@pytest.mark.parametrize("N", [9, 20])
@pytest.mark.parametrize("rho,share", [(1.0, 0.75), (0.005, 0.60)])
def test_check_adaptive_rho_refactorizes(cuda, N, rho, share):
    """The check's adaptive-rho decision changes rho: ADMM factorizes again (factorizations - polish
    passes >= 2) on most QPs of the restatement, and the kernel takes every one of those decisions alike."""
    batch, params, cpu = _restatement(N, rho=rho)
    refac = float((cpu["iters"][:, 2] - cpu["iters"][:, 1] >= 2).mean())
    print(f"N={N} rho={rho}: {refac:.0%} of the restatement's QPs factorize twice or more in ADMM")
    assert refac >= share
    for pairing in _pairings(N):
        _assert_same(solve(params, batch, pairing=pairing, rho=rho), cpu, f"N={N} rho={rho} pairing={pairing}")


@pytest.mark.parametrize("N", [9, 20])
def test_check_at_max_iter_off_the_grid(cuda, N):
    """max_iter = 40: the final check runs at iteration 40, between two multiples of check_termination."""
    batch, params, cpu = _restatement(N, max_iter=40)
    st, cnt = np.unique(cpu["status"], return_counts=True)
    print(f"N={N} max_iter=40: restatement statuses {dict(zip(st.tolist(), cnt.tolist()))}")
    assert int((cpu["status"] == 2).sum()) >= 20
    for pairing in _pairings(N):
        _assert_unpolished_rule(solve(params, batch, pairing=pairing, max_iter=40), cpu,
                                f"N={N} max_iter=40 pairing={pairing}", polished_exact=True)


@pytest.mark.parametrize("N", [9, 20])
@pytest.mark.parametrize("settings", [dict(polish=0, max_iter=60), dict(polish=0)], ids=["max_iter60", "to_convergence"])
def test_check_without_polish(cuda, N, settings):
    """Polish off: the termination test alone ends the solve (or max_iter = 60 does, after two checks)."""
    batch, params, cpu = _restatement(N, **settings)
    # checks of a QP: one per 25 iterations, and the one at max_iter when that is off the grid
    checks = (cpu["iters"][:, 0] + 24) // 25
    print(f"N={N} {settings}: restatement checks per QP {np.bincount(checks).tolist()} (index = checks)")
    if "max_iter" in settings:  # 60 iterations: the checks at 25, 50 and 60 (36 QPs at N = 9, 11 at N = 20)
        assert int(checks.max()) == 3 and int((checks == 3).sum()) >= 8
    else:  # convergence by the test itself, several checks into the solve
        assert (cpu["status"] == 1).all()
        assert int(checks.max()) >= 4 and int((checks >= 2).sum()) >= 64
    for pairing in _pairings(N):
        _assert_unpolished_rule(solve(params, batch, pairing=pairing, **settings), cpu,
                                f"N={N} {settings} pairing={pairing}", polished_exact=False)
