"""Newton from a caller's guess on a condensed QP: the host model of the warm start's attempt.

``newton_from`` is ``mpc_oracle.solve_condensed`` started at a given ``U`` instead of the unconstrained
minimiser: the first active set classifies the guess's rows, each pass solves the exact quadratic
model of the current set, and the point is the optimum once the set reproduces itself.  Its steps are
Armijo steps where the kernel searches the line exactly, so pass counts beyond 1 may differ from the
kernel's; a 1-pass convergence depends on the guess's active set alone and is the same in both.

The margin of an optimum is the smallest distance of any soft row to one of its bounds: where it is
large against rounding, the kernel and this model classify every row the same way.
"""
from __future__ import annotations

from dataclasses import dataclass

import mpc_oracle as mo
import numpy as np

MARGIN = 1e-6  # an optimum's rows are "clear of their bounds" past this distance


@dataclass
class NewtonResult:
    U: np.ndarray  # (2N,) in the oracle's order (a_0, delta_0, a_1, ...)
    Umat: np.ndarray  # (2, N)
    codes: np.ndarray  # (5N+1,) active codes at U
    passes: int
    converged: bool
    margin: float  # min over rows of the distance to the nearer bound, at U


def margin(qp: mo.CondensedQP, U) -> float:
    z = qp.C @ np.asarray(U, dtype=float) + qp.b
    return float(np.minimum(np.abs(z - qp.lo), np.abs(z - qp.hi)).min())


def newton_from(qp: mo.CondensedQP, Umat, max_iter: int = 200) -> NewtonResult:
    """Semismooth Newton on ``qp`` from the guess ``Umat`` (2, N)."""
    N = qp.H.shape[0] // mo.NU
    U = np.asarray(Umat, dtype=float).reshape(mo.NU, N).T.reshape(-1).copy()
    codes = mo.active_codes(qp.C @ U + qp.b, qp.lo, qp.hi)
    ok, it = False, 0
    for it in range(1, max_iter + 1):
        act = codes != mo.ACT_NONE
        bnd = np.where(codes == mo.ACT_UPPER, qp.hi, qp.lo)
        Ca, wa = qp.C[act], qp.w[act]
        M = qp.H + Ca.T @ (wa[:, None] * Ca)
        rhs = -(qp.g + Ca.T @ (wa * (qp.b[act] - bnd[act])))
        U_new = np.linalg.solve(M, rhs)
        codes_new = mo.active_codes(qp.C @ U_new + qp.b, qp.lo, qp.hi)
        if np.array_equal(codes_new, codes):
            U, ok = U_new, True
            break
        d = U_new - U
        f0 = mo.objective(qp, U)
        slope = 2.0 * float(mo.gradient(qp, U) @ d)
        t = 1.0
        while t > 1e-12 and mo.objective(qp, U + t * d) > f0 + 1e-4 * t * slope:
            t *= 0.5
        U = U + t * d
        codes = mo.active_codes(qp.C @ U + qp.b, qp.lo, qp.hi)
    return NewtonResult(U, U.reshape(N, mo.NU).T.copy(), codes, it, ok, margin(qp, U))


def shifted(Umat) -> np.ndarray:
    """The guess a closed loop carries to its next step: every input one step on, the last repeated."""
    Umat = np.asarray(Umat, dtype=float)
    return np.concatenate([Umat[:, 1:], Umat[:, -1:]], axis=1)


_WINDOWS = {}


def golden_windows(loop, params, N):
    """The windows of the reference's closed loop at horizon N (``closed_loop.npz``) with what the
    warm-start tests share, computed once per session: each window's exact optimum and its margin, and
    from the second window on the Newton run from the previous optimum shifted one step."""
    if N in _WINDOWS:
        return _WINDOWS[N]
    x0, win, up = loop[f"N{N}_x0"], loop[f"N{N}_window"], loop[f"N{N}_u_prev"]
    qps = [mo.condense(params, x0[k], win[k], up[k]) for k in range(len(x0))]
    exact = [mo.solve_exact(params, x0[k], win[k], up[k]) for k in range(len(x0))]
    margins = np.array([margin(q, e.U) for q, e in zip(qps, exact)])
    guesses = np.stack([exact[0].Umat] + [shifted(exact[k - 1].Umat) for k in range(1, len(x0))])
    runs = [None] + [newton_from(qps[k], guesses[k]) for k in range(1, len(x0))]
    _WINDOWS[N] = dict(x0=x0, window=win, u_prev=up, qps=qps, exact=exact, margins=margins, guesses=guesses,
                       shifted_runs=runs)
    return _WINDOWS[N]
