"""The sweep's pivot step (Ctx::sweep, Ctx::sweep_reg: the pivot lane's coefficient and new r[k] written
under a one-lane exec mask, the pivot test decided once after the last step) through what is most
sensitive to the KKT inverse it leaves, against the C restatement.

Inputs: scenarios.CONFIGS["config3"], 64 QPs per horizon.

  * the LDS-column sweep at N = 17 (its first horizon), 20 and 23 (the middle and the last unpacked
    Pbar), 24 (the first packed Pbar) and 31 (the register limit);
  * the register-broadcast sweep on the whole wave at N = 10 and 16, and in the half-wave layout at
    N = 9 and 15 with pairing forced on, whose outputs must also equal the unpaired kernel's bit for bit;
  * an unpolished iterate (polish = 0, max_iter = 40) at N = 20 and at N = 15 paired: every ADMM step
    multiplies by the inverse, so one wrong coefficient on one lane shows in U;
  * one QP of 8 with NaN in x0, or with inf in its reference, at N = 20 and at N = 15 paired with a healthy
    partner: MPCQP_NUMERICAL_ERROR on that QP, the restatement's results on the others.

Statuses, all four counters and active sets equal the restatement's; U within 1e-8 relative of it.
"""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import OUTS, REL_TOL, assert_same, base_params, rel, solve

pytestmark = pytest.mark.gpu

B = 64
UNPOLISHED = dict(polish=0, max_iter=40)

_cache: dict = {}


def _restatement(N, batch_size=B, **settings):
    """The config-3 batch at horizon N and the C restatement's result for it, computed once."""
    import cpu_solver
    from mpcqp import scenarios

    key = (N, batch_size, tuple(sorted(settings.items())))
    if key not in _cache:
        batch = scenarios.CONFIGS["config3"](batch_size, horizon=N)
        params = base_params(N)
        cpu = cpu_solver.cpu_solve(params, batch.x0, batch.ref, batch.u_prev, **settings)
        for v in cpu.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = (batch, params, cpu)
    return _cache[key]


def _assert_restatement(out, cpu, what, idx=slice(None)):
    e = rel(out["U"][idx], cpu["U"][idx])
    print(f"{what}: rel U {e:.3e}, statuses {np.unique(out['status'][idx]).tolist()}, "
          f"counters equal on {int((out['iters'][idx] == cpu['iters'][idx]).all(axis=1).sum())} QPs")
    assert np.array_equal(out["status"][idx], cpu["status"][idx]), what
    assert np.array_equal(out["iters"][idx], cpu["iters"][idx]), what
    assert np.array_equal(out["active"][idx], cpu["active"][idx]), what
    assert e <= REL_TOL, f"{what}: rel U {e:.3e}"


@pytest.mark.parametrize("N", [17, 20, 23, 24, 31])
def test_lds_column_sweep(cuda, N):
    batch, params, cpu = _restatement(N)
    assert (cpu["status"] == 1).all()
    _assert_restatement(solve(params, batch), cpu, f"N={N}")


@pytest.mark.parametrize("N", [10, 16])
def test_register_sweep_whole_wave(cuda, N):
    batch, params, cpu = _restatement(N)
    assert (cpu["status"] == 1).all()
    _assert_restatement(solve(params, batch, pairing="off"), cpu, f"N={N} unpaired")


@pytest.mark.parametrize("N", [9, 15])
def test_register_sweep_half_wave(cuda, N):
    batch, params, cpu = _restatement(N)
    assert (cpu["status"] == 1).all()
    two = solve(params, batch, pairing="on")
    _assert_restatement(two, cpu, f"N={N} paired")
    assert_same(two, solve(params, batch, pairing="off"), f"N={N} paired against unpaired", OUTS)


@pytest.mark.parametrize("N,pairing", [(20, "auto"), (15, "on")])
def test_unpolished_iterate(cuda, N, pairing):
    """U of an unpolished ADMM iterate (polish = 0, max_iter = 40) within 1e-8 of the restatement's
    under the same settings."""
    batch, params, cpu = _restatement(N, **UNPOLISHED)
    out = solve(params, batch, pairing=pairing, **UNPOLISHED)
    e = rel(out["U"], cpu["U"])
    print(f"N={N} pairing={pairing} unpolished: rel U {e:.3e}")
    assert e <= REL_TOL, f"N={N} pairing={pairing}: rel U {e:.3e}"


@pytest.mark.parametrize("N,pairing", [(20, "auto"), (15, "on")])
@pytest.mark.parametrize("bad_input", ["nan_x0", "inf_ref"])
def test_non_finite_qp_among_healthy_ones(cuda, N, pairing, bad_input):
    """QP 2 of 8 has non-finite data (in the pair layout QP 3 shares its wave): numerical error there,
    the restatement's results for the seven others."""
    from mpcqp import _lib

    batch, params, cpu = _restatement(N, 8)
    x0, ref = batch.x0.copy(), batch.ref.copy()
    if bad_input == "nan_x0":
        x0[2, 0] = np.nan
    else:
        ref[2, N // 2, 1] = np.inf
    out = solve(params, x0, ref, batch.u_prev, pairing=pairing)
    assert out["status"][2] == _lib.NUMERICAL_ERROR
    _assert_restatement(out, cpu, f"N={N} pairing={pairing} {bad_input}", np.arange(8) != 2)
