"""The MPCParameters variants and the edge inputs on the mid (N = 33..64) and wide (N > 64, and every N
under ``reproducible = 1``) kernels, against references that share no code with them.

Each solve path condenses the QP with its own code: its own symmetrisation of Q / Q_N / R, its own
bound, weight and active-code tables, and (one-wave and mid) its own "the weights are diagonal" branch.
``test_gpu_params.py`` holds the one-wave kernel to the exact oracle under the nine variants of
``param_variants.py``; this file does the same for the other two:

  1. every variant at N = 33 (bucket 40, seven padding steps), 40 (a full two-part bucket), 49 (bucket
     56, four parts), 64 (full rows, the second gradient-column pass, state row 64 from lane 63), 65 (the
     first wide horizon, K1 in two chunks) and 72 (2N = 144, past the in-LDS sweep) against
     ``mpc_oracle.solve_exact``: U / X / u0 to 1e-8 relative, identical active sets;
  2. ``reproducible = 1`` (the wide kernel at every horizon) under every variant at N = 20, 40, 72 against
     the C restatement fed the GPU's own model: statuses, counters, U, X and active sets bit for bit;
  3. the mid cases of (1) against the C restatement: statuses and active sets equal, U to 1e-8.  The
     four counters are NOT asserted here: how many QPs agree on all four is recorded per variant and
     horizon (``profiles/params_long/iters_agreement.json`` is that record from one run; set
     ``MPCQP_ITERS_AGREEMENT_JSON=<path>`` to write it again);
  4. edge inputs at N = 33, 40, 49, 64, 65 under the default block, ``tight_bounds`` and ``q_nondiag``,
     with and without ``u_prev``: start speeds outside [v_lo, v_hi], reference speeds far outside it over
     the whole window and over its last three steps only (the last speed row), ``u_prev`` outside the
     input box on either side, a heading step over the last four steps (the last input and rate rows) and
     a heading window wrapping through pi.  That the batch reaches those rows is asserted on the ORACLE's
     active sets, so a kernel that never reports them cannot satisfy it;
  5. ``mpcqp_solve`` with outputs left NULL (all but ``status`` may be, include/mpcqp.h) at N = 40 and 65.

1e-8 is the project's tolerance against the exact oracle; on these inputs the two CPU references
(the oracle and the C restatement) agree to 1.1e-9 relative in U and X at worst (``slack_x10``, N = 33)
and to 1.7e-10 on the edge batches, with identical active sets: 1e-8 leaves about 9x over the references'
own spread.
"""
from __future__ import annotations

import json
import os
from functools import lru_cache

import numpy as np
import pytest
from gpu_helpers import REL_TOL, assert_exact, controller, rel, solve, solve_with_model, variant_params
from param_variants import VARIANTS

pytestmark = pytest.mark.gpu

MID_N = (33, 40, 49, 64)
FAST_N = MID_N + (65, 72)
EDGE_N = (33, 40, 49, 64, 65)
EDGE_BLOCKS = ("default", "tight_bounds", "q_nondiag")


def _exact_active_sets(params, x0, ref, u_prev, out, what):
    """Every QP of ``out`` solved and equal to solve_exact under ``params`` (gpu_helpers.assert_exact); returns
    the oracle's active sets (B, 5N+1)."""
    import mpc_oracle as mo

    acts = []
    for b in range(len(x0)):
        ex = mo.solve_exact(params, x0[b], ref[b], None if u_prev is None else u_prev[b])
        assert ex.converged, f"{what} QP {b}: the oracle did not converge"
        assert_exact(out, b, ex, what, solved=True)
        acts.append(ex.active)
    return np.stack(acts)


@lru_cache(maxsize=None)
def _fast_case(name, N):
    """The 12-QP batch of part 1 under variant ``name``, solved once in fast mode: (params, batch, out, model)."""
    from mpcqp import scenarios

    params = variant_params(name, N)
    batch = scenarios.config3(12, horizon=N, seed=6000 + N)
    out, model = solve_with_model(params, batch.x0, batch.ref, batch.u_prev)
    assert model is not None  # the mid and wide kernels read the model K1 wrote
    for a in (*out.values(), model):
        a.setflags(write=False)  # shared by parts 1 and 3
    return params, batch, out, model


# ---------------------------------------------------------------------- 1. exact oracle, fast mode
@pytest.mark.parametrize("N", FAST_N)
@pytest.mark.parametrize("name", VARIANTS)
def test_variants_match_exact_oracle_on_mid_and_wide(cuda, name, N):
    params, batch, out, _ = _fast_case(name, N)
    acts = _exact_active_sets(params, batch.x0, batch.ref, batch.u_prev, out, f"{name} N={N}")
    assert (acts != 0).any()  # the variant's soft rows are exercised


# ---------------------------------------------------------------------- 2. reproducible mode, bit for bit
@pytest.mark.parametrize("N", [20, 40, 72])
@pytest.mark.parametrize("name", VARIANTS)
def test_variants_reproducible_mode_bit_exact_with_c_restatement(cuda, name, N):
    """The mode's guarantee (same model in -> same bits out as oracle/mpcqp_cpu.c) under every variant."""
    import cpu_solver
    from mpcqp import scenarios

    params = variant_params(name, N)
    batch = scenarios.config3(12, horizon=N, seed=6100 + N)
    out, model = solve_with_model(params, batch.x0, batch.ref, batch.u_prev, reproducible=1)
    assert model is not None
    ref = cpu_solver.cpu_solve_models(params, model)
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["iters"], ref["iters"]), np.argwhere((out["iters"] != ref["iters"]).any(axis=1))
    assert np.array_equal(out["U"], ref["U"])
    assert np.array_equal(out["X"], ref["X"])
    assert np.array_equal(out["active"], ref["active"])
    assert (out["status"] == 1).any(), out["status"]  # solves, not a batch of early exits


# ---------------------------------------------------------------------- 3. fast mode vs the C restatement
_AGREEMENT: dict = {}


def _write_agreement():
    path = os.environ.get("MPCQP_ITERS_AGREEMENT_JSON")
    if not path or not _AGREEMENT:
        return
    rec = {"what": "mid kernel (fast mode) vs the C restatement on the GPU's model, config3(12, horizon=N, "
                   "seed=6000+N) under each MPCParameters variant: QPs (of 12) whose four counters (ADMM "
                   "iterations, polish passes, factorizations, line-search trials) all agree",
           "qps_per_case": 12,
           "all_four_counters_agree": {name: {f"N{N}": _AGREEMENT[name, N] for N in MID_N if (name, N) in _AGREEMENT}
                                       for name in VARIANTS if any(k[0] == name for k in _AGREEMENT)}}
    cases = list(_AGREEMENT.values())
    rec["total"] = {"qps": 12 * len(cases), "agree": int(sum(cases))}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


@pytest.fixture(scope="module", autouse=True)
def _agreement_record():
    yield
    _write_agreement()


@pytest.mark.parametrize("N", MID_N)
@pytest.mark.parametrize("name", VARIANTS)
def test_variants_mid_kernel_against_c_restatement(cuda, name, N):
    """Same statuses and active sets as the C restatement on the GPU's own model, U to 1e-8.  The counters'
    agreement is an observation for the variants (the mid kernel sums in tree order), so it is recorded,
    not asserted."""
    import cpu_solver

    params, _, out, model = _fast_case(name, N)
    assert model is not None
    ref = cpu_solver.cpu_solve_models(params, model)
    same = int((out["iters"] == ref["iters"]).all(axis=1).sum())
    _AGREEMENT[name, N] = same
    print(f"{name} N={N}: {same} of {len(model)} QPs agree on all four counters; "
          f"rel U {rel(out['U'], ref['U']):.3e}")
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["active"], ref["active"])
    assert rel(out["U"], ref["U"]) <= REL_TOL


# ---------------------------------------------------------------------- 4. edge inputs
def _edge_batch(N):
    from mpcqp import scenarios

    batch = scenarios.config3(16, horizon=N, seed=7000 + N)
    x0, ref, up = batch.x0.copy(), batch.ref.copy(), batch.u_prev.copy()
    x0[0, 3] = -3.0  # below v_lo: the constant v0 row, lower side
    x0[1, 3] = 120.0  # above v_hi: upper side
    ref[2, :, 3] = 200.0  # reference speed far above v_hi
    ref[3, :, 2] = np.linspace(3.0, 3.4, N + 1)
    ref[3, N // 2:, 2] -= 2 * np.pi  # wraps through pi
    up[4] = [60.0, 1.0]  # outside the input box and the rate band, above
    ref[5, :, 3] = -50.0  # reference speed far below v_lo
    ref[6, N - 3:, 3] = 200.0  # the last speed rows, and the last acceleration / rate rows
    ref[7, N - 3:, 3] = -50.0
    up[8] = [-60.0, -1.0]  # ... below
    ref[9, N - 4:, 2] += 1.2  # a heading step at the end: the last steering / rate rows
    ref[10, N - 4:, 2] -= 1.2
    # the last acceleration-rate row: rows 6 / 7 end with the acceleration saturated (a flat 35, rate 0), so
    # a speed reference that reverses at the end: Q pulls v_{N-1} one way with weight 0.1, Q_N pulls v_N the
    # other way with 0.2 and half the distance, which about cancels on a_{N-2} and leaves a_{N-1} alone
    # to jump past the rate band (upper side in row 11, lower in row 12)
    ref[11, N - 1, 3], ref[11, N, 3] = -600.0, 300.0
    ref[12, N - 1, 3], ref[12, N, 3] = 600.0, -300.0
    # the last steering row: after the single step of rows 9 / 10 the steering comes back down the rate band
    # (0.607, 0.456 at the last two steps), and delta_{N-1} moves only psi_N, weakly at the low speed the
    # windows end with; a staircase (+3, +6, +9 rad over the last three rows, each step under pi so
    # np.unwrap keeps it) holds it at the bound to the end
    for s in range(3):
        ref[13, N - s:, 2] += 3.0
    # the first acceleration row without u_prev: the rate band holds a_0 of row 1 (120) just inside -35 at N = 33
    x0[14, 3] = 200.0
    return x0, ref, up  # row 15 stays as generated


def _assert_edge_coverage(act, N, what):
    """The rows the batch is built to reach, on the oracle's active sets ``act`` (B, 5N+1)."""
    def sides(rows):
        return {int(c) for c in np.unique(act[:, rows]) if c}

    assert sides([0]) == {1, 2}, f"{what}: v row 0 {sides([0])}"
    assert sides([N]), f"{what}: v row N never active"
    for k in (0, N - 1):
        for c in (0, 1):
            assert sides([N + 1 + 2 * k + c]), f"{what}: input row (step {k}, input {c}) never active"
            assert sides([3 * N + 1 + 2 * k + c]), f"{what}: rate row (step {k}, input {c}) never active"
    for kind, rows in (("speed", slice(0, N + 1)), ("input", slice(N + 1, 3 * N + 1)),
                       ("rate", slice(3 * N + 1, 5 * N + 1))):
        assert sides(rows) == {1, 2}, f"{what}: {kind} rows active on sides {sides(rows)} only"


@pytest.mark.parametrize("with_u_prev", [True, False], ids=["u_prev", "no_u_prev"])
@pytest.mark.parametrize("N", EDGE_N)
@pytest.mark.parametrize("name", EDGE_BLOCKS)
def test_edge_inputs_on_mid_and_wide(cuda, name, N, with_u_prev):
    params = variant_params(name, N)
    x0, ref, up = _edge_batch(N)
    if not with_u_prev:
        up = None
    out = solve(params, x0, ref, up)
    what = f"{name} N={N} {'with' if with_u_prev else 'without'} u_prev"
    acts = _exact_active_sets(params, x0, ref, up, out, what)
    _assert_edge_coverage(acts, N, what)


# ---------------------------------------------------------------------- 5. NULL outputs
@pytest.mark.parametrize("N", [40, 65])
def test_null_outputs_on_mid_and_wide(cuda, N):
    """Every output but ``status`` may be NULL: a kernel that writes one unconditionally faults here.
    Buffers not passed are not passed at all (no undersized or poisoned stand-ins)."""
    import torch
    from mpcqp import _lib, scenarios

    B = 8
    params = variant_params("default", N)
    batch = scenarios.config3(B, horizon=N, seed=8000 + N)
    ctrl = controller(params, B)
    L = _lib.lib()
    x0, ref, up = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (batch.x0, batch.ref, batch.u_prev))
    dev = dict(device="cuda:0")

    def run(*, u0=False, rest=False):
        st = torch.full((B,), 77, dtype=torch.int32, **dev)
        bufs = {"u0": torch.full((B, 2), 7.25, dtype=torch.float64, **dev) if u0 else None,
                "X": torch.full((B, 4, N + 1), 7.25, dtype=torch.float64, **dev) if rest else None,
                "U": torch.full((B, 2, N), 7.25, dtype=torch.float64, **dev) if rest else None,
                "status": st,
                "iters": torch.full((B, 4), 77, dtype=torch.int32, **dev) if rest else None,
                "active": torch.full((B, 5 * N + 1), 77, dtype=torch.uint8, **dev) if rest else None}
        assert L.mpcqp_build(ctrl._ws, B, x0.data_ptr(), ref.data_ptr(), up.data_ptr(), None) == 0
        assert L.mpcqp_solve(ctrl._ws, B, *(None if t is None else t.data_ptr() for t in bufs.values()), None) == 0
        torch.cuda.synchronize()  # raises if the launch faulted
        return {k: None if t is None else t.cpu().numpy() for k, t in bufs.items()}

    full = run(u0=True, rest=True)
    some = run(u0=True)
    none = run()
    ctrl.close()
    assert (full["status"] == 1).all(), full["status"]
    assert np.array_equal(full["u0"], full["U"][:, :, 0]) and (full["active"] <= 2).all()  # the full run wrote them
    assert np.array_equal(some["status"], full["status"]) and np.array_equal(none["status"], full["status"])
    assert np.array_equal(some["u0"].view(np.uint8), full["u0"].view(np.uint8))
