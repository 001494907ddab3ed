"""GPU tests of per-QP parameter classes (``mpcqp_set_classes`` / ``mpcqp_build_mixed``): one launch
for a batch whose QPs do not share one ``mpcqp_params`` block.

A mixed launch runs the iteration of the homogeneous kernels unchanged, with the block read per QP
from a device table.  So (1) each QP meets the exact oracle under its own block, and (2) -- the
project's own standard for a kernel variant -- every output of QP b equals, BIT FOR BIT, what a plain
controller built with block ``cls[b]`` returns for it: in the one-wave kernel (N <= 32, pairing
ignored), the mid kernel (33..64), the wide kernel (N > 64) and reproducible mode.  Classes may differ
in solver settings and method too (3).  A class index outside the table is reported per QP and never
indexes anything (4); the calls keep a build tied to the table it was made with (5).

(1) runs at the one-wave horizons only.  The plain controllers that (2) compares with meet the exact
oracle under every variant on all three kernels: ``test_gpu_params.py`` at N = 10 / 20 / 30 and
``test_gpu_params_long.py`` at N = 33 / 40 / 49 / 64 (mid) and 65 / 72 (wide), the horizons 33 / 40 /
64 / 65 of (2) among them -- so a mixed launch at those horizons is tied to the oracle through the
plain launch it equals bit for bit, not only to itself.
"""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import (BAD_CLASS, E_ARG, E_HORIZON, E_STATE, FAIL_NOMINAL, OUTS, assert_exact, assert_same,
                         base_params, controller, fleet_tracker, loop_buffers, take, variant_blocks, varied_fleet)
from param_variants import VARIANTS

pytestmark = pytest.mark.gpu


def _plain(params, batch, idx, **kw):
    ctrl = controller(params, len(idx), **kw)
    up = None if batch.u_prev is None else batch.u_prev[idx]
    out = take(ctrl.solve_batch(batch.x0[idx], batch.ref[idx], up))
    ctrl.close()
    return out


def _mixed(base, plist, cls, batch, idx=None, *, class_settings=None, class_method=None, **kw):
    idx = np.arange(batch.size) if idx is None else idx
    ctrl = controller(base, len(idx), **kw)
    ctrl.set_classes(plist, class_settings, method=class_method)
    out = take(ctrl.solve_batch(batch.x0[idx], batch.ref[idx], batch.u_prev[idx], classes=np.asarray(cls)[idx]))
    ctrl.close()
    return out


def _assert_rows_equal(mixed, rows, plain, what):
    assert_same({k: mixed[k][rows] for k in OUTS}, plain, what)


# ---------------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("N", [10, 20, 30])
def test_mixed_batch_matches_exact_oracle_per_class(cuda, N):
    """The inputs on which test_gpu_params.py shows each variant solves every QP, nine classes in one
    launch: QP b against solve_exact under block cls[b]."""
    import mpc_oracle as mo
    from mpcqp import scenarios

    plist = variant_blocks(N)
    batch = scenarios.config3(48, horizon=N, seed=1000 + N)
    cls = np.arange(batch.size) % len(plist)
    out = _mixed(base_params(N), plist, cls, batch)
    assert (out["status"] == 1).all(), np.unique(out["status"], return_counts=True)
    n_active = 0
    for b in range(batch.size):
        ex = mo.solve_exact(plist[cls[b]], batch.x0[b], batch.ref[b], batch.u_prev[b])
        assert ex.converged
        e = assert_exact(out, b, ex, f"N={N} ({VARIANTS[cls[b]]})")
        print(f"N={N} QP {b} class {VARIANTS[cls[b]]}: rel err {e:.3e}")
        n_active += int((ex.active != 0).any())
    assert n_active > 0


# ---------------------------------------------------------------------- 2. bit identity
@pytest.mark.parametrize("N,B,kw", [(3, 18, {}), (15, 18, dict(pairing="on")), (16, 18, {}), (20, 18, {}),
                                    (32, 18, {}), (33, 18, {}), (40, 18, {}), (64, 18, {}), (65, 9, {}),
                                    (10, 18, dict(reproducible=1))],
                         ids=["N3", "N15_pairing_on", "N16", "N20", "N32", "N33", "N40", "N64", "N65",
                              "N10_reproducible"])
def test_mixed_launch_equals_homogeneous_launches_bitwise(cuda, N, B, kw):
    """For each class c the QPs with cls == c through a plain controller built with block c: the mixed
    launch's outputs for those QPs are the same bits (pairing forced on at N = 15 on both sides: the
    plain side runs two QPs per wave, the mixed launch never does)."""
    from mpcqp import scenarios

    plist = variant_blocks(N)
    batch = scenarios.config3(B, horizon=N, seed=2000 + N)
    cls = np.arange(B) % len(plist)
    mixed = _mixed(base_params(N), plist, cls, batch, **kw)
    for c, p in enumerate(plist):
        rows = np.flatnonzero(cls == c)
        _assert_rows_equal(mixed, rows, _plain(p, batch, rows, **kw), f"N={N} class {VARIANTS[c]}")
    assert (mixed["status"] != BAD_CLASS).all()
    assert (mixed["status"] == 1).any(), mixed["status"]  # solves, not a batch of early exits


@pytest.mark.parametrize("N", [12, 20, 40, 65])
def test_one_class_equals_plain_solve_batch_bitwise(cuda, N):
    """K = 1 with an all-zero cls (an int32 device tensor, used in place) == the plain solve_batch."""
    import torch
    from mpcqp import scenarios

    B = 18 if N <= 64 else 9
    batch = scenarios.config3(B, horizon=N, seed=3000 + N)
    p = base_params(N)
    ctrl = controller(p, B)
    plain = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev))
    ctrl.set_classes([p])
    cls = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    one = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=cls))
    ctrl.close()
    _assert_rows_equal(one, np.arange(B), plain, f"N={N} K=1")
    assert (plain["status"] == 1).any(), plain["status"]


@pytest.mark.parametrize("case", ["cold", "guess", "classes"])
def test_solve_raw_equals_solve_batch_bitwise(cuda, case):
    """``solve_raw`` on device tensors in the C layout == ``solve_batch`` on the same tensors, all six outputs:
    cold, from a guess (the cold U shifted one step), and with classes (two blocks).  The outputs are
    overwritten between the two, so equal bits are the raw call's own."""
    import torch
    from mpcqp import scenarios
    from mpcqp.control.mpc_controller import BatchSolution

    N, B = 10, 8
    batch = scenarios.config3(B, horizon=N, seed=4000 + N)
    ctrl = controller(base_params(N), B)
    x0, ref, up = (torch.from_numpy(a).to(cuda) for a in (batch.x0, batch.ref, batch.u_prev))
    kw = {}
    if case == "guess":
        U = ctrl.solve_batch(x0, ref, up).U
        kw = dict(U_guess=torch.cat([U[:, :, 1:], U[:, :, -1:]], dim=2).contiguous())
    elif case == "classes":
        ctrl.set_classes(variant_blocks(N, VARIANTS[:2]))
        kw = dict(classes=torch.from_numpy((np.arange(B) % 2).astype(np.int32)).to(cuda))
    want = take(ctrl.solve_batch(x0, ref, up, **kw))
    outs = BatchSolution(ctrl._u0, ctrl._X, ctrl._U, ctrl._status, ctrl._iters, ctrl._active)
    for t in outs:
        t.fill_(77)
    assert ctrl.solve_raw(B, x0, ref, up, torch.cuda.current_stream(cuda), **kw) is None
    got = take(outs)
    ctrl.close()
    assert_same(got, want, f"solve_raw ({case})")
    assert (want["status"] == 1).any(), want["status"]  # solves, not a batch of early exits


# ---------------------------------------------------------------------- 3. settings per class
def test_classes_differ_in_solver_settings(cuda):
    """Class 0 the defaults, class 1 one ADMM iteration without polish: solved and max_iter side by
    side in one launch, and the class 0 results do not depend on their neighbours."""
    from mpcqp import scenarios

    N, B = 20, 24
    p = base_params(N)
    batch = scenarios.config3(B, horizon=N, seed=41)
    cls = np.arange(B) % 2
    out = _mixed(p, [p, p], cls, batch, class_settings=[{}, FAIL_NOMINAL])
    assert (out["status"][cls == 0] == 1).all() and (out["status"][cls == 1] == -2).all(), out["status"]
    assert (out["iters"][cls == 1, 0] == 1).all() and (out["iters"][cls == 1, 1] == 0).all()
    _assert_rows_equal(out, np.flatnonzero(cls == 0), _plain(p, batch, np.flatnonzero(cls == 0)), "defaults")
    _assert_rows_equal(out, np.flatnonzero(cls == 1), _plain(p, batch, np.flatnonzero(cls == 1), **FAIL_NOMINAL),
                       "one iteration")


def test_classes_differ_in_method(cuda):
    """Class 1 runs method newton (the polish iteration alone) beside ADMM in class 0."""
    from mpcqp import scenarios

    N, B = 20, 24
    p = base_params(N)
    batch = scenarios.config3(B, horizon=N, seed=42)
    cls = np.arange(B) % 2
    out = _mixed(p, [p, p], cls, batch, class_method=["admm", "newton"])
    assert (out["status"] == 1).all(), out["status"]
    assert (out["iters"][cls == 0, 0] > 0).all() and (out["iters"][cls == 1, 0] == 0).all()  # ADMM iterations
    _assert_rows_equal(out, np.flatnonzero(cls == 0), _plain(p, batch, np.flatnonzero(cls == 0)), "admm")
    _assert_rows_equal(out, np.flatnonzero(cls == 1), _plain(p, batch, np.flatnonzero(cls == 1), method="newton"),
                       "newton")


# ---------------------------------------------------------------------- 4. bad indices
@pytest.mark.parametrize("N", [20, 40, 65])
def test_bad_class_indices_are_reported_per_qp(cuda, N):
    """cls holding -1, K and 2^31 - 1 among valid entries: those QPs report MPCQP_BAD_CLASS with zero
    iters and nothing else of theirs is written; every valid QP equals the run without the bad ones.
    The guard is index arithmetic ahead of every access, so this passes only when it holds."""
    from mpcqp import scenarios

    B = 12
    plist = variant_blocks(N)[:4]
    K = len(plist)
    batch = scenarios.config3(B, horizon=N, seed=4000 + N)
    cls = np.arange(B) % K
    bad = {2: -1, 5: K, 9: 2**31 - 1}
    for b, c in bad.items():
        cls[b] = c
    good = np.array([b for b in range(B) if b not in bad])
    ctrl = controller(base_params(N), B)
    ctrl.set_classes(plist)
    for buf, fill in ((ctrl._u0, 7.25), (ctrl._X, 7.25), (ctrl._U, 7.25), (ctrl._active, 77), (ctrl._iters, 77)):
        buf.fill_(fill)
    out = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=cls))  # returns, and the sync is clean
    ctrl.close()
    rows = np.array(sorted(bad))
    assert (out["status"][rows] == BAD_CLASS).all(), out["status"]
    assert (out["iters"][rows] == 0).all()
    for k, fill in (("u0", 7.25), ("X", 7.25), ("U", 7.25), ("active", 77)):
        assert (out[k][rows] == fill).all(), f"{k} of a bad-class QP was written"
    assert (out["status"][good] == 1).any(), out["status"]
    _assert_rows_equal(out, good, _mixed(base_params(N), plist, cls, batch, good), f"N={N} valid QPs")


# ---------------------------------------------------------------------- 5. state rules
def test_class_state_rules(cuda):
    import torch
    from mpcqp import _lib, scenarios

    N, B = 12, 10
    p = base_params(N)
    plist = variant_blocks(N)[:3]
    batch = scenarios.config3(B, horizon=N, seed=5)
    ctrl = controller(p, B)
    L, ws = ctrl._L, ctrl._ws
    x0, ref, up = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (batch.x0, batch.ref, batch.u_prev))
    cls = torch.from_numpy((np.arange(B) % 3).astype(np.int32)).to("cuda:0")
    outs = (ctrl._u0, ctrl._X, ctrl._U, ctrl._status, ctrl._iters, ctrl._active)

    def build_mixed():
        return L.mpcqp_build_mixed(ws, B, x0.data_ptr(), ref.data_ptr(), up.data_ptr(), cls.data_ptr(), None)

    def solve():
        return L.mpcqp_solve(ws, B, *(t.data_ptr() for t in outs), None)

    # no table yet
    assert build_mixed() == E_STATE
    assert b"class table" in L.mpcqp_last_error()
    with pytest.raises(ValueError):
        ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=np.zeros(B, np.int32))
    # a block with another horizon / with debug_state is refused and leaves no table behind
    wrong = _lib.class_table([base_params(N + 1)])
    assert L.mpcqp_set_classes(ws, 1, wrong) == E_HORIZON
    dbg = _lib.class_table(plist)
    dbg[1].debug_state = 1
    assert L.mpcqp_set_classes(ws, 3, dbg) == E_ARG
    assert L.mpcqp_set_classes(ws, 3, None) == E_ARG and L.mpcqp_set_classes(ws, -1, dbg) == E_ARG
    assert build_mixed() == E_STATE
    # a new table invalidates a mixed build: the solve would run under blocks the build did not see
    ctrl.set_classes(plist)
    assert build_mixed() == 0
    ctrl.set_classes(plist)
    assert solve() == E_STATE
    assert build_mixed() == 0 and solve() == 0
    mixed = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=cls))
    for c in range(3):
        rows = np.flatnonzero(np.arange(B) % 3 == c)
        _assert_rows_equal(mixed, rows, _plain(plist[c], batch, rows), f"class {c}")
    # set_params leaves the table alone (and invalidates the build, as ever)
    assert build_mixed() == 0
    ctrl.set_params(p)
    assert solve() == E_STATE
    assert build_mixed() == 0 and solve() == 0
    # a plain build after a mixed one solves under the workspace's own block
    plain = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev))
    _assert_rows_equal(plain, np.arange(B), _plain(p, batch, np.arange(B)), "plain after mixed")
    # dropping the table
    ctrl.set_classes(None)
    assert ctrl.num_classes == 0 and build_mixed() == E_STATE
    with pytest.raises(ValueError):
        ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=cls)
    again = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev))
    _assert_rows_equal(again, np.arange(B), plain, "plain after the table is dropped")
    torch.cuda.synchronize()
    ctrl.close()


_FILLS = (("_u0", 7.25), ("_X", 7.25), ("_U", 7.25), ("_status", 77), ("_iters", 77), ("_active", 77))


def _raw_solve(ctrl, B):
    """mpcqp_solve on the controller's own output buffers, as the C caller sees it."""
    return ctrl._L.mpcqp_solve(ctrl._ws, B, *(getattr(ctrl, name).data_ptr() for name, _ in _FILLS), None)


def test_solve_without_a_valid_build_is_refused(cuda, golden):
    """mpcqp_solve answers MPCQP_E_STATE, and launches nothing, when the workspace holds no valid
    build: B = -1 on a fresh workspace (once the value that stood for "no build"), and any B after a
    fleet step has used the workspace of an earlier mpcqp_build."""
    import ctypes

    import torch
    from mpcqp import scenarios

    N, V = 3, 2
    g, paths, starts, goals = varied_fleet(golden, V, seed=5)
    ft = fleet_tracker(N, V, 128, 4, use_graph=False)
    ctrl = ft._nominal
    L, ws = ctrl._L, ctrl._ws
    for name, fill in _FILLS:
        getattr(ctrl, name).fill_(fill)
    assert _raw_solve(ctrl, -1) == E_STATE
    assert b"mpcqp_build" in L.mpcqp_last_error()
    batch = scenarios.config3(V, horizon=N, seed=8)
    x0, ref, up = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (batch.x0, batch.ref, batch.u_prev))
    assert L.mpcqp_build(ws, V, x0.data_ptr(), ref.data_ptr(), up.data_ptr(), None) == 0
    ft.reset_from_plans(paths, starts, goals)
    assert L.mpcqp_fleet_step(ws, ft._relaxed._ws, ctypes.byref(ft._fleet), None) == 0
    assert _raw_solve(ctrl, -1) == E_STATE
    assert _raw_solve(ctrl, V) == E_STATE
    torch.cuda.synchronize()
    assert (ft.buffers()["mask"][0].cpu().numpy() == 1).all()  # the fleet step itself ran
    for name, fill in _FILLS:
        assert (getattr(ctrl, name).cpu().numpy() == fill).all(), f"{name} was written"
    ft.close()


def test_fused_loop_after_a_mixed_build_equals_fresh_workspaces(cuda, golden):
    """A fleet call invalidates the whole build record, the class indices of an mpcqp_build_mixed
    included: the fused loop (pairing forced on, three vehicles: a half-empty last wave) on workspaces
    whose nominal one last held a mixed build leaves every fleet buffer as on fresh workspaces, bit for
    bit, and mpcqp_solve afterwards needs a new build."""
    import torch
    from mpcqp import scenarios

    N, V, steps = 3, 3, 4
    g, paths, starts, goals = varied_fleet(golden, V, seed=5)
    batch = scenarios.config3(V, horizon=N, seed=9)
    bufs = []
    for mixed_first in (False, True):
        ft = fleet_tracker(N, V, 128, steps, fused=True)
        for c in (ft._nominal, ft._relaxed):
            c.set_pairing("on")
        if mixed_first:
            ft._nominal.set_classes(variant_blocks(N)[:2])
            out = take(ft._nominal.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=np.arange(V) % 2))
            assert (out["status"] != BAD_CLASS).all() and (out["status"] == 1).any(), out["status"]
        ft.reset_from_plans(paths, starts, goals)
        ft.step(steps)
        torch.cuda.synchronize()
        bufs.append(loop_buffers(ft, tuple(ft.buffers())))
        assert _raw_solve(ft._nominal, V) == E_STATE
        ft.close()
    assert (bufs[0]["steps"] > 0).any(), bufs[0]["steps"]  # the loop stepped
    for k in bufs[0]:
        np.testing.assert_array_equal(bufs[0][k], bufs[1][k], err_msg=k)
