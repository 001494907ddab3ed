"""GPU tests of mixed batches at two QPs per wave (``mpcqp_set_class_pairing``, ``k_solve_pair_mixed`` in
csrc/mpcqp_solve.h; ``BatchedMPCController(class_pairing="on")``).

The claim: a mixed launch that pairs QPs of the same class returns, BIT FOR BIT, what the same launch returns
at one QP per wave -- every field of ``OUTS``, whatever the two halves of a wave do apart (iteration counts,
polish passes, statuses, a class index outside the table) -- and ``launch_info()`` says which of the two ran.
The unpaired mixed launch is itself tied to the plain launches and to the exact oracle by
``test_gpu_classes.py``; one spot check against the exact oracle stands here as well.  The switch is opt-in:
with it off a mixed launch runs one QP per wave whatever ``pairing`` says, as before."""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import (BAD_CLASS, E_ARG, FAIL_NOMINAL, OUTS, assert_exact, assert_same, base_params, controller,
                         take, variant_blocks)
from param_variants import VARIANTS

pytestmark = pytest.mark.gpu

FILLS = (("_u0", 7.25), ("_X", 7.25), ("_U", 7.25), ("_status", 77), ("_iters", 77), ("_active", 77))
KNOWN_PARTNERS_SEED = 7100  # test_known_partners_part_ways: picked with the C restatement (oracle/cpu_solver.py)


def _waves(B, K):
    from mpcqp import _lib

    return _lib.lib().mpcqp_class_slot_waves(B, K)


def _both(base, plist, cls, batch, *, class_settings=None, class_method=None, fill=False, **kw):
    """The same mixed launch on one controller with class pairing off, then on: (off, on, launch_info of each).
    ``fill``: every output buffer holds a sentinel before each launch."""
    ctrl = controller(base, batch.size, **kw)
    ctrl.set_classes(plist, class_settings, method=class_method)
    outs, infos = [], []
    for mode in ("off", "on"):
        ctrl.set_class_pairing(mode)
        if fill:
            for name, value in FILLS:
                getattr(ctrl, name).fill_(value)
        outs.append(take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=np.asarray(cls))))
        infos.append(ctrl.launch_info())
    ctrl.close()
    return outs[0], outs[1], infos[0], infos[1]


# ---------------------------------------------------------------------- 1. paired against unpaired
@pytest.mark.parametrize("N", [1, 3, 10, 15])
def test_class_paired_launch_equals_unpaired_bitwise(cuda, N):
    """19 QPs over the nine variants, cls = b % 9: one class of three (a half-empty wave) and eight of two."""
    import mpc_oracle as mo
    from mpcqp import _lib, scenarios

    B = 19
    plist = variant_blocks(N)
    K = len(plist)
    batch = scenarios.config3(B, horizon=N, seed=6000 + N)
    cls = np.arange(B) % K
    off, on, info_off, info_on = _both(base_params(N), plist, cls, batch)
    assert info_off["kind"] == info_on["kind"] == _lib.LAUNCH_SOLVE_MIXED
    assert info_off["per_wave"] == 1 and info_off["workgroups"] == B
    assert info_on["per_wave"] == 2 and info_on["workgroups"] == _waves(B, K) == 14 and info_on["count"] == B
    assert_same(on, off, f"N={N} class pairing on against off")
    assert (off["status"] == 1).any(), off["status"]  # solves, not a batch of early exits
    assert (on["status"] != BAD_CLASS).all()
    if N == 10:  # three QPs against the exact oracle, each under its own block
        for b in (0, 7, 18):
            ex = mo.solve_exact(plist[cls[b]], batch.x0[b], batch.ref[b], batch.u_prev[b])
            assert ex.converged
            e = assert_exact(on, b, ex, f"class-paired ({VARIANTS[cls[b]]})", solved=True)
            print(f"QP {b} class {VARIANTS[cls[b]]}: rel err {e:.3e}")


def test_switch_off_keeps_one_per_wave_under_pairing_on(cuda):
    """Today's behaviour, which the switch leaves alone: pairing="on" does not pair a mixed launch."""
    from mpcqp import scenarios

    N, B = 10, 19
    plist = variant_blocks(N)
    batch = scenarios.config3(B, horizon=N, seed=6010)
    ctrl = controller(base_params(N), B, pairing="on")
    ctrl.set_classes(plist)
    out = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=np.arange(B) % len(plist)))
    info = ctrl.launch_info()
    ctrl.close()
    assert info["per_wave"] == 1 and info["workgroups"] == B, info
    assert (out["status"] == 1).any()


# ---------------------------------------------------------------------- 2. known partners
def test_known_partners_part_ways(cuda):
    """B = 2 K, every class exactly two QPs: the pair of each wave is known.  On this seed (picked on the CPU,
    whose counters equal the kernel's) some partners differ in ADMM iterations and some in polish passes --
    one half polishes while the other still iterates -- which is asserted on the unpaired result first."""
    from mpcqp import scenarios

    N = 10
    plist = variant_blocks(N)
    K = len(plist)
    batch = scenarios.config3(2 * K, horizon=N, seed=KNOWN_PARTNERS_SEED)
    cls = np.arange(2 * K) // 2
    off, on, _, info_on = _both(base_params(N), plist, cls, batch)
    it = off["iters"].reshape(K, 2, 4)
    print("ADMM iterations per pair", it[:, :, 0].tolist(), "polish passes", it[:, :, 1].tolist())
    assert (it[:, 0, 0] != it[:, 1, 0]).any(), "no pair differs in ADMM iterations"
    assert (it[:, 0, 1] != it[:, 1, 1]).any(), "no pair differs in polish passes"
    assert info_on["per_wave"] == 2 and info_on["workgroups"] == _waves(2 * K, K)
    assert_same(on, off, "known partners")


# ---------------------------------------------------------------------- 3. divergent settings
def test_partner_classes_differ_in_settings_and_method(cuda):
    """Class 0 the defaults, class 1 one ADMM iteration without polish, class 2 method newton, in waves next
    to each other: each class is the unpaired result bit for bit, with test_gpu_classes.py's statuses."""
    from mpcqp import scenarios

    N, B = 10, 19
    p = base_params(N)
    batch = scenarios.config3(B, horizon=N, seed=6030)
    cls = np.arange(B) % 3
    off, on, _, info_on = _both(p, [p, p, p], cls, batch, class_settings=[{}, FAIL_NOMINAL, {}],
                                class_method=["admm", "admm", "newton"])
    assert info_on["per_wave"] == 2
    assert (on["status"][cls == 0] == 1).all() and (on["status"][cls == 1] == -2).all(), on["status"]
    assert (on["iters"][cls == 1, 0] == 1).all() and (on["iters"][cls == 1, 1] == 0).all()
    assert (on["status"][cls == 2] == 1).all()
    assert (on["iters"][cls == 0, 0] > 0).all() and (on["iters"][cls == 2, 0] == 0).all()  # ADMM iterations
    for c in range(3):
        assert_same({k: on[k][cls == c] for k in OUTS}, {k: off[k][cls == c] for k in OUTS}, f"class {c}")


# ---------------------------------------------------------------------- 4. bad classes
@pytest.mark.parametrize("case", ["lone", "two", "even_classes"])
def test_bad_class_in_a_paired_launch(cuda, case):
    """Indices outside [0, K) form a bucket of their own: a lone one sits in a half-empty wave, two share a
    wave (either half's first lane reports), and with every good class even no good QP's wave is touched.
    They report BAD_CLASS with zero iters and nothing else of theirs is written; everyone else is as in the
    unpaired launch."""
    from mpcqp import scenarios

    N, K = 10, 3
    plist = variant_blocks(N)[:K]
    if case == "even_classes":
        cls = np.array([0, 0, 1, 1, 2, 2, 0, 0, 2**31 - 1], dtype=np.int64)
    else:
        cls = np.arange(13) % K
        cls[4] = -1
        if case == "two":
            cls[9] = K
    B = len(cls)
    bad = np.flatnonzero((cls < 0) | (cls >= K))
    good = np.flatnonzero((cls >= 0) & (cls < K))
    batch = scenarios.config3(B, horizon=N, seed=6040)
    off, on, _, info_on = _both(base_params(N), plist, cls, batch, fill=True)
    assert info_on["per_wave"] == 2 and info_on["workgroups"] == _waves(B, K)
    assert (on["status"][bad] == BAD_CLASS).all(), on["status"]
    assert (on["iters"][bad] == 0).all()
    for k, fill in (("u0", 7.25), ("X", 7.25), ("U", 7.25), ("active", 77)):
        assert (on[k][bad] == fill).all(), f"{k} of a bad-class QP was written"
    assert (on["status"][good] == 1).any(), on["status"]
    assert (on["status"][good] != 77).all()
    assert_same(on, off, f"{case}: every QP against the unpaired launch")


# ---------------------------------------------------------------------- 5. other small cases
def test_one_class_equals_the_plain_paired_launch_bitwise(cuda):
    """K = 1: the class-paired mixed launch against k_solve_pair under pairing="on"."""
    import torch
    from mpcqp import scenarios

    N, B = 12, 19
    p = base_params(N)
    batch = scenarios.config3(B, horizon=N, seed=6050)
    ctrl = controller(p, B, pairing="on", class_pairing="on")
    plain = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev))
    assert ctrl.launch_info()["per_wave"] == 2
    ctrl.set_classes([p])
    one = take(ctrl.solve_batch(batch.x0, batch.ref, batch.u_prev, classes=torch.zeros(B, dtype=torch.int32, device="cuda:0")))
    info = ctrl.launch_info()
    ctrl.close()
    assert info["per_wave"] == 2 and info["workgroups"] == _waves(B, 1) == 10, info
    assert_same(one, plain, "K = 1")
    assert (plain["status"] == 1).any(), plain["status"]


@pytest.mark.parametrize("B", [1, 2])
def test_smallest_batches(cuda, B):
    from mpcqp import scenarios

    N = 10
    plist = variant_blocks(N)[:2]
    batch = scenarios.config3(B, horizon=N, seed=6060 + B)
    off, on, _, info_on = _both(base_params(N), plist, np.ones(B, np.int32), batch)
    assert info_on["per_wave"] == 2 and info_on["workgroups"] == _waves(B, 2) == B  # B = 2: the grid's bound, one wave used
    assert_same(on, off, f"B = {B}")
    assert (on["status"] == 1).all(), on["status"]


@pytest.mark.parametrize("N,kw", [(16, {}), (10, dict(reproducible=1))], ids=["N16", "N10_reproducible"])
def test_without_the_paired_kernel_the_switch_changes_nothing(cuda, N, kw):
    """N > 15 and reproducible mode have no paired kernel: one QP per wave with the switch on, the same bits."""
    from mpcqp import scenarios

    B = 19
    plist = variant_blocks(N)
    batch = scenarios.config3(B, horizon=N, seed=6070 + N)
    off, on, info_off, info_on = _both(base_params(N), plist, np.arange(B) % len(plist), batch, **kw)
    assert info_on == info_off and info_on["per_wave"] == 1 and info_on["workgroups"] == B, info_on
    assert_same(on, off, f"N={N} {kw}")
    assert (on["status"] == 1).any()


def test_more_classes_than_the_slot_pass_supports_fall_back(cuda):
    """K above MPCQP_CLASS_SLOT_MAX_CLASSES: one QP per wave, the same bits."""
    from mpcqp import _lib, scenarios

    N, B = 10, 19
    K = _lib.CLASS_SLOT_MAX_CLASSES + 1
    blocks = variant_blocks(N)[:3]
    plist = [blocks[k % 3] for k in range(K)]
    batch = scenarios.config3(B, horizon=N, seed=6080)
    cls = np.arange(B) % 3
    cls[5] = K - 1
    off, on, info_off, info_on = _both(base_params(N), plist, cls, batch)
    assert info_on == info_off and info_on["per_wave"] == 1, info_on
    assert_same(on, off, "K above the cap")
    assert (on["status"] == 1).any()


def test_switch_argument_checks(cuda):
    ctrl = controller(base_params(10), 4)
    assert ctrl.class_pairing == "off"
    assert ctrl._L.mpcqp_set_class_pairing(ctrl._ws, 2) == E_ARG
    assert ctrl._L.mpcqp_set_class_pairing(ctrl._ws, -1) == E_ARG
    ctrl.set_class_pairing("on")
    ctrl.set_class_pairing("on")  # the table is there: nothing to allocate
    ctrl.set_class_pairing("off")
    assert ctrl.class_pairing == "off"
    ctrl.close()
