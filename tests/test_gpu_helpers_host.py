"""The assertion helpers of ``gpu_helpers`` on the host: they carry the oracle contract for every GPU test,
so each is shown to pass on the oracle's own answer and to raise on the smallest violation of each clause.
Horizon 3, two QPs of ``scenarios.config3(2, horizon=3, seed=1)``, ``out`` built from ``solve_exact`` itself:
no library and no device."""
from __future__ import annotations

import numpy as np
import pytest
from gpu_helpers import OUTS, REL_TOL, assert_exact, assert_same, base_params, check_against_oracle, config3_case, rel

N = 3


@pytest.fixture(scope="module")
def case():
    """(params, batch, the two solve_exact results, out as a solver would return it) -- not to be written to."""
    import mpc_oracle as mo
    from mpcqp import scenarios

    params = base_params(N)
    batch = scenarios.config3(2, horizon=N, seed=1)
    exact = [mo.solve_exact(params, batch.x0[b], batch.ref[b], batch.u_prev[b]) for b in range(2)]
    assert all(e.converged for e in exact)
    out = dict(U=np.stack([e.Umat for e in exact]), X=np.stack([e.X for e in exact]),
               u0=np.stack([e.Umat[:, 0] for e in exact]), active=np.stack([e.active for e in exact]),
               status=np.ones(2, np.int32), iters=np.zeros((2, 4), np.int32))
    return params, batch, exact, out


def _copy(out):
    return {k: v.copy() for k, v in out.items()}


def _check(case, out):
    params, batch, exact, _ = case
    worst = check_against_oracle(params, batch.x0, batch.ref, batch.u_prev, out, range(2), "host")
    for b in range(2):
        assert assert_exact(out, b, exact[b], "host", solved=True) <= worst
    return worst


def test_rel_by_hand():
    assert rel(np.array([0.0, 3.0]), np.array([0.0, 2.0])) == 0.5  # |3 - 2| / max(1, 2)
    assert rel(np.array([1e-3]), np.array([0.0])) == 1e-3  # the denominator's floor of 1.0
    assert rel(np.array([1e-3]), np.array([0.5])) == 0.5 - 1e-3


def test_the_oracles_own_answer_passes(case):
    assert _check(case, case[3]) == 0.0
    one = {k: v[1] for k, v in case[3].items()}
    assert assert_exact(one, None, case[2][1], "one QP", solved=True) == 0.0  # an ``out`` that holds one QP


@pytest.mark.parametrize("name", ["U", "X", "u0"])
def test_a_value_off_by_twice_the_tolerance_raises(case, name):
    """One entry moved by 2 REL_TOL relative, scaled as ``rel`` scales; half the tolerance still passes."""
    want = {"U": case[2][1].Umat, "X": case[2][1].X, "u0": case[2][1].Umat[:, 0]}[name]
    scale = max(1.0, np.abs(want).max())
    entry = (1,) + np.unravel_index(np.abs(want).argmin(), want.shape)  # QP 1's smallest entry: the maximum stays
    for factor, passes in ((0.5, True), (2.0, False)):
        out = _copy(case[3])
        out[name][entry] += factor * REL_TOL * scale
        if passes:
            assert 0.4 * REL_TOL <= _check(case, out) <= 0.6 * REL_TOL
        else:
            with pytest.raises(AssertionError, match="rel err"):
                _check(case, out)
            with pytest.raises(AssertionError, match="rel err"):
                assert_exact(out, 1, case[2][1], "host")
            assert assert_exact(out, 0, case[2][0], "host") == 0.0  # the other QP is untouched


def test_a_flipped_active_code_raises(case):
    out = _copy(case[3])
    out["active"][0, 2] = (out["active"][0, 2] + 1) % 3
    with pytest.raises(AssertionError, match="active set differs in rows \\[2\\]"):
        _check(case, out)


def test_status_is_held_where_the_call_asks_for_solved(case):
    out = _copy(case[3])
    out["status"][1] = 2  # solved_inaccurate
    with pytest.raises(AssertionError, match="status"):
        assert_exact(out, 1, case[2][1], "host", solved=True)
    assert assert_exact(out, 1, case[2][1], "host") == 0.0  # not asked for: the caller asserts it
    params, batch, _, _ = case
    assert check_against_oracle(params, batch.x0, batch.ref, batch.u_prev, out, range(2)) == 0.0


def test_assert_same_is_bitwise_over_the_named_outputs(case):
    got, want = _copy(case[3]), case[3]
    assert_same(got, want, "equal")
    got["X"].view(np.uint64)[1, 2, 1] ^= 1  # the last bit of one double
    assert rel(got["X"], want["X"]) < 1e-15
    with pytest.raises(AssertionError, match="one bit: X"):
        assert_same(got, want, "one bit")
    with pytest.raises(AssertionError):
        assert_same(got, want, "one bit", names=("U", "X"))
    assert_same(got, want, "X left out", names=tuple(k for k in OUTS if k != "X"))


def test_config3_case_is_cached_by_every_argument():
    a = config3_case(N, 2, 1)
    assert config3_case(N, 2, 1) is a  # served from the cache
    b = config3_case(N, 2, 2)
    assert b is not a and not np.array_equal(a["x0"], b["x0"])
    m = config3_case(N, 2, 1, margins=True)
    assert m is not a and "margins" not in a and m["margins"].shape == (2,)
    np.testing.assert_array_equal(m["guesses"], a["guesses"])
    assert all(e.converged for e in a["exact"]) and a["guesses"].shape == (2, 2, N)
