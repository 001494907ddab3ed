"""The measuring rule of the tools (``tools/bench_common.py``) on the host: the order of the legs,
which repeats count, the setup hook, what an exception does, the timed window's call sequence and the summary;
and ``scenarios.pairs`` against the function it replaced.  No library and no device."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

TOOLS = Path(__file__).resolve().parents[1] / "tools"
if str(TOOLS) not in sys.path:
    sys.path.insert(0, str(TOOLS))

import bench_common as bc  # noqa: E402


def _legs(log, names="abc", fail=None):
    """Legs that append their name to ``log`` and return (name, how many times they ran before); ``fail`` =
    (name, nth run): that run of that leg raises."""
    runs = {k: 0 for k in names}

    def leg(k):
        def fn():
            log.append(k)
            runs[k] += 1
            if fail == (k, runs[k] - 1):
                raise RuntimeError(f"leg {k}")
            return k, runs[k] - 1
        return fn

    return {k: leg(k) for k in names}


def test_the_order_rotates_and_repeat_0_is_dropped():
    log = []
    values, last = bc.interleaved(_legs(log), 3, setup=lambda: log.append("|"))
    assert "".join(log) == "|abc|bca|cab|abc"  # the hook once before each repeat's first leg: four times
    assert log.count("|") == 4
    # only the last three repeats' values, in repeat order
    assert values == {k: [(k, 1), (k, 2), (k, 3)] for k in "abc"}
    assert last == {k: (k, 3) for k in "abc"}
    assert list(values) == list("abc")


def test_value_picks_what_is_collected_and_last_keeps_the_whole_return():
    values, last = bc.interleaved(_legs([]), 2, value=lambda ret: ret[1])
    assert values == {k: [1, 2] for k in "abc"} and last == {k: (k, 2) for k in "abc"}


def test_rotation_off_keeps_the_given_order():
    log = []
    values, _ = bc.interleaved(_legs(log), 3, setup=lambda: log.append("|"), rotate=False)
    assert "".join(log) == "|abc|abc|abc|abc"
    assert values == {k: [(k, 1), (k, 2), (k, 3)] for k in "abc"}


def test_warm_up_off_runs_reps_repeats_and_collects_all():
    log = []
    values, last = bc.interleaved(_legs(log), 3, setup=lambda: log.append("|"), warmup=False)
    assert "".join(log) == "|abc|bca|cab"
    assert values == {k: [(k, 0), (k, 1), (k, 2)] for k in "abc"}
    log.clear()
    values, _ = bc.interleaved(_legs(log), 2, rotate=False, warmup=False)  # mixed_bench.py, b1_latency.py --warm
    assert "".join(log) == "abcabc" and values == {k: [(k, 0), (k, 1)] for k in "abc"}


def test_an_exception_from_a_leg_ends_the_run_there():
    log = []
    with pytest.raises(RuntimeError, match="leg c"):
        bc.interleaved(_legs(log, fail=("c", 1)), 3)  # repeat 1 visits b, c, a: a is never started
    assert "".join(log) == "abc" + "bc"


def test_an_exception_from_the_hook_ends_the_run_there():
    log = []

    def hook():
        if len(log) == 3:
            raise ValueError("hook")

    with pytest.raises(ValueError, match="hook"):
        bc.interleaved(_legs(log), 3, setup=hook)
    assert "".join(log) == "abc"


def test_the_timed_window():
    log = []
    ticks = iter([10.0, 12.5])

    def clock():
        log.append("clock")
        return next(ticks)

    dt, out = bc.timed(lambda: log.append("fn") or "result", lambda: log.append("sync"), clock)
    assert log == ["sync", "clock", "fn", "sync", "clock"]
    assert dt == 2.5 and out == "result"


def test_the_summary():
    ts = [3.0, 1.0, 2.0]
    assert bc.summary(ts) == {"median": 2.0, "min": 1.0, "max": 3.0, "all": [3.0, 1.0, 2.0]}
    assert bc.summary([4.0, 1.0])["median"] == 2.5


def test_loop_counts():
    from types import SimpleNamespace

    res = SimpleNamespace(steps=np.array([3, 5, 2]), phase=np.array([1, 2, 1]), replans=np.array([0, 2, 1]))
    assert bc.loop_counts(res) == {"vehicle_steps": 10, "goal_reached": 2, "aborted": 1}
    assert bc.loop_counts(res, ("vehicle_steps", "goal_reached", "replans")) == {
        "vehicle_steps": 10, "goal_reached": 2, "replans": 3}


def _old_pairs(occ, V, seed):
    """``tools/swarm_bench.py``'s and ``tests/gpu_helpers.py``'s function before it moved, kept literally."""
    rng = np.random.default_rng(seed)
    free = np.argwhere(occ == 1)
    s, g = [], []
    while len(s) < V:
        a, b = free[rng.integers(0, len(free), 2)]
        if np.hypot(*(a - b)) > 30:
            s.append(a[::-1].astype(float))
            g.append(b[::-1].astype(float))
    return np.array(s), np.array(g)


@pytest.mark.parametrize("V,seed", [(3, 5), (100, 9)])
def test_scenarios_pairs_is_the_function_it_replaced(V, seed):
    import gpu_helpers
    from mpcqp import scenarios

    occ = bc.default_grid()
    assert occ is bc.default_grid() and occ.shape == (80, 80)  # loaded once
    assert gpu_helpers.pairs is scenarios.pairs  # the tests' name is the same function
    got, want = scenarios.pairs(occ, V, seed), _old_pairs(occ, V, seed)
    for x, y in zip(got, want):
        assert x.shape == (V, 2) and x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
