"""GPU tests of the slot table of class-paired mixed launches (``mpcqp_class_slots``, ``k_class_slots`` in
csrc/mpcqp_fleet.hip): which two members of a batch or fleet share a wave.

The contract (include/mpcqp.h) is checked whole against a numpy reading of the table: every member exactly
once, one class per wave, at most one half-empty wave per bucket, -1 / -1 past the used waves, waves class by
class, a class's members in the order of the sequence chunk by chunk -- and the grid's bound, used waves <=
mpcqp_class_slot_waves(V, K) <= V, as a condition on every case."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 1024  # the workgroup's stride over the sequence
SENT = -77  # no member, and not the -1 of an empty half


def _cls(V, K, rng):
    """Class indices in [0, K) with -1, K and 2^31 - 1 mixed in (about one entry in five, from V = 3 on)."""
    cls = rng.integers(0, K, size=V).astype(np.int64)
    if V >= 3:
        bad = rng.random(V) < 0.2
        bad[rng.integers(0, V)] = True
        cls[bad] = rng.choice([-1, K, 2**31 - 1], size=int(bad.sum()))
    return cls.astype(np.int32)


def _slots(V, K, cls, seq):
    """The table of one call, with SENT before the call in it and in eight guard entries behind it."""
    import torch
    from mpcqp import _lib

    L = _lib.lib()
    W = L.mpcqp_class_slot_waves(V, K)
    d_cls = torch.from_numpy(cls).to("cuda:0")
    d_seq = None if seq is None else torch.from_numpy(seq.astype(np.int32)).to("cuda:0")
    d_slots = torch.full((2 * W + 8,), SENT, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.mpcqp_class_slots(V, K, d_cls.data_ptr(), None if d_seq is None else d_seq.data_ptr(),
                                   d_slots.data_ptr(), stream), "mpcqp_class_slots")
    torch.cuda.synchronize()
    out = d_slots.cpu().numpy()
    assert (out[2 * W:] == SENT).all(), "written past the table"
    return W, out[:2 * W].reshape(W, 2)


def check_table(table, W, V, K, cls, seq):
    members = np.arange(V) if seq is None else seq
    bucket_of = np.where((cls >= 0) & (cls < K), cls, K)  # per index of [0, V)
    flat = table.ravel()
    # every entry written; every member exactly once, every other entry -1
    assert (flat != SENT).all(), "an entry of the table was not written"
    assert sorted(flat[flat >= 0]) == sorted(members)
    assert (flat[flat < 0] == -1).all()
    # the grid's bound
    counts = np.bincount(bucket_of[members], minlength=K + 1)
    used = (V + int((counts % 2).sum())) // 2
    assert used <= W <= V
    live = (table >= 0).any(axis=1)
    assert live[:used].all() and not live[used:].any()  # -1 / -1 beyond the used waves, and only there
    # one class per wave, at most one half-empty wave per bucket
    wave_bucket = np.array([bucket_of[row[row >= 0][0]] for row in table[:used]], dtype=np.int64)
    half_empty = np.zeros(K + 1, dtype=int)
    for row, k in zip(table[:used], wave_bucket):
        got = row[row >= 0]
        assert (bucket_of[got] == k).all(), (row, k)
        half_empty[k] += len(got) == 1
    assert (half_empty <= 1).all()
    np.testing.assert_array_equal(half_empty, counts % 2)
    # class-major layout
    assert (np.diff(wave_bucket) >= 0).all()
    # within a class: the order of the sequence, chunk by chunk
    position = np.empty(V, dtype=np.int64)
    position[members] = np.arange(V)
    for k in np.unique(wave_bucket):
        laid = table[:used][wave_bucket == k].ravel()
        chunks = position[laid[laid >= 0]] // CHUNK
        assert (np.diff(chunks) >= 0).all(), f"class {k}: a later chunk's member ahead of an earlier one's"


@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
@pytest.mark.parametrize("V", [1, 2, 3, 7, 64, 1025, 2500])
def test_slot_table_invariants(cuda, V, permuted):
    for K in sorted({1, 3, V}):
        rng = np.random.default_rng(100 * V + K)
        cls = _cls(V, K, rng)
        seq = rng.permutation(V) if permuted else None
        W, table = _slots(V, K, cls, seq)
        check_table(table, W, V, K, cls, seq)


def test_every_class_odd_fills_the_grid(cuda):
    """K + 1 buckets of one member each: the formula's bound is met with equality, every wave half-empty."""
    K = 6
    cls = np.array([0, 1, 2, 3, 4, 5, -1], dtype=np.int32)
    W, table = _slots(7, K, cls, None)
    assert W == 7
    check_table(table, W, 7, K, cls, None)
    assert ((table >= 0).sum(axis=1) == 1).all()


def test_checker_rejects_wrong_tables():
    """The numpy check itself, on the host: a pair across classes, a duplicate, and a class split over two
    half-empty waves are all refused."""
    cls = np.array([0, 0, 1, 1], dtype=np.int32)
    good = np.array([[0, 1], [2, 3], [-1, -1]])
    check_table(good, 3, 4, 2, cls, None)
    for bad in (np.array([[0, 2], [1, 3], [-1, -1]]), np.array([[0, 1], [2, 2], [-1, -1]]),
                np.array([[0, -1], [1, -1], [2, 3]]), np.array([[2, 3], [0, 1], [-1, -1]])):
        with pytest.raises(AssertionError):
            check_table(bad, 3, 4, 2, cls, None)
