"""tests/knn_ref.py pinned on the CPU: topk() against the literal insertion loop on heavily tied matrices, and
against the two existing k = 2 yardsticks (oracle.knn2 for float rows, hamming_ref.knn2 for binary rows)."""
import numpy as np
import pytest

import cross_ref
import float_ref
import hamming_ref
import knn_ref

FLT_MAX = knn_ref.FLT_MAX


def _same(got, exp):
    np.testing.assert_array_equal(got[0], exp[0])
    np.testing.assert_array_equal(got[1].view(np.int32), exp[1].view(np.int32))


def test_topk_equals_the_insertion_loop_on_tied_matrices():
    rng = np.random.default_rng(0x70B4)
    for trial in range(300):
        nq, nt = int(rng.integers(1, 6)), int(rng.integers(0, 40))
        k = int(rng.integers(1, knn_ref.MAX_K + 1))
        d = rng.integers(0, int(rng.integers(1, 6)), size=(nq, nt)).astype(np.float32)  # at most 5 distinct values
        if trial % 3 == 0 and nt:  # entries that are never inserted, among them whole rows
            bad = rng.random((nq, nt)) < 0.4
            d[bad] = rng.choice(np.array([np.inf, FLT_MAX, np.nan], np.float32), size=int(bad.sum()))
            if trial % 6 == 0:
                d[0] = np.inf
        _same(knn_ref.topk(d, k), knn_ref.insertion_loop(d, k))


def test_absent_entries():
    d = np.array([[3, 1, FLT_MAX, 1, np.inf]], np.float32)
    idx, dist = knn_ref.topk(d, 5)
    assert idx.tolist() == [[1, 3, 0, -1, -1]] and dist.tolist() == [[1, 1, 3, FLT_MAX, FLT_MAX]]
    idx, dist = knn_ref.topk(np.zeros((2, 0), np.float32), 3)
    assert (idx == -1).all() and (dist == FLT_MAX).all() and idx.shape == (2, 3)
    assert knn_ref.topk(np.zeros((0, 4), np.float32), 2)[0].shape == (0, 2)


@pytest.mark.parametrize("dim", [7, 64, 128])
def test_k2_equals_oracle_knn2(oracle, dim):
    rng = np.random.default_rng(dim)
    q, t = float_ref.normal_rows(rng, 40, dim), float_ref.normal_rows(rng, 90, dim)
    t[50], t[70] = t[3], t[3]
    q[0] = t[3]
    _same(knn_ref.topk(cross_ref.distances("f32", q, t), 2), oracle.knn2(q, t))
    q, t = float_ref.collision_fixture(dim)
    got = knn_ref.topk(cross_ref.distances("f32", q, t), 2)
    _same(got, oracle.knn2(q, t))
    assert got[0].tolist() == [[0, 1]]
    _same(knn_ref.topk(cross_ref.distances("f32", q, t[:1]), 2), oracle.knn2(q, t[:1]))


@pytest.mark.parametrize("width", [16, 32, 61])
def test_k2_equals_hamming_ref_knn2(width):
    rng = np.random.default_rng(width)
    q = rng.integers(0, 256, size=(50, width), dtype=np.uint8)
    t = rng.integers(0, 256, size=(130, width), dtype=np.uint8)
    t[::7] = t[0]
    _same(knn_ref.topk(cross_ref.distances("bin", q, t), 2), hamming_ref.knn2(q, t))
    _same(knn_ref.topk(cross_ref.distances("bin", q, t[:1]), 2), hamming_ref.knn2(q, t[:1]))
