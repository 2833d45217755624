"""Pins tests/hamming_ref.py, the CPU yardstick of the Hamming kNN (BFMatcher(NORM_HAMMING), k = 2)."""
import numpy as np

import hamming_ref as R


def test_known_popcounts():
    assert [int(R.POPCOUNT[v]) for v in (0, 1, 2, 3, 0x0F, 0x55, 0x80, 0xFE, 0xFF)] == [0, 1, 1, 2, 4, 4, 1, 7, 8]
    q = np.array([[0x00, 0xFF, 0x0F, 0x01]], np.uint8)
    t = np.array([[0xFF, 0xFF, 0xF0, 0x00], [0x00, 0xFF, 0x0F, 0x01], [0x01, 0xFE, 0x0F, 0x03]], np.uint8)
    np.testing.assert_array_equal(R.distances(q, t), [[8 + 0 + 8 + 1, 0, 1 + 1 + 0 + 1]])
    idx, dist = R.knn2(q, t)
    np.testing.assert_array_equal(idx, [[1, 2]])
    np.testing.assert_array_equal(dist, np.array([[0, 3]], np.float32))
    assert dist.dtype == np.float32 and idx.dtype == np.int32


def test_zeros_against_ones():
    for width in (1, 16, 31, 32, 61, 64):
        d = R.distances(np.zeros((1, width), np.uint8), np.full((1, width), 0xFF, np.uint8))
        assert d.shape == (1, 1) and int(d[0, 0]) == 8 * width


def test_duplicate_train_row_keeps_lower_index():
    rng = np.random.default_rng(1)
    t = rng.integers(0, 256, size=(50, 32), dtype=np.uint8)
    t[40] = t[9]
    t[30] = t[9]
    idx, dist = R.knn2(t[[9, 40]], t, chunk=1)
    np.testing.assert_array_equal(idx, [[9, 30], [9, 30]])
    np.testing.assert_array_equal(dist, np.zeros((2, 2), np.float32))


def test_short_train_sets():
    q = np.zeros((3, 8), np.uint8)
    idx, dist = R.knn2(q, np.zeros((0, 8), np.uint8))
    assert (idx == -1).all() and (dist == R.FLT_MAX).all()
    idx, dist = R.knn2(q, np.full((1, 8), 1, np.uint8))
    np.testing.assert_array_equal(idx, [[0, -1]] * 3)
    np.testing.assert_array_equal(dist, np.array([[8, R.FLT_MAX]] * 3, np.float32))
    idx, dist = R.knn2(np.zeros((0, 8), np.uint8), np.zeros((5, 8), np.uint8))
    assert idx.shape == (0, 2) and dist.shape == (0, 2)
