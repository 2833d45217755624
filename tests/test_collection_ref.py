"""tests/collection_ref.py against itself and against knn_ref: the vectorised (distance, imgIdx,
trainIdx) rule equals OpenCV's per-image insertion with `update`, one image is plain knnMatch, and cutting the
collection into groups that are merged one after another changes nothing."""
import numpy as np
import pytest

import collection_ref as CR
import knn_ref as K

FLT_MAX = CR.FLT_MAX


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))


def _collection(rng, nq, sizes, levels):
    """Heavily tied distances (a few levels), with never-inserted values (FLT_MAX, inf, NaN) among them."""
    out = []
    for nt in sizes:
        d = rng.integers(0, levels, size=(nq, nt)).astype(np.float32) * np.float32(0.37)
        bad = rng.random((nq, nt)) < 0.1
        d[bad] = rng.choice(np.array([FLT_MAX, np.inf, np.nan], np.float32), size=int(bad.sum()))
        out.append(d)
    return out


def _cases():
    rng = np.random.default_rng(18)
    cases = []
    for c in range(300):
        n_img = int(rng.integers(1, 7))
        sizes = [int(rng.choice([0, 0, 1, 2, 3, 5, 9, 17])) for _ in range(n_img)]  # empty images, fewer than k rows
        cases.append((_collection(rng, int(rng.integers(1, 4)), sizes, int(rng.integers(1, 5))), int(rng.integers(1, 17))))
    return cases


def test_vectorised_rule_equals_the_update_loop():
    empty = short = never = 0
    for dists, k in _cases():
        got = CR.topk_collection(dists, k)
        _same(got, CR.update_loop(dists, k))
        empty += any(d.shape[1] == 0 for d in dists)
        short += sum(d.shape[1] for d in dists) < k
        never += bool((got[0] == -1).any() and sum(d.shape[1] for d in dists) >= k)
        assert ((got[0] == -1) == (got[1] == -1)).all() and (got[2][got[0] == -1] == FLT_MAX).all()
    assert empty > 50 and short > 50 and never > 5  # the cases are there


def test_one_image_is_knn_match():
    rng = np.random.default_rng(1)
    for nt in (0, 1, 5, 40):
        d = _collection(rng, 6, [nt], 3)
        for k in (1, 2, 5, 16):
            idx, img, dist = CR.topk_collection(d, k)
            oi, od = K.topk(d[0], k)
            _same((idx, dist), (oi, od))
            assert ((img == 0) == (idx >= 0)).all()


def test_any_split_into_groups_gives_the_same_lists():
    rng = np.random.default_rng(2)
    for _ in range(40):
        n_img = int(rng.integers(2, 7))
        dists = _collection(rng, 3, [int(rng.choice([0, 1, 2, 4, 9])) for _ in range(n_img)], 3)
        k = int(rng.integers(1, 9))
        exp = CR.topk_collection(dists, k)
        for cuts in ([0, n_img], list(range(n_img + 1)), [0, 1, n_img], [0, n_img - 1, n_img]):
            _same(CR.merge_groups(dists, k, cuts), exp)


def test_image_index_breaks_ties_before_the_row():
    d = [np.array([[2, 1, 1]], np.float32), np.array([[1, 0]], np.float32), np.array([[0, 1]], np.float32)]
    idx, img, dist = CR.topk_collection(d, 6)
    assert list(zip(img[0], idx[0])) == [(1, 1), (2, 0), (0, 1), (0, 2), (1, 0), (2, 1)]
    assert dist[0].tolist() == [0, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("k", [1, 16])
def test_limits(k):
    assert CR.MAX_IMAGES << CR.IMG_SHIFT < 2**31 - 1 <= (CR.MAX_IMAGES + 1) << CR.IMG_SHIFT
    d = [np.zeros((1, 0), np.float32)] * 3
    idx, img, dist = CR.topk_collection(d, k)
    assert (idx == -1).all() and (img == -1).all() and (dist == FLT_MAX).all()
