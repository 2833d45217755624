"""The radiusMatch yardstick against itself (tests/radius_ref.py): the vectorised form equals the
literal push-then-sort form on heavily tied matrices with NaN, +inf and empty rows, and at r = +inf a finite
matrix gives every row's full stable order, whose first k columns are knnMatch's (knn_ref.topk)."""
import numpy as np
import pytest

import knn_ref as K
import radius_ref as R


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)


def _matrix(rng):
    nq, nt = int(rng.integers(0, 7)), int(rng.integers(0, 12))
    d = rng.integers(0, 4, size=(nq, nt)).astype(np.float32) * np.float32(0.37)  # four values: ties everywhere
    if d.size:
        d[rng.random(d.shape) < 0.1] = np.nan
        d[rng.random(d.shape) < 0.1] = np.inf
        if nq and rng.random() < 0.3:
            d[int(rng.integers(nq))] = 9.0  # a row no finite radius below 9 reaches
    return d


def test_vectorised_equals_literal():
    rng = np.random.default_rng(17)
    n_nan = n_inf = n_empty = 0
    for case in range(300):
        d = _matrix(rng)
        for r in (0.1, 0.37, 0.5, np.float32(0.37) * 2, 1.2, np.inf):
            got = R.radius(d, r)
            _same(got, R.radius_loop(d, r))
            off = got[0]
            assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(got[1]) == len(got[2])
            n_empty += int((np.diff(off) == 0).sum())
        n_nan += int(np.isnan(d).sum())
        n_inf += int(np.isinf(d).sum())
    assert n_nan > 100 and n_inf > 100 and n_empty > 100


def test_nan_never_and_inf_only_at_inf():
    d = np.array([[np.nan, np.inf, 1.0, 1.0, 0.5]], np.float32)
    off, idx, dist = R.radius(d, 3e38)
    assert list(idx) == [4, 2, 3] and list(off) == [0, 3]
    off, idx, dist = R.radius(d, np.inf)
    assert list(idx) == [4, 2, 3, 1] and np.isinf(dist[-1])
    off, idx, dist = R.radius(d, np.nan)  # the library rejects it; the compare itself passes nothing
    assert list(off) == [0, 0]


@pytest.mark.parametrize("nq,nt", [(1, 1), (5, 3), (9, 40)])
def test_infinite_radius_is_the_full_stable_order(nq, nt):
    rng = np.random.default_rng(nq * 100 + nt)
    d = rng.integers(0, 6, size=(nq, nt)).astype(np.float32)
    off, idx, dist = R.radius(d, np.inf)
    assert (off == np.arange(nq + 1) * nt).all()
    idx, dist = idx.reshape(nq, nt), dist.reshape(nq, nt)
    np.testing.assert_array_equal(idx, np.argsort(d, axis=1, kind="stable"))
    for k in range(1, min(nt, K.MAX_K) + 1):
        ki, kd = K.topk(d, k)
        np.testing.assert_array_equal(idx[:, :k], ki)
        np.testing.assert_array_equal(dist[:, :k], kd)
