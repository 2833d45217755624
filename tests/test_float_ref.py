"""The summation order the generic-float kernel is written to, pinned on the CPU: tests/float_ref.py's numpy
float32 restatement (rounds, reduction, tail) against oracle.knn2, indices and distance bits equal."""
import numpy as np
import pytest

import float_ref as F


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("dim", F.DIMS)
def test_restatement_matches_oracle(oracle, dim):
    rng = np.random.default_rng(1000 + dim)
    q, t = F.normal_rows(rng, 40, dim), F.normal_rows(rng, 150, dim)
    t[77] = t[5]  # a tie
    q[0] = t[5]
    got = F.knn2(q, t)
    _same(got, oracle.knn2(q, t))
    assert tuple(got[0][0]) == (5, 77)


def test_restatement_rootsift_rows(oracle):
    rng = np.random.default_rng(7)
    q, t = F.rootsift_like(rng, 50), F.rootsift_like(rng, 300)
    assert (q != np.rint(q)).any()
    _same(F.knn2(q, t), oracle.knn2(q, t))


@pytest.mark.parametrize("dim", F.COLLISION_DIMS)
def test_sqrt_collision(oracle, dim):
    q, t = F.collision_fixture(dim)
    d2 = F.l2sqr(q, t)[0]
    nine = np.float32(9.0)
    assert d2[0] == np.nextafter(np.nextafter(nine, np.float32(10)), np.float32(10))
    assert d2[1] == np.nextafter(nine, np.float32(10)) and d2[2] > d2[0]
    oi, od = oracle.knn2(q, t)
    assert tuple(oi[0]) == (0, 1) and od[0, 0] == od[0, 1] == np.float32(3.0000002)
    _same(F.knn2(q, t), (oi, od))


def test_overflow_and_denormals(oracle):
    rng = np.random.default_rng(9)
    tiny_q, tiny_t = F.normal_rows(rng, 20, 100) * np.float32(1e-20), F.normal_rows(rng, 60, 100) * np.float32(1e-20)
    _same(F.knn2(tiny_q, tiny_t), oracle.knn2(tiny_q, tiny_t))
    q = F.normal_rows(rng, 20, 64)
    huge = (np.float32(3e19) * (1 + np.abs(F.normal_rows(rng, 30, 64)))).astype(np.float32)
    oi, od = oracle.knn2(q, huge)
    assert (oi == -1).all()
    _same(F.knn2(q, huge), (oi, od))
