"""The private sets of the host-buffer entries (mim_knn2_l2, mim_knn2_hamming, mim_knn2_l2_f32, mim_knn_l2,
mim_knn_hamming, mim_radius_l2, mim_radius_hamming) interleaved with registered sets: every entry appends two sets,
runs and drops them again (api.cpp with_private_sets), on success and on every failure.  The caller's sets keep
their ids, mim_sets_info keeps its count and generation, pending preps of the caller's sets survive, and a batch on
the caller's sets gives the records of a context that never made a host-buffer call, byte for byte.

Shapes: nq = 70, nt = 130 (more than one 64-row tile, not a multiple of one); 128-D rows integer-valued (the i8
path), binary rows of 32 bytes, generic float rows of dim 7.  Expected values: float_ref.knn2 / hamming_ref.knn2 at
k = 2, knn_ref.topk at k = 3, radius_ref.radius, on the distance matrices of float_ref.l2sqr and
hamming_ref.distances."""
import ctypes as C

import numpy as np
import pytest

import float_ref as F
import hamming_ref as H
import knn_ref as K
import radius_ref as R
from computervision_objectdetection_featurematching_amd import Matcher, _lib, default_params
from computervision_objectdetection_featurematching_amd._lib import MimError
from computervision_objectdetection_featurematching_amd.synthetic import make_dataset, orb_like, sift_like

pytestmark = pytest.mark.gpu

NQ, NT = 70, 130
PRM = default_params(max_iters=2000)
DS = make_dataset(1, 2, 300, 600, 120, inlier_frac=0.3, seed=4242)  # the caller's sets: model 0, scenes 0 and 1
_rng = np.random.default_rng(20240)
SQ, ST = sift_like(_rng, NQ), sift_like(_rng, NT)
BQ, BT = orb_like(_rng, NQ, 32), orb_like(_rng, NT, 32)
FQ, FT = F.normal_rows(_rng, NQ, 7), F.normal_rows(_rng, NT, 7)
with np.errstate(over="ignore", under="ignore"):
    D_SIFT, D_F7 = np.sqrt(F.l2sqr(SQ, ST)), np.sqrt(F.l2sqr(FQ, FT))
D_BIN = H.distances(BQ, BT).astype(np.float32)
# radii from the inputs' own distance matrices: about a tenth of the pairs, none empty
R_SIFT, R_F7, R_BIN = (float(np.float32(np.quantile(d, 0.1))) for d in (D_SIFT, D_F7, D_BIN))


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype
        np.testing.assert_array_equal(g, e)
        if g.dtype == np.float32:
            np.testing.assert_array_equal(g.view(np.int32), e.view(np.int32))


# (entry, call on a Matcher, expected): the seven entries, mim_radius_l2 at dim 128 and at dim 7
HOST_CALLS = [
    ("mim_knn2_l2", lambda m: m.knn_match_arrays(SQ, ST, 2), lambda: F.knn2(SQ, ST)),
    ("mim_knn2_hamming", lambda m: m.knn_match_hamming_arrays(BQ, BT, 2), lambda: H.knn2(BQ, BT)),
    ("mim_knn2_l2_f32", lambda m: m.knn_match_float_arrays(FQ, FT, 2), lambda: F.knn2(FQ, FT)),
    ("mim_knn_l2", lambda m: m.knn_match_float_arrays(FQ, FT, 3), lambda: K.topk(D_F7, 3)),
    ("mim_knn_hamming", lambda m: m.knn_match_hamming_arrays(BQ, BT, 3), lambda: K.topk(D_BIN, 3)),
    ("mim_radius_l2 dim 128", lambda m: m.radius_match_arrays(SQ, ST, R_SIFT), lambda: R.radius(D_SIFT, R_SIFT)),
    ("mim_radius_l2 dim 7", lambda m: m.radius_match_float_arrays(FQ, FT, R_F7), lambda: R.radius(D_F7, R_F7)),
    ("mim_radius_hamming", lambda m: m.radius_match_hamming_arrays(BQ, BT, R_BIN), lambda: R.radius(D_BIN, R_BIN)),
]


def _register(m):
    assert m.add_set(DS.model_desc[0], DS.model_kp[0]) == 0
    assert m.add_set(DS.scene_desc[0], DS.scene_kp[0]) == 1


def _batch(m, pair):
    res = m.match_batch([pair], PRM).copy()
    return res, m.problem_detail(0, int(res[0]["n_good"]))


def _same_batch(got, exp):
    assert got[0].tobytes() == exp[0].tobytes()
    for g, e in zip(got[1], exp[1]):
        assert g.tobytes() == e.tobytes()


@pytest.fixture(scope="module")
def expected(matcher):
    """The host entries' reference results, and the batches of a context that made no host-buffer call."""
    m = Matcher(0)
    try:
        _register(m)
        b01 = _batch(m, (0, 1))
        assert m.add_set(DS.scene_desc[1], DS.scene_kp[1]) == 2
        b02 = _batch(m, (0, 2))
    finally:
        m.close()
    assert int(b01[0][0]["n_good"]) > 4 and int(b02[0][0]["n_good"]) > 4  # the batches have something to compare
    return {"host": [exp() for _, _, exp in HOST_CALLS], (0, 1): b01, (0, 2): b02}


def _host_calls_keep_the_sets(m, expected):
    for (name, call, _), exp in zip(HOST_CALLS, expected["host"]):
        before = m.sets_info()
        got = call(m)
        assert m.sets_info() == before, name
        _same(got, exp)


def test_interleaved_with_pending_preps(expected):
    m = Matcher(0)
    try:
        _register(m)  # no batch yet: the two sets' prep is pending
        _host_calls_keep_the_sets(m, expected)
        _same_batch(_batch(m, (0, 1)), expected[(0, 1)])
    finally:
        m.close()


def test_interleaved_after_a_batch(expected):
    m = Matcher(0)
    try:
        _register(m)
        _same_batch(_batch(m, (0, 1)), expected[(0, 1)])  # no prep pending: the private sets' storage goes back
        _host_calls_keep_the_sets(m, expected)
        assert m.add_set(DS.scene_desc[1], DS.scene_kp[1]) == 2
        _same_batch(_batch(m, (0, 2)), expected[(0, 2)])
    finally:
        m.close()


def _radius_cap_one_short(m):
    total = int(R.radius(D_SIFT, R_SIFT)[0][-1])
    assert total > 1
    off = np.zeros(NQ + 1, np.int64)
    idx, dist = np.zeros(total, np.int32), np.zeros(total, np.float32)
    m._check(m.L.mim_radius_l2(m.ctx, C.c_void_p(SQ.ctypes.data), NQ, C.c_void_p(ST.ctypes.data), NT, 128, R_SIFT,
                               C.c_void_p(off.ctypes.data), C.c_void_p(idx.ctypes.data),
                               C.c_void_p(dist.ctypes.data), total - 1))


BIG = 2 ** 18  # train rows: OpenCV's limit, rejected by the problem check after both private sets exist
FAILURES = {
    "knn2_hamming_2^18": (lambda m: m.knn_match_hamming_arrays(BQ[:, :1], np.zeros((BIG, 1), np.uint8), 2),
                          _lib.MIM_EINVAL, "2^18 limit"),
    "knn2_l2_f32_2^18": (lambda m: m.knn_match_float_arrays(FQ[:, :1], np.zeros((BIG, 1), np.float32), 2),
                         _lib.MIM_EINVAL, "2^18 limit"),
    "knn2_l2_2^18": (lambda m: m.knn_match_arrays(SQ, np.zeros((BIG, 128), np.float32), 2), _lib.MIM_EINVAL,
                     "2^18 limit"),
    "radius_l2_cap": (_radius_cap_one_short, _lib.MIM_ERANGE, "room for"),
}


@pytest.mark.parametrize("case", list(FAILURES))
def test_failure_leaves_nothing_behind(expected, case):
    call, code, text = FAILURES[case]
    m = Matcher(0)
    try:
        _register(m)
        before = m.sets_info()
        with pytest.raises(MimError) as err:
            call(m)
        assert err.value.code == code and text in str(err.value)  # the rejection meant, not another
        assert m.sets_info() == before
        assert m.add_set(DS.scene_desc[1], DS.scene_kp[1]) == 2
        _same_batch(_batch(m, (0, 1)), expected[(0, 1)])
    finally:
        m.close()
