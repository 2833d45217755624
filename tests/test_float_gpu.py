"""GPU parity of the generic-float path (mim_set_create_f32, mim_knn2_l2_f32, csrc/knn_float.hip):
BFMatcher(NORM_L2).knnMatch(k=2) on float rows of any dim and the fused batch on such sets, against
oracle.knn2 / orc_match_problem at the rows' dim (indices and distance bits equal)."""
import ctypes as C

import numpy as np
import pytest

import float_ref as F
import hamming_ref as HR
from computervision_objectdetection_featurematching_amd import _lib, default_params
from computervision_objectdetection_featurematching_amd.synthetic import make_dataset

pytestmark = pytest.mark.gpu


def _same(got, exp):
    gi, gd = got
    oi, od = exp
    assert gi.shape == oi.shape and gi.dtype == np.int32 and gd.dtype == np.float32
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.int32), od.view(np.int32))


def _check(matcher, oracle, q, t):
    got = matcher.knn_match_float_arrays(q, t)
    _same(got, oracle.knn2(q, t))
    return got


# 1. shapes at dim 128, non-integer rows ((700, 4100): 65 row units, which the schedule cuts into splits)
@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (5, 3), (333, 257), (2000, 2000), (700, 4100)])
def test_shapes_dim_128(matcher, oracle, nq, nt):
    rng = np.random.default_rng(nq * 7919 + nt)
    q, t = F.rootsift_like(rng, nq), F.rootsift_like(rng, nt)
    assert (t != np.rint(t)).any()
    _check(matcher, oracle, q, t)


# 2. dims: no full round, a tail only, a tail after full rounds, the resident and the streamed path
@pytest.mark.parametrize("dim", F.DIMS)
def test_dims(matcher, oracle, dim):
    rng = np.random.default_rng(dim)
    _check(matcher, oracle, F.normal_rows(rng, 300, dim), F.normal_rows(rng, 700, dim))


# 3. two d^2 one ulp apart share a sqrtf: OpenCV's strict < on the sqrt values keeps the lower index first
@pytest.mark.parametrize("dim", F.COLLISION_DIMS)
def test_sqrt_collision(matcher, oracle, dim):
    q, t = F.collision_fixture(dim)
    gi, gd = _check(matcher, oracle, q, t)
    assert tuple(gi[0]) == (0, 1) and gd[0, 0] == gd[0, 1] == np.float32(3.0000002)


# 4. ties
@pytest.mark.parametrize("dim", [64, 200])
def test_ties_lower_index(matcher, oracle, dim):
    rng = np.random.default_rng(5 + dim)
    t = F.normal_rows(rng, 300, dim)
    for j in (130, 200, 250):
        t[j] = t[17]
    # two distinct rows at one distance from the query: q +- e on one coordinate
    q1 = F.normal_rows(rng, 1, dim)[0]
    q1[3] = 1.0  # 1.5 and 0.5 are exact
    t[40], t[90] = q1, q1
    t[40, 3] += np.float32(0.5)
    t[90, 3] -= np.float32(0.5)
    gi, gd = _check(matcher, oracle, np.stack([t[17], q1, t[250]]), t)
    assert tuple(gi[0]) == (17, 130) and gd[0, 0] == 0 and gd[0, 1] == 0
    assert tuple(gi[1]) == (40, 90) and gd[1, 0] == gd[1, 1]
    dm = matcher.knn_match_float(np.stack([t[17]]), t)
    assert [(m.queryIdx, m.trainIdx, m.distance) for m in dm[0]] == [(0, 17, 0.0), (0, 130, 0.0)]


# 5. magnitudes: denormal squares; d^2 = +inf is never inserted (index -1)
def test_magnitudes(matcher, oracle):
    rng = np.random.default_rng(9)
    s = np.float32(1e-20)
    gi, gd = _check(matcher, oracle, F.normal_rows(rng, 70, 128) * s, F.normal_rows(rng, 200, 128) * s)
    assert (gi >= 0).all() and (gd > 0).all() and (gd < 1e-18).all()
    _check(matcher, oracle, F.normal_rows(rng, 70, 20) * s, F.normal_rows(rng, 200, 20) * s)
    q = F.normal_rows(rng, 70, 64)
    big = (np.float32(1e18) * F.normal_rows(rng, 90, 64)).astype(np.float32)    # finite d^2 ~ 1e38
    huge = (np.float32(3e19) * (1 + np.abs(F.normal_rows(rng, 90, 64)))).astype(np.float32)  # every square overflows
    _check(matcher, oracle, q, big)
    gi, _ = _check(matcher, oracle, q, huge)
    assert (gi == -1).all()
    one = huge.copy()
    one[50] = q[3]
    gi, gd = _check(matcher, oracle, q, one)
    assert (gi[:, 0] == 50).all() and (gi[:, 1] == -1).all() and gd[3, 0] == 0
    gi, _ = _check(matcher, oracle, q.repeat(4, axis=1), np.concatenate([one, big]).repeat(4, axis=1))  # dim 256
    assert (gi[:, 0] == 50).all() and (gi[:, 1] >= 90).all()


# 6. splits: one query block over 70,000 train rows must be cut along the train rows; 300 x 5000 is the
# batch shape class; the result does not depend on the split count
@pytest.mark.parametrize("nq,nt,dim", [(64, 70000, 64), (300, 5000, 128)])
def test_splits(matcher, oracle, nq, nt, dim):
    rng = np.random.default_rng(nt)
    t = F.normal_rows(rng, nt, dim)
    t[nt - 1] = t[3]  # a tie across the first and the last split
    q = F.normal_rows(rng, nq, dim)
    q[0] = t[3]
    gi, _ = _check(matcher, oracle, q, t)
    assert tuple(gi[0]) == (3, nt - 1)


def _knn_sets(matcher, qs, ts, nq):
    import torch
    idx = torch.full((max(nq, 1), 2), -7, dtype=torch.int32, device="cuda")
    dist = torch.zeros((max(nq, 1), 2), dtype=torch.float32, device="cuda")
    matcher.knn_sets_dev(qs, ts, idx, dist)
    matcher.synchronize()
    return idx.cpu().numpy()[:nq], dist.cpu().numpy()[:nq]


# 7. strided host rows (step > 4 dim) and device tensors equal the dense host result
@pytest.mark.parametrize("dim", [64, 129])
def test_strided_and_device_sets(matcher, oracle, dim):
    import torch
    rng = np.random.default_rng(77 + dim)
    qbuf, tbuf = F.normal_rows(rng, 210, dim + 5), F.normal_rows(rng, 777, dim + 5)
    q, t = qbuf[:, :dim], tbuf[:, :dim]
    assert q.strides[0] == 4 * (dim + 5)
    dense = matcher.knn_match_float_arrays(q, t)
    _same(dense, oracle.knn2(q, t))
    matcher.clear_sets()
    qs = matcher.add_float_set(q, np.zeros((210, 2), np.float32))
    ts = matcher.add_float_set(t, np.zeros((777, 2), np.float32))
    assert (qs, ts) == (0, 1) and matcher.sets_info()[0] == 2
    _same(_knn_sets(matcher, qs, ts, 210), dense)
    qd = matcher.add_float_set(torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.zeros((210, 2), device="cuda"))
    td = matcher.add_float_set(torch.from_numpy(tbuf).cuda()[:, :dim], torch.zeros((777, 2), device="cuda"))
    _same(_knn_sets(matcher, qd, td, 210), dense)
    matcher.clear_sets()


def _records(matcher, res, ids):
    return [(res[i].tobytes(), matcher.problem_detail(i, int(res[i]["n_good"]))) for i in ids]


def _records_equal(a, b):
    assert len(a) == len(b)
    for (ra, da), (rb, db) in zip(a, b):
        assert ra == rb
        for x, y in zip(da, db):
            np.testing.assert_array_equal(x, y)


# 8. integer SIFT-like rows registered both ways, as problems of one batch: identical records
def test_same_rows_both_kinds(matcher):
    ds = make_dataset(2, 2, 700, 1500, 120)
    prm = default_params(max_iters=2000)
    matcher.clear_sets()
    iq = [matcher.add_set(d, k) for d, k in zip(ds.model_desc, ds.model_kp)]
    it = [matcher.add_set(d, k) for d, k in zip(ds.scene_desc, ds.scene_kp)]
    fq = [matcher.add_float_set(d, k) for d, k in zip(ds.model_desc, ds.model_kp)]
    ft = [matcher.add_float_set(d, k) for d, k in zip(ds.scene_desc, ds.scene_kp)]
    probs = []
    for a, b in ds.problems:
        probs += [(iq[a], it[b]), (fq[a], ft[b])]
    res = matcher.match_batch(probs, prm)
    assert (res["status"] == HR.MIM_ACCEPTED).any()
    n = len(probs)
    _records_equal(_records(matcher, res, range(0, n, 2)), _records(matcher, res, range(1, n, 2)))
    matcher.clear_sets()


def _compare_records(matcher, res, first, exp):
    for j, e in enumerate(exp):
        i = first + j
        r = res[i]
        assert int(r["n_good"]) == e["n_good"], i
        gq, gt, gm = matcher.problem_detail(i, e["n_good"])
        np.testing.assert_array_equal(gq, e["good_q"])
        np.testing.assert_array_equal(gt, e["good_t"])
        assert (int(r["status"]), int(r["n_inl"])) == (e["status"], e["n_inl"]), (i, r, e)
        if e["n_good"] > 4:
            assert int(r["iters"]) == e["iters"], i
        if e["n_good"] >= 4:
            np.testing.assert_array_equal(gm, e["mask"])
        if e["status"] != HR.MIM_EMPTY_H and e["n_good"] >= 4:
            np.testing.assert_array_equal(r["H"].view(np.int64), e["H"].view(np.int64))


def _register_float(matcher, qsets, tsets):
    return [matcher.add_float_set(d, k) for d, k in qsets], [matcher.add_float_set(d, k) for d, k in tsets]


# 9. the full path on the planted batch, at a resident and a streamed dim
@pytest.mark.parametrize("dim", [64, 256])
def test_full_path_planted_batch(matcher, oracle, dim):
    qsets, tsets, problems = F.planted_batch(dim)
    exp = F.expected_batch(oracle, dim)
    matcher.clear_sets()
    q, t = _register_float(matcher, qsets, tsets)
    res = matcher.match_batch([(q[a], t[b]) for a, b in problems], default_params(max_iters=F.MAX_ITERS))
    _compare_records(matcher, res, 0, exp)
    assert (res["status"] == HR.MIM_ACCEPTED).sum() >= 4
    scales = np.array([1.0 if i % 2 else 0.7 for i in range(len(problems))], np.float32)
    offs, pts = matcher.batch_inlier_points(len(problems), scales)
    for i, ((a, b), e) in enumerate(zip(problems, exp)):
        want = np.zeros((0, 2), np.float32)
        if e["status"] == HR.MIM_ACCEPTED:
            want = tsets[b][1][e["good_t"][e["mask"] != 0]]
            if scales[i] != 1.0:
                want = want / scales[i]
        np.testing.assert_array_equal(pts[offs[i]:offs[i + 1]].view(np.int32), want.astype(np.float32).view(np.int32))
    matcher.clear_sets()


# 10. i8, binary and generic-float problems in one batch equal each alone
def test_mixed_batch(matcher, oracle):
    prm = default_params(max_iters=F.MAX_ITERS)
    ds = make_dataset(2, 2, 700, 1500, 120)
    bq_sets, bt_sets, bproblems = HR.planted_batch()
    fq_sets, ft_sets, fproblems = F.planted_batch(64)
    matcher.clear_sets()
    iq = [matcher.add_set(d, k) for d, k in zip(ds.model_desc, ds.model_kp)]
    it = [matcher.add_set(d, k) for d, k in zip(ds.scene_desc, ds.scene_kp)]
    bq = [matcher.add_binary_set(d, k) for d, k in bq_sets]
    bt = [matcher.add_binary_set(d, k) for d, k in bt_sets]
    fq, ft = _register_float(matcher, fq_sets, ft_sets)
    lists = {"i": [(iq[a], it[b]) for a, b in ds.problems], "b": [(bq[a], bt[b]) for a, b in bproblems[:5]],
             "f": [(fq[a], ft[b]) for a, b in fproblems]}
    alone = {}
    for kind, probs in lists.items():
        res = matcher.match_batch(probs, prm)
        alone[kind] = _records(matcher, res, range(len(probs)))
    _compare_records(matcher, matcher.match_batch(lists["f"], prm), 0, F.expected_batch(oracle, 64))
    mixed, where = [], []
    for i in range(max(len(v) for v in lists.values())):
        for kind in ("f", "i", "b"):
            if i < len(lists[kind]):
                where.append((kind, i))
                mixed.append(lists[kind][i])
    res = matcher.match_batch(mixed, prm)
    got = _records(matcher, res, range(len(mixed)))
    for pos, (kind, i) in enumerate(where):
        _records_equal([got[pos]], [alone[kind][i]])
    matcher.clear_sets()


# 11. empty inputs, as mim_knn2_l2: no rows for an empty query; index -1 and the distance that call writes
@pytest.mark.parametrize("dim", [64, 200])
def test_empty_inputs(matcher, oracle, dim):
    rng = np.random.default_rng(8)
    q = F.normal_rows(rng, 9, dim)
    gi, gd = _check(matcher, oracle, q, np.zeros((0, dim), np.float32))
    li, ld = matcher.knn_match_arrays(np.zeros((9, 128), np.float32), np.zeros((0, 128), np.float32))
    np.testing.assert_array_equal(gi, li)
    np.testing.assert_array_equal(gd.view(np.int32), ld.view(np.int32))
    gi, gd = matcher.knn_match_float_arrays(np.zeros((0, dim), np.float32), q)
    assert gi.shape == (0, 2) and gd.shape == (0, 2)
    assert matcher.knn_match_float(np.zeros((0, dim), np.float32), q) == []
    # empty sets in a batch: no good matches
    matcher.clear_sets()
    e = matcher.add_float_set(np.zeros((0, dim), np.float32), np.zeros((0, 2), np.float32))
    s = matcher.add_float_set(q, np.zeros((9, 2), np.float32))
    res = matcher.match_batch([(e, s), (s, e)], default_params())
    assert [int(r["n_good"]) for r in res] == [0, 0] and [int(r["status"]) for r in res] == [HR.MIM_FEW_GOOD] * 2
    matcher.clear_sets()


# ---- 12. errors: MIM_EINVAL, the ctx usable afterwards, the next call correct --------------------------
def _einval(matcher, st):
    assert st == _lib.MIM_EINVAL
    assert matcher.L.mim_last_error(matcher.ctx).decode() != ""


def _still_works(matcher, oracle):
    rng = np.random.default_rng(99)
    _check(matcher, oracle, F.normal_rows(rng, 70, 33), F.normal_rows(rng, 150, 33))


@pytest.mark.parametrize("case", ["dim0", "dim513", "step_short", "step_odd"])
def test_set_create_f32_errors(matcher, oracle, case):
    matcher.clear_sets()
    rows = np.zeros((10, 600), np.float32)
    kp = np.zeros((10, 2), np.float32)
    dim, step = {"dim0": (0, 2400), "dim513": (513, 2400), "step_short": (64, 252), "step_odd": (64, 258)}[case]
    sid = C.c_int32(-1)
    st = matcher.L.mim_set_create_f32(matcher.ctx, C.c_void_p(rows.ctypes.data), step, C.c_void_p(kp.ctypes.data), 10,
                                      dim, 0, C.byref(sid))
    _einval(matcher, st)
    assert matcher.sets_info()[0] == 0
    if case.startswith("dim"):
        idx, dist = np.zeros((10, 2), np.int32), np.zeros((10, 2), np.float32)
        st = matcher.L.mim_knn2_l2_f32(matcher.ctx, C.c_void_p(rows.ctypes.data), 10, C.c_void_p(rows.ctypes.data), 10,
                                       dim, C.c_void_p(idx.ctypes.data), C.c_void_p(dist.ctypes.data))
        _einval(matcher, st)
    _still_works(matcher, oracle)
    matcher.clear_sets()


@pytest.mark.parametrize("case", ["generic_plain", "plain_generic", "dims", "bin_generic", "generic_bin"])
def test_problem_pairing_errors(matcher, oracle, case):
    from computervision_objectdetection_featurematching_amd.synthetic import orb_like
    rng = np.random.default_rng(31)
    matcher.clear_sets()
    kp = rng.uniform(0, 400, size=(40, 2)).astype(np.float32)
    g64 = matcher.add_float_set(F.normal_rows(rng, 40, 64), kp)
    g128 = matcher.add_float_set(F.normal_rows(rng, 40, 128), kp)
    plain = matcher.add_set(np.zeros((40, 128), np.float32), kp)
    b32 = matcher.add_binary_set(orb_like(rng, 40, 32), kp)
    pair = {"generic_plain": (g128, plain), "plain_generic": (plain, g128), "dims": (g64, g128),
            "bin_generic": (b32, g64), "generic_bin": (g64, b32)}[case]
    arr = np.array([(g64, g64), pair], np.int32)
    prm = default_params()
    st = matcher.L.mim_batch_run(matcher.ctx, arr.ctypes.data_as(C.POINTER(_lib.Problem)), 2, C.byref(prm))
    _einval(matcher, st)
    import torch
    idx = torch.zeros((40, 2), dtype=torch.int32, device="cuda")
    dist = torch.zeros((40, 2), dtype=torch.float32, device="cuda")
    st = matcher.L.mim_knn2_sets_dev(matcher.ctx, pair[0], pair[1], C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()))
    _einval(matcher, st)
    # the sets are still registered and usable
    res = matcher.match_batch([(g64, g64), (g128, g128)], prm)
    assert [int(r["n_good"]) for r in res] == [40, 40]  # every row finds itself at distance 0
    _still_works(matcher, oracle)
    matcher.clear_sets()


def test_set_rows_of_float_set(matcher, oracle):
    rng = np.random.default_rng(32)
    matcher.clear_sets()
    g = matcher.add_float_set(F.normal_rows(rng, 40, 128), np.zeros((40, 2), np.float32))
    n = C.c_int32()
    _einval(matcher, matcher.L.mim_set_rows(matcher.ctx, g, 0, None, None, C.byref(n)))
    _still_works(matcher, oracle)
    matcher.clear_sets()
