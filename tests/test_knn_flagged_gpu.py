"""GPU parity of 128-D sets with non-integer rows in every distance mode (csrc/knn.hip, csrc/radius.hip, csrc/api.cpp).

prep_tile raises a set's flags word when a value is not an integer in [0, 255]; every later kernel reads the flags
of a problem's two sets and decides per block who answers (knn2_i8_kernel and knn2_rescan_kernel skip a flagged
problem, knn2_f32_kernel takes it; the radius kernels split the same way; cross-check swaps the sides).  The host
never knows which kernel answered, so a wrong classification gives plausible numbers and no error.  Here:

1. integer, jittered and single-value sets on either side of the problems of one fused batch, in every mode
   (verdict, ratio, exact) and under every schedule knob: records byte-equal across the environments and equal to
   the oracle's, an integer problem still in verdict mode beside flagged neighbours;
2. one altered value in an otherwise integer set, at the positions prep_tile's lanes and passes read, with the
   values either side of the classification's boundary;
3. cross-check, top-k and radius with an integer and a jittered side in both orders;
4. flags blocks released by mim_sets_truncate and reused by sets of the other kind.

Zero tolerance throughout: integer rows give the oracle's bits on either kernel (tests/test_flagged_inputs.py holds
the CPU side: the cases differ from what a wrong classification would compute).
"""
import os

import numpy as np
import pytest

import cross_ref as X
import flagged_inputs as FI
import knn_ref
import radius_ref

pytestmark = pytest.mark.gpu

KNOBS = ("MIM_KNN_DYN", "MIM_KNN_FLIP", "MIM_KNN_RATIO", "MIM_KNN_TAIL", "MIM_KNN_SUB")
# (environment, knn_mode at a ratio below 1): 2 verdict, 1 ratio, 0 exact.  600 x 1500 is far fewer sweeps than
# resident blocks, so without MIM_KNN_DYN the schedule is the static one (several splits: the ratio mode), and
# MIM_KNN_TAIL finds no partly filled last round to cut.
ENVS = [({"MIM_KNN_DYN": "1"}, (2,)),
        ({"MIM_KNN_DYN": "1", "MIM_KNN_FLIP": "0"}, (1,)),
        ({"MIM_KNN_DYN": "1", "MIM_KNN_RATIO": "0"}, (0,)),
        ({"MIM_KNN_DYN": "0"}, (1,)),
        ({"MIM_KNN_DYN": "1", "MIM_KNN_TAIL": "1"}, (1, 2)),
        ({"MIM_KNN_SUB": "0"}, (1,)),
        ({"MIM_KNN_SUB": "16"}, (1,)),
        ({"MIM_KNN_SUB": "64"}, (1,))]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _run(m, problems, ratio, env, filter="ratio", max_iters=FI.MAX_ITERS):
    """One batch under the knobs of `env` alone (read per launch), the process environment restored after."""
    from computervision_objectdetection_featurematching_amd import default_params
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        res = m.match_batch(problems, default_params(ratio=ratio, max_iters=max_iters), filter=filter)
        det = [m.problem_detail(i, int(r["n_good"])) for i, r in enumerate(res)]
        mode = int(m.kernel_ms("knn_mode"))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, det, mode


def _same(new, ref, what):
    assert new[0].tobytes() == ref[0].tobytes(), f"records differ ({what})"
    for i, (a, b) in enumerate(zip(new[1], ref[1])):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg=f"problem {i} {what}")


def _vs_oracle(r, det, o, what):
    """The fields test_ransac_gpu._batch_vs_oracle compares, H to the bit."""
    gq, gt, gm = det
    assert r["n_good"] == o["n_good"], what
    np.testing.assert_array_equal(gq, o["good_q"], err_msg=str(what))
    np.testing.assert_array_equal(gt, o["good_t"], err_msg=str(what))
    assert r["status"] == o["status"], (what, r["status"], o["status"])
    assert r["n_inl"] == o["n_inl"], what
    if o["n_good"] > 4:
        assert r["iters"] == o["iters"], what
        np.testing.assert_array_equal(gm, o["mask"], err_msg=str(what))
    if o["status"] != 2 and o["n_good"] >= 4:
        Hg, Ho = r["H"].reshape(3, 3), o["H"]
        assert np.max(np.abs(Hg - Ho) / (np.abs(Ho) + 1e-3)) <= 0.0, (what, Hg, Ho)


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own with every set of the batch registered: (matcher, name -> set id)."""
    from computervision_objectdetection_featurematching_amd import Matcher, build
    build.build()
    m = Matcher(0)
    ids = {name: m.add_set(d, k) for name, (d, k) in FI.sets().items()}
    yield m, ids
    m.close()


_oracle_records = {}


def _expected(oracle, ratio):
    """The oracle's records of the nine problems at `ratio`, computed once per process and shared."""
    if ratio not in _oracle_records:
        S = FI.sets()
        prm = oracle.default_params(ratio=ratio, max_iters=FI.MAX_ITERS)
        _oracle_records[ratio] = [oracle.match_problem(*S[a], *S[b], prm) for a, b in FI.PROBLEMS]
    return _oracle_records[ratio]


# ---- 1. the batch path, every mode and schedule ------------------------------------------------------------
@pytest.mark.parametrize("ratio", FI.RATIOS)
def test_batch_every_mode_and_schedule(ctx, oracle, ratio):
    m, ids = ctx
    problems = [(ids[a], ids[b]) for a, b in FI.PROBLEMS]
    runs = []
    for env, modes in ENVS:
        runs.append(_run(m, problems, ratio, env))
        # one launch serves the batch: the integer problem runs in this mode beside its flagged neighbours
        assert runs[-1][2] in (modes if ratio < 1 else (0,)), (env, runs[-1][2])
    for (env, _), run in zip(ENVS[1:], runs[1:]):
        _same(run, runs[0], f"{env} against {ENVS[0][0]}, ratio {ratio}")
    res, det, _ = runs[0]
    exp = _expected(oracle, ratio)
    for i, o in enumerate(exp):
        _vs_oracle(res[i], det[i], o, (FI.PROBLEMS[i], ratio))
    # a single altered value moves nothing for the queries it is not a neighbour of (the subset is the oracle's)
    S = FI.sets()
    row = FI.T1_POS[0]
    near = [oracle.knn2(S["QI"][0], S[t][0])[0] for t in ("TI", "T1")]
    keep_t1 = ~((near[0] == row).any(axis=1) | (near[1] == row).any(axis=1))
    keep_q1 = np.arange(FI.NQ) != FI.Q1_POS[0]
    assert keep_t1.sum() > FI.NQ - 20
    base_q, base_t, _ = det[0]
    for i, keep in ((4, keep_t1), (5, keep_q1)):
        gq, gt, _ = det[i]
        np.testing.assert_array_equal(gq[keep[gq]], base_q[keep[base_q]], err_msg=str(FI.PROBLEMS[i]))
        np.testing.assert_array_equal(gt[keep[gq]], base_t[keep[base_q]], err_msg=str(FI.PROBLEMS[i]))
    if ratio < 1:
        assert exp[0]["n_good"] > 50 and exp[6]["n_good"] == 0


def test_sub_batch_in_either_order_equals_the_batch(ctx, oracle):
    """The four problems over the integer and the jittered sets, run twice in one context, the second time in
    reverse order: each record is its record of the nine-problem batch."""
    m, ids = ctx
    nine = _run(m, [(ids[a], ids[b]) for a, b in FI.PROBLEMS], 0.9, {"MIM_KNN_DYN": "1"})
    four = [(ids[a], ids[b]) for a, b in FI.SUB_BATCH]
    for order in (list(range(4)), list(range(4))[::-1]):
        res, det, _ = _run(m, [four[i] for i in order], 0.9, {})
        for pos, i in enumerate(order):
            assert res[pos].tobytes() == nine[0][i].tobytes(), (order, pos, res[pos], nine[0][i])
            for x, y in zip(det[pos], nine[1][i]):
                np.testing.assert_array_equal(x, y, err_msg=f"order {order} position {pos}")
    for i, o in enumerate(_expected(oracle, 0.9)[:4]):
        _vs_oracle(nine[0][i], nine[1][i], o, FI.PROBLEMS[i])


def test_knn_rows_of_the_registered_sets(ctx, oracle):
    """mim_knn2_sets_dev on the batch's own sets: the records above hold no distances, and the single values of T1
    and Q1 move only distance bits (tests/test_flagged_inputs.py: they do move them)."""
    import torch
    m, ids = ctx
    S = FI.sets()
    for a, b in FI.PROBLEMS:
        nq = len(S[a][0])
        idx = torch.full((nq, 2), -7, dtype=torch.int32, device="cuda")
        dist = torch.full((nq, 2), -7, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m.knn_sets_dev(ids[a], ids[b], idx, dist)
        m.synchronize()
        oi, od = oracle.knn2(S[a][0], S[b][0])
        np.testing.assert_array_equal(idx.cpu().numpy(), oi, err_msg=f"{a} {b}")
        np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(od), err_msg=f"{a} {b}")


# ---- 2. the classification boundary ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FI.VALUES))
def test_single_value_at_every_position(matcher, oracle, name):
    """One value of an otherwise integer set: mim_knn2_l2 (the device classifies) gives the oracle's rows, and so
    does mim_knn2_l2_f32 (generic float sets: no classification), bit for bit."""
    for side, r, c in FI.boundary_cases():
        q, t = FI.altered(side, r, c, FI.VALUES[name])
        oi, od = oracle.knn2(q, t)
        gi, gd = matcher.knn_match_arrays(q, t)
        np.testing.assert_array_equal(gi, oi, err_msg=f"{name} in {side} at ({r}, {c})")
        np.testing.assert_array_equal(_bits(gd), _bits(od), err_msg=f"{name} in {side} at ({r}, {c})")
        fi, fd = matcher.knn_match_float_arrays(q, t)
        np.testing.assert_array_equal(fi, gi, err_msg=f"float entry, {name} in {side} at ({r}, {c})")
        np.testing.assert_array_equal(_bits(fd), _bits(gd), err_msg=f"float entry, {name} in {side} at ({r}, {c})")


# ---- 3. the other entries, an integer and a jittered side in both orders ------------------------------------
_mixed_d = {}


def _mixed_distances(a, b):
    if (a, b) not in _mixed_d:
        M = FI.mixed_sets()
        _mixed_d[a, b] = X.distances("f32", M[a], M[b])
    return _mixed_d[a, b]


def _register_mixed(matcher, a, b):
    M = FI.mixed_sets()
    matcher.clear_sets()
    kp = lambda n: np.zeros((n, 2), np.float32)
    return matcher.add_set(M[a], kp(FI.M_NQ)), matcher.add_set(M[b], kp(FI.M_NT))


@pytest.mark.parametrize("a,b", FI.MIXED_PAIRS)
def test_cross_sets_mixed(matcher, a, b):
    qs, ts = _register_mixed(matcher, a, b)
    try:
        idx, dist = matcher.match_cross_sets(qs, ts)
    finally:
        matcher.clear_sets()
    want = X.mutual(_mixed_distances(a, b))
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(_bits(dist), _bits(want[1]))
    assert (idx >= 0).sum() >= 100


@pytest.mark.parametrize("k", [1, 2, 3, 16])
@pytest.mark.parametrize("a,b", FI.MIXED_PAIRS)
def test_topk_mixed(matcher, a, b, k):
    M = FI.mixed_sets()
    idx, dist = matcher.knn_match_arrays(M[a], M[b], k)
    want = knn_ref.topk(_mixed_distances(a, b), k)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(_bits(dist), _bits(want[1]))


@pytest.mark.parametrize("a,b", FI.MIXED_PAIRS)
def test_radius_sets_mixed(matcher, a, b):
    """("QR", "TI") is the direction tests/test_radius_gpu.py lacks; the other one rides along."""
    from test_radius_gpu import _radii
    d = _mixed_distances(a, b)
    qs, ts = _register_mixed(matcher, a, b)
    try:
        for r in _radii(d):
            got = matcher.radius_sets(qs, ts, r)
            matcher.synchronize()
            go, gi, gd = (x.cpu().numpy() for x in got)
            eo, ei, ed = radius_ref.radius(d, r)
            np.testing.assert_array_equal(go, eo, err_msg=f"radius {r!r}")
            np.testing.assert_array_equal(gi, ei, err_msg=f"radius {r!r}")
            np.testing.assert_array_equal(_bits(gd), _bits(ed), err_msg=f"radius {r!r}")
    finally:
        matcher.clear_sets()


_batch_d = {}  # (query rows, train rows) of FI.sets() by address -> distance matrix (the arrays live as long)


@pytest.mark.parametrize("filter", [X.FILTER_CROSS, X.FILTER_RATIO_CROSS])
def test_batch_cross_filters_mixed(ctx, oracle, monkeypatch, filter):
    """The four-problem sub-batch under the cross-check filters: the shadow of (QI, TR) is (TR, QI), so each flagged
    set is read from both sides in one launch."""
    m, ids = ctx
    S = FI.sets()
    distances = X.distances

    def shared(kind, q, t, chunk=128):  # one distance matrix per problem for both filters
        key = (q.ctypes.data, t.ctypes.data)
        if key not in _batch_d:
            _batch_d[key] = distances(kind, q, t, chunk)
        return _batch_d[key]

    monkeypatch.setattr(X, "distances", shared)
    res, det, mode = _run(m, [(ids[a], ids[b]) for a, b in FI.SUB_BATCH], 0.9, {}, filter=X.FILTER_NAMES[filter])
    assert mode == 0 and int(m.kernel_ms("knn_cross")) == 1
    accepted = 0
    for i, (a, b) in enumerate(FI.SUB_BATCH):
        e = X.expected_problem(oracle, "f32", *S[a], *S[b], filter, FI.MAX_ITERS)
        r, (gq, gt, gm) = res[i], det[i]
        assert int(r["n_good"]) == e["n_good"], (a, b)
        np.testing.assert_array_equal(gq, e["good_q"])
        np.testing.assert_array_equal(gt, e["good_t"])
        assert (int(r["status"]), int(r["n_inl"])) == (e["status"], e["n_inl"]), (a, b, r, e)
        if e["n_good"] >= 4:
            np.testing.assert_array_equal(gm, e["mask"])
        if e["H"] is not None:
            np.testing.assert_array_equal(r["H"].view(np.int64), e["H"].reshape(9).view(np.int64))
        if e["iters"] is not None:
            assert int(r["iters"]) == e["iters"], (a, b)
        accepted += e["status"] == X.MIM_ACCEPTED
    assert accepted >= 3


# ---- 4. flags across truncate -----------------------------------------------------------------------------
def test_flags_across_truncate(oracle):
    """Flags blocks come from the arena and go back to it: sets of the other kind registered where the dropped
    ones stood read their own classification, not the previous one's."""
    from computervision_objectdetection_featurematching_amd import Matcher
    S = FI.sets()
    exp = {p: o for p, o in zip(FI.PROBLEMS, _expected(oracle, 0.9))}
    m = Matcher(0)
    try:
        def run(pairs, names):
            res, det, _ = _run(m, pairs, 0.9, {})
            for i, p in enumerate(names):
                _vs_oracle(res[i], det[i], exp[p], (p, names))
            return {p: (res[i].tobytes(), det[i]) for i, p in enumerate(names)}

        qi, ti, tr = m.add_set(*S["QI"]), m.add_set(*S["TI"]), m.add_set(*S["TR"])  # one flush, at the first batch
        first = run([(qi, ti), (qi, tr)], [("QI", "TI"), ("QI", "TR")])
        m.truncate_sets(1)
        tr2, ti2 = m.add_set(*S["TR"]), m.add_set(*S["TI"])  # the kinds swapped in the same slots
        assert (tr2, ti2) == (ti, tr)
        second = run([(qi, ti2), (qi, tr2)], [("QI", "TI"), ("QI", "TR")])
        for p in first:
            assert first[p][0] == second[p][0], p
            for x, y in zip(first[p][1], second[p][1]):
                np.testing.assert_array_equal(x, y, err_msg=str(p))
        m.truncate_sets(1)
        t1 = m.add_set(*S["T1"])
        assert t1 == ti
        run([(qi, t1)], [("QI", "T1")])
    finally:
        m.close()
