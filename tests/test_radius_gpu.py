"""GPU parity of radiusMatch for every descriptor kind (mim_radius_count, mim_radius_fill_dev, mim_radius_l2,
mim_radius_hamming; csrc/radius.hip): offsets equal, indices equal and distance bits equal against
radius_ref.radius(cross_ref.distances(kind, q, t), r).  The semantics are recalled from OpenCV 4.5.4, which this
suite cannot call, so the yardstick itself is unpinned against it."""
import ctypes as C

import numpy as np
import pytest

import cross_ref as X
import float_ref as F
import radius_ref as R
from computervision_objectdetection_featurematching_amd import Matcher, _lib, default_params
from computervision_objectdetection_featurematching_amd._lib import MimError, Problem
from computervision_objectdetection_featurematching_amd.synthetic import orb_like, sift_like

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS = np.finfo(np.float32).eps
SHAPES = [(1, 1), (5, 3), (257, 129), (333, 700)]
KINDS = ["bin16", "bin32", "bin61", "bin64", "f32_7", "f32_64", "f32_128", "f32_200", "f32_512", "sift_int", "sift_real"]
MAX_D2 = 128 * 255 * 255


def _same(got, exp):
    go, gi, gd = got
    eo, ei, ed = exp
    assert go.dtype == np.int64 and gi.dtype == np.int32 and gd.dtype == np.float32
    np.testing.assert_array_equal(go, eo)
    np.testing.assert_array_equal(gi, ei)
    np.testing.assert_array_equal(gd.view(np.int32), ed.view(np.int32))


def _rows(kind, rng, n):
    if kind.startswith("bin"):
        return orb_like(rng, n, int(kind[3:]))
    if kind.startswith("f32_"):
        return F.normal_rows(rng, n, int(kind[4:]))
    return sift_like(rng, n) if kind == "sift_int" else F.rootsift_like(rng, n)


def _dist(kind, q, t, chunk=128):
    return X.distances("bin" if kind.startswith("bin") else "f32", q, t, chunk)


def _add(matcher, kind, rows):
    kp = np.zeros((len(rows), 2), np.float32)
    if kind.startswith("bin"):
        return matcher.add_binary_set(rows, kp)
    if kind.startswith("f32"):
        return matcher.add_float_set(rows, kp)
    return matcher.add_set(rows, kp)


def _host(matcher, q, t, r, cap=None, want_idx=True):
    """mim_radius_hamming (uint8 rows) / mim_radius_l2 (float rows) on host arrays: (status, offsets, idx, dist),
    the buffers of `cap` entries (default: every pair) prefilled with -7."""
    q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
    nq = q.shape[0]
    cap = nq * t.shape[0] if cap is None else cap
    off = np.full(nq + 1, -7, np.int64)
    idx = np.full(max(cap, 1), -7, np.int32)
    dist = np.full(max(cap, 1), -7, np.float32)
    fn = matcher.L.mim_radius_hamming if q.dtype == np.uint8 else matcher.L.mim_radius_l2
    st = fn(matcher.ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data), t.shape[0], q.shape[1], float(r),
            C.c_void_p(off.ctypes.data), C.c_void_p(idx.ctypes.data) if want_idx else None,
            C.c_void_p(dist.ctypes.data) if want_idx else None, cap)
    return st, off, idx, dist


def _host_ok(matcher, q, t, r):
    st, off, idx, dist = _host(matcher, q, t, r)
    matcher._check(st)
    return off, idx[:off[-1]], dist[:off[-1]]


def _np(triple):
    return tuple(x.cpu().numpy() for x in triple)


def _sets(matcher, qs, ts, r):
    got = matcher.radius_sets(qs, ts, r)
    matcher.synchronize()
    return _np(got)


def _run(matcher, kind, q, t, r):
    """The kind's own route: 128-D sets of mim_set_create through registered sets, the others through the host entries."""
    if not kind.startswith("sift"):
        return _host_ok(matcher, q, t, r)
    matcher.clear_sets()
    try:
        return _sets(matcher, _add(matcher, kind, q), _add(matcher, kind, t), r)
    finally:
        matcher.clear_sets()


def _radii(d):
    """An exact distance of the matrix (the <= boundary), its neighbour below, below every distance (every list
    empty), the 1 % quantile, above every distance (every pair)."""
    v = np.sort(d.ravel())
    assert v[0] > 2 * EPS and np.isfinite(v[-1])  # the fixed seeds give no zero distance
    exact = v[len(v) // 2]
    return [exact, np.nextafter(exact, f32(0)), np.nextafter(v[0], f32(0)), v[len(v) // 100], np.nextafter(v[-1], f32(np.inf))]


# 1. shapes x kinds x radii
@pytest.mark.parametrize("nq,nt", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_shapes(matcher, kind, nq, nt):
    rng = np.random.default_rng(KINDS.index(kind) * 1000 + nq + nt)
    q, t = _rows(kind, rng, nq), _rows(kind, rng, nt)
    if kind == "sift_real":
        assert (t != np.rint(t)).any()
    d = _dist(kind, q, t)
    sizes = []
    for r in _radii(d):
        exp = R.radius(d, r)
        _same(_run(matcher, kind, q, t, r), exp)
        sizes.append(int(exp[0][-1]))
    assert sizes[2] == 0 and sizes[4] == nq * nt and sizes[1] < sizes[0]


# a second i8 query block of one problem (512 queries to a block): its second wave has one valid column tile
# with one valid column, and the three train tiles take two stages
def test_second_query_block(matcher):
    test_shapes(matcher, "sift_int", 577, 129)


def test_host_entry_at_dim_128_takes_either_path(matcher):
    """mim_radius_l2 at dim 128 registers its private sets through the 128-D path: integer rows (the MFMA kernel)
    and non-integer rows (the float kernel) both give the yardstick's bits."""
    rng = np.random.default_rng(128)
    for rows in (sift_like, F.rootsift_like):
        q, t = rows(rng, 70), rows(rng, 300)
        d = _dist("f32", q, t)
        for r in _radii(d):
            _same(_host_ok(matcher, q, t, r), R.radius(d, r))


def test_borrowed_rows_of_any_alignment(matcher):
    """Device rows of a 128-D set are borrowed as they are: a base 4 bytes past a 16-byte boundary (float path)."""
    import torch
    rng = np.random.default_rng(41)
    q, t = F.rootsift_like(rng, 70), F.rootsift_like(rng, 300)
    d = _dist("f32", q, t)
    bufs = [torch.zeros(len(a) * 128 + 1, dtype=torch.float32, device="cuda") for a in (q, t)]
    views = []
    for b, a in zip(bufs, (q, t)):
        v = b[1:].view(len(a), 128)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        views.append(v)
    matcher.clear_sets()
    try:
        qs = matcher.add_set(views[0], torch.zeros((70, 2), device="cuda"))
        ts = matcher.add_set(views[1], torch.zeros((300, 2), device="cuda"))
        for r in _radii(d)[:1] + _radii(d)[3:]:
            _same(_sets(matcher, qs, ts, r), R.radius(d, r))
    finally:
        matcher.clear_sets()


def test_overflowed_distances_match_only_an_infinite_radius(matcher):
    """A squared distance that overflows gives the distance +inf: inside r = +inf alone, and sorted last."""
    rng = np.random.default_rng(9)
    q = F.normal_rows(rng, 70, 64)
    huge = (np.float32(3e19) * (1 + np.abs(F.normal_rows(rng, 90, 64)))).astype(np.float32)  # every square overflows
    t = huge.copy()
    t[[7, 50]] = q[[5, 3]]
    big = (np.float32(1e18) * F.normal_rows(rng, 2, 64)).astype(np.float32)  # finite d^2 ~ 1e38
    t = np.concatenate([t, big])
    d = _dist("f32", q, t)
    assert np.isinf(d).sum() == 70 * 88 and not np.isnan(d).any()
    for r in (f32(1.0), f32(20.0), f32(1e19), f32(2e19), np.finfo(np.float32).max, f32(np.inf)):
        exp = R.radius(d, r)
        _same(_host_ok(matcher, q, t, r), exp)
    assert exp[0][-1] == d.size and np.isinf(exp[2][exp[0][1] - 1])
    assert R.radius(d, np.finfo(np.float32).max)[0][-1] == 70 * 4


# 2. MFMA boundaries on integer rows, with planted rows
def _planted():
    rng = np.random.default_rng(2)
    qa = sift_like(rng, 1)[0]
    qa[:6] = (100, 50, 50, 50, 50, 50)
    qb = qa.copy()
    qb[5] += 1  # the other parity of |q - 128|^2, so of c(q) and of the train norms at one d^2
    deltas = {9999: (99, 14, 1, 1), 10000: (100, 0, 0, 0), 10001: (100, 1, 0, 0), 10002: (100, 1, 1, 0)}
    t = sift_like(rng, 150 + 8 + 5)  # 163 rows: two whole tiles and 35 rows of a third
    pos = [3, 40, 63, 64, 97, 128, 150, 162]  # both 32-row halves of every tile, the last row
    for p, (base, d2) in zip(pos, [(b, d2) for b in (qa, qb) for d2 in sorted(deltas)]):
        t[p] = base
        t[p, :4] += np.asarray(deltas[d2], np.float32)
    # d^2 = 8,000,001 and 8,000,000 from the zero row (they share a sqrtf), 8,000,005, 7,999,752 and the maximum
    far = np.zeros((5, 128), np.float32)
    far[:, :123] = 255
    far[0, 123:] = (43, 8, 3, 2, 0)
    far[1, 123:] = (43, 8, 2, 2, 2)
    far[2, 123:] = (43, 8, 3, 2, 2)
    far[3, 123:] = (40, 8, 3, 2, 0)
    far[4] = 255
    t[[10, 70, 71, 130, 161]] = far
    q = np.concatenate([np.stack([qa, qb, np.zeros(128, np.float32)]), sift_like(rng, 67)])  # 70 rows
    return q, t


def test_mfma_boundaries(matcher):
    q, t = _planted()
    assert len(q) % 64 and len(t) % 64 and (t >= 0).all() and (t <= 255).all() and (t == np.rint(t)).all()
    d2 = F.l2sqr(q, t)
    n2_par = (((t - 128) ** 2).sum(axis=1).astype(np.int64)) & 1
    for row in (0, 1):  # pairs at T2 and T2 + 1 for an even and an odd T2, under both parities of the train norm
        for T2 in (10000, 10001):
            assert (d2[row] == T2).any() and (d2[row] == T2 + 1).any()
    at = lambda v: {int(p) for p in n2_par[np.nonzero((d2[:2] == v).any(axis=0))[0]]}
    assert at(10000) == {0, 1} and at(10001) == {0, 1}
    assert d2[2, 10] == 8000001 and d2[2, 70] == 8000000 and d2[2, 161] == MAX_D2
    d = _dist("f32", q, t)
    s8 = np.sqrt(f32(8000000))
    assert s8 == np.sqrt(f32(8000001)) and d[2, 10] == d[2, 70] == s8
    top = np.sqrt(f32(MAX_D2))
    radii = [f32(100), np.sqrt(f32(10001)), np.sqrt(f32(9999)), np.nextafter(f32(100), f32(0)), s8, np.nextafter(s8, f32(0)),
             top, np.nextafter(top, f32(0)), f32(np.inf)]
    matcher.clear_sets()
    try:
        qs, ts = matcher.add_set(q, np.zeros((len(q), 2), f32)), matcher.add_set(t, np.zeros((len(t), 2), f32))
        # the same train rows and one more that is not an integer: the float kernel's problem
        t_mixed = np.concatenate([t, np.full((1, 128), 0.5, f32)])
        tm = matcher.add_set(t_mixed, np.zeros((len(t_mixed), 2), f32))
        d_mixed = _dist("f32", q, t_mixed)
        for r in radii:
            exp = R.radius(d, r)
            got = _sets(matcher, qs, ts, r)
            _same(got, exp)
            assert (got[1] < len(t)).all() and (got[1] >= 0).all()
            mixed = _sets(matcher, qs, tm, r)
            _same(mixed, R.radius(d_mixed, r))
            keep = mixed[1] < len(t)  # without the extra row: the MFMA path's answer, bit for bit
            np.testing.assert_array_equal(mixed[1][keep], got[1])
            np.testing.assert_array_equal(mixed[2][keep].view(np.int32), got[2].view(np.int32))
        o, i, _ = _sets(matcher, qs, ts, s8)
        assert {10, 70} <= set(i[o[2]:o[3]]) and 71 not in set(i[o[2]:o[3]])
        o, i, dd = _sets(matcher, qs, ts, f32(np.inf))  # no padded row, no padded query
        assert o[-1] == len(q) * len(t) and (np.diff(o) == len(t)).all() and i[o[3] - 1] == 161 and dd[o[3] - 1] == top
        o, i, _ = _sets(matcher, qs, ts, np.nextafter(top, f32(0)))
        assert o[3] - o[2] == len(t) - 1
    finally:
        matcher.clear_sets()


# 3. lists longer than the in-LDS sort: two merge levels, a one-key last run, distances tied in the thousands
def test_long_lists(matcher):
    cap = int(matcher.kernel_ms("radius_sort_cap"))
    assert cap >= 64 and cap & (cap - 1) == 0
    nq, nt = 3, 4 * cap + 1
    assert nt < (1 << 18) and nq * nt < 1_000_000
    rng = np.random.default_rng(3)
    q, t = orb_like(rng, nq, 4), orb_like(rng, nt, 4)  # 33 possible distances
    d = _dist("bin4", q, t)
    assert max(np.unique(d[0], return_counts=True)[1]) > 1000
    exp = R.radius(d, 32.0)
    assert exp[0][-1] == nq * nt
    _same(_host_ok(matcher, q, t, 32.0), exp)
    r = np.sort(d[0])[2 * cap + 7]  # lists of about 2 cap: one merge level, runs of unequal length
    _same(_host_ok(matcher, q, t, r), R.radius(d, r))


# 4. one count / fill call over all four kinds: every problem's segment equals its own one-problem result
def test_batch_of_mixed_kinds(matcher):
    rng = np.random.default_rng(4)
    data = [("bin32", 257, 129), ("f32_200", 5, 3), ("sift_int", 333, 700), ("sift_real", 70, 130), ("bin61", 40, 300)]
    matcher.clear_sets()
    try:
        probs, rows = [], []
        for kind, nq, nt in data:
            q, t = _rows(kind, rng, nq), _rows(kind, rng, nt)
            probs.append((_add(matcher, kind, q), _add(matcher, kind, t)))
            rows.append((kind, q, t))
        ds = [_dist(kind, q, t) for kind, q, t in rows]
        # one radius for the whole call: the 5 % quantile of each kind's own problem in turn (the others' lists are
        # then empty, partial or complete)
        for r in (np.sort(ds[0].ravel())[ds[0].size // 20], np.sort(ds[2].ravel())[ds[2].size // 20],
                  np.sort(ds[3].ravel())[ds[3].size // 20]):
            got = matcher.radius_batch(probs, r)
            matcher.synchronize()
            off, idx, dist = _np(got)
            assert len(off) == sum(nq for _, nq, _ in data) + 1 and off[-1] == len(idx) == len(dist)
            q0 = 0
            for (qs, ts), (kind, q, t) in zip(probs, rows):
                seg = off[q0:q0 + len(q) + 1]
                got = (seg - seg[0], idx[seg[0]:seg[-1]], dist[seg[0]:seg[-1]])
                _same(got, _sets(matcher, qs, ts, r))
                _same(got, R.radius(ds[probs.index((qs, ts))], r))
                q0 += len(q)
    finally:
        matcher.clear_sets()


# 5. the contract of the entries
def test_contract(matcher):
    import torch
    rng = np.random.default_rng(5)
    L, ctx = matcher.L, matcher.ctx
    matcher.clear_sets()
    try:
        q, t = sift_like(rng, 300), sift_like(rng, 900)
        t[:60] = q[:60]
        qs = matcher.add_set(q, rng.uniform(0, 500, (300, 2)).astype(np.float32))
        ts = matcher.add_set(t, rng.uniform(0, 500, (900, 2)).astype(np.float32))
        empty = matcher.add_set(np.zeros((0, 128), f32), np.zeros((0, 2), f32))
        bq = matcher.add_binary_set(orb_like(rng, 40, 32), np.zeros((40, 2), f32))
        prm = default_params(max_iters=500)
        batch_before = matcher.match_batch([(qs, ts)], prm).tobytes()
        knn_before = matcher.knn_match_arrays(q, t)
        d = _dist("f32", q, t)
        r = np.sort(d.ravel())[3000]
        exp = R.radius(d, r)
        total = C.c_int64(-1)
        one = (Problem * 1)(Problem(qs, ts))

        def count(problems, n, rr, off=None):
            return L.mim_radius_count(ctx, problems, n, float(rr), C.c_void_p(off.data_ptr()) if off is not None else None,
                                      C.byref(total))

        # max_distance of 0, negative, NaN, FLT_EPSILON itself: MIM_EINVAL with a text
        for bad in (0.0, -1.0, float("nan"), float(EPS), float("-inf")):
            assert count(one, 1, bad) == _lib.MIM_EINVAL and L.mim_last_error(ctx).decode() != ""
            assert _host(matcher, q[:5], t[:5], bad)[0] == _lib.MIM_EINVAL
            assert _host(matcher, orb_like(rng, 5, 32), orb_like(rng, 5, 32), bad)[0] == _lib.MIM_EINVAL
            with pytest.raises(ValueError):
                matcher.radius_match(q[:5], t[:5], bad)
        # a failed count leaves nothing to fill
        idx = torch.full((exp[0][-1] + 8,), -7, dtype=torch.int32, device="cuda")
        dist = torch.full((exp[0][-1] + 8,), -7, dtype=torch.float32, device="cuda")
        fill = lambda cap: L.mim_radius_fill_dev(ctx, C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()), cap)
        assert fill(len(idx)) == _lib.MIM_EINVAL and L.mim_last_error(ctx).decode() != ""
        # pairing rules are mim_batch_run's
        assert count((Problem * 1)(Problem(qs, bq)), 1, r) == _lib.MIM_EINVAL
        assert count((Problem * 1)(Problem(qs, 99)), 1, r) == _lib.MIM_EINVAL
        # cap < total: MIM_ERANGE, nothing written; then the same count filled twice
        off = torch.full((301,), -7, dtype=torch.int64, device="cuda")
        assert count(one, 1, r, off) == _lib.MIM_OK and total.value == exp[0][-1] > 300
        assert fill(total.value - 1) == _lib.MIM_ERANGE
        matcher.synchronize()
        assert (idx == -7).all() and (dist == -7).all()
        for _ in range(2):
            assert fill(len(idx)) == _lib.MIM_OK
            matcher.synchronize()
            _same((off.cpu().numpy(), idx.cpu().numpy()[:total.value], dist.cpu().numpy()[:total.value]), exp)
            assert (idx[total.value:] == -7).all()
        rec = np.full(4, 0x5A5A5A5A, np.int64)  # no batch records after a radius call
        assert L.mim_batch_results(ctx, C.c_void_p(rec.ctypes.data)) == _lib.MIM_OK and (rec == 0x5A5A5A5A).all()
        # host entries: cap < total gives the offsets and nothing else; idx NULL the offsets only
        st, o, i, dd = _host(matcher, q, t, r, cap=int(exp[0][-1]) - 1)
        assert st == _lib.MIM_ERANGE and (o == exp[0]).all() and (i == -7).all() and (dd == -7).all()
        st, o, i, dd = _host(matcher, q, t, r, cap=0, want_idx=False)
        assert st == _lib.MIM_OK and (o == exp[0]).all()
        # a host call consumed the ctx's last count: nothing to fill
        assert fill(len(idx)) == _lib.MIM_EINVAL
        # n = 0 and empty sets
        off1 = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        assert count(None, 0, r, off1) == _lib.MIM_OK and total.value == 0
        assert L.mim_radius_fill_dev(ctx, None, None, 0) == _lib.MIM_OK
        matcher.synchronize()
        assert off1.item() == 0
        for a, b, nq in ((empty, ts, 0), (qs, empty, 300), (empty, empty, 0)):
            o, i, dd = _sets(matcher, a, b, r)
            assert len(o) == nq + 1 and (o == 0).all() and len(i) == len(dd) == 0
        for qq, tt in ((q[:0], t), (q[:7], t[:0])):
            st, o, i, dd = _host(matcher, qq, tt, r, cap=4)
            assert st == _lib.MIM_OK and (o == 0).all() and (i == -7).all()
        # fill after clear_sets: MIM_EINVAL (checked last: it drops the sets)
        assert count(one, 1, r) == _lib.MIM_OK
        # a k = 2 call and a batch run after radius calls give what they gave before
        for a, b in zip(matcher.knn_match_arrays(q, t), knn_before):
            np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
        assert matcher.match_batch([(qs, ts)], prm).tobytes() == batch_before
        assert count(one, 1, r) == _lib.MIM_OK
        matcher.clear_sets()
        assert fill(len(idx)) == _lib.MIM_EINVAL and "cleared" in L.mim_last_error(ctx).decode()
    finally:
        matcher.clear_sets()


def test_fill_without_a_count():
    m = Matcher(0)
    try:
        assert m.L.mim_radius_fill_dev(m.ctx, None, None, 0) == _lib.MIM_EINVAL
        assert m.L.mim_last_error(m.ctx).decode() != ""
    finally:
        m.close()


def test_python_lists(matcher):
    rng = np.random.default_rng(6)
    for fn, q, t, kind in ((matcher.radius_match, sift_like(rng, 9), sift_like(rng, 80), "f32"),
                           (matcher.radius_match_float, F.normal_rows(rng, 9, 33), F.normal_rows(rng, 80, 33), "f32"),
                           (matcher.radius_match_hamming, orb_like(rng, 9, 32), orb_like(rng, 80, 32), "bin")):
        d = X.distances(kind, q, t)
        r = np.sort(d.ravel())[100]
        off, idx, dist = R.radius(d, r)
        lists = fn(q, t, r)
        assert [len(m) for m in lists] == list(np.diff(off))
        flat = [m for ms in lists for m in ms]
        assert [m.trainIdx for m in flat] == list(idx) and [f32(m.distance) for m in flat] == list(dist)
        assert all(m.queryIdx == i and m.imgIdx == 0 for i, ms in enumerate(lists) for m in ms)
    matcher.clear_sets()
    try:
        qs = matcher.add_set(sift_like(rng, 9), np.zeros((9, 2), f32))
        with pytest.raises(MimError):
            matcher.radius_batch([(qs, 98)], 1.0)
        with pytest.raises(ValueError):
            matcher.radius_sets(98, qs, 1.0)  # a query set this object did not register: its rows are not known
    finally:
        matcher.clear_sets()


# 6. the first 16 entries of every list are knnMatch's (mim_knn_sets_dev at k = 16), bit for bit
@pytest.mark.parametrize("kind", ["bin32", "f32_64", "sift_int", "sift_real"])
def test_agrees_with_the_topk_entries(matcher, kind):
    import torch
    rng = np.random.default_rng(60 + KINDS.index(kind))
    nq, nt, k = 150, 400, 16
    q, t = _rows(kind, rng, nq), _rows(kind, rng, nt)
    matcher.clear_sets()
    try:
        qs, ts = _add(matcher, kind, q), _add(matcher, kind, t)
        ki = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
        kd = torch.full((nq, k), -7, dtype=torch.float32, device="cuda")
        matcher._check(matcher.L.mim_knn_sets_dev(matcher.ctx, qs, ts, k, C.c_void_p(ki.data_ptr()), C.c_void_p(kd.data_ptr())))
        matcher.synchronize()
        ki, kd = ki.cpu().numpy(), kd.cpu().numpy()
        r = kd[:, k - 1].max()  # every query's 16th distance lies within it
        off, idx, dist = _sets(matcher, qs, ts, r)
        assert (np.diff(off) >= k).all()
        first = off[:-1, None] + np.arange(k)
        np.testing.assert_array_equal(idx[first], ki)
        np.testing.assert_array_equal(dist[first].view(np.int32), kd.view(np.int32))
    finally:
        matcher.clear_sets()
