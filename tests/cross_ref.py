"""CPU yardstick for cross-check matching, BFMatcher(norm, crossCheck=True).match.

With d(i, j) the DMatch::distance of the descriptor kind, s(i) the lowest j that minimises d(i, j) and t(j)
the lowest i that minimises d(i, j) (what batchDistance(..., K=1) gives in each direction: a strict `<`
while scanning ascending indices), query i is matched to s(i) iff t(s(i)) == i.

* mutual(d): that rule on a distance matrix, vectorised.
* cross_match_loops(d): the literal form, two batchDistance(K=1) scans and the loop over the queries.
* one_directional(d): the older form that is deliberately not provided (each query takes the closest train
  row among those that chose it, without a look at its own nearest).
* distances(kind, q, t): the yardstick distances of the kind, float32 (the bits the library returns).
* expected_problem(...): one problem's record under a filter, composed as hamming_ref.expected_problem.

A distance that is not below FLT_MAX is never a match, as in the top-2 (it is never inserted).
"""
import numpy as np

import float_ref
import hamming_ref

FLT_MAX = np.finfo(np.float32).max
FILTER_RATIO, FILTER_CROSS, FILTER_RATIO_CROSS = 0, 1, 2
FILTER_NAMES = {FILTER_RATIO: "ratio", FILTER_CROSS: "cross", FILTER_RATIO_CROSS: "ratio+cross"}
MIM_ACCEPTED, MIM_FEW_GOOD, MIM_EMPTY_H, MIM_FEW_INLIERS, MIM_BAD_DET = range(5)


def mutual(d):
    """(idx int32[nq], dist float32[nq]): the matched train row or -1, its distance or FLT_MAX."""
    d = np.asarray(d)
    nq, nt = d.shape
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, FLT_MAX, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    s = np.argmin(d, axis=1)  # the first of equal minima: the lowest index
    t = np.argmin(d, axis=0)
    rows = np.arange(nq)
    ok = (t[s] == rows) & (d[rows, s] < FLT_MAX)
    idx[ok] = s[ok]
    dist[ok] = d[rows, s][ok]
    return idx, dist


def batch_distance_k1(d):
    """batchDistance(src1, src2, K=1) on a distance matrix: per row, index and distance of the nearest column."""
    nidx, dist = [], []
    for row in d:
        best, bi = FLT_MAX, -1
        for j, v in enumerate(row):
            if v < best:
                best, bi = v, j
        nidx.append(bi)
        dist.append(best)
    return nidx, dist


def cross_match_loops(d):
    """The two-batchDistance form: forward and reverse nearest rows, then the mutual pairs in query order."""
    d = np.asarray(d)
    fwd, fdist = batch_distance_k1(d)
    rev, _ = batch_distance_k1(d.T)
    idx = np.full(d.shape[0], -1, np.int32)
    dist = np.full(d.shape[0], FLT_MAX, np.float32)
    for i in range(d.shape[0]):
        j = fwd[i]
        if j >= 0 and rev[j] == i:
            idx[i], dist[i] = j, fdist[i]
    return idx, dist


def one_directional(d):
    """The older form: query i is matched to the closest train row among those whose nearest query is i."""
    d = np.asarray(d)
    rev, _ = batch_distance_k1(d.T)
    idx = np.full(d.shape[0], -1, np.int32)
    dist = np.full(d.shape[0], FLT_MAX, np.float32)
    for j, i in enumerate(rev):
        if i >= 0 and d[i, j] < dist[i]:
            idx[i], dist[i] = j, d[i, j]
    return idx, dist


# the fixed counter-example: train row 1 chose query 0, whose own nearest row is 0, which chose query 1
COUNTER_EXAMPLE = np.array([[1, 2, 9], [0, 9, 9], [9, 9, 0]], np.float32)


def distances(kind, q, t, chunk=128):
    """float32 (nq, nt) distances: kind "bin" (uint8 rows, Hamming) or "f32" (float rows of any dim, the
    sqrt of float_ref.l2sqr, which is exact for integer-valued 128-D rows)."""
    nq, nt = len(q), len(t)
    out = np.zeros((nq, nt), np.float32)
    for a in range(0, nq, chunk):
        if kind == "bin":
            out[a:a + chunk] = hamming_ref.distances(q[a:a + chunk], t)
        else:
            with np.errstate(over="ignore", under="ignore"):
                out[a:a + chunk] = np.sqrt(float_ref.l2sqr(q[a:a + chunk], t))
    return out


def top2(d):
    """knnMatch(k=2) rows from a distance matrix (stable order; absent entries -1 / FLT_MAX)."""
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), FLT_MAX, np.float32)
    k = min(2, nt)
    if nq and k:
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        dd = np.take_along_axis(d, order, axis=1)
        ok = dd < FLT_MAX
        idx[:, :k] = np.where(ok, order, -1)
        dist[:, :k] = np.where(ok, dd, FLT_MAX)
    return idx, dist


def good_matches(O, d, filter, ratio):
    """(query rows, train rows) of the filter's survivors in ascending query order."""
    if filter == FILTER_RATIO:
        return O.ratio_filter(*top2(d), ratio)
    midx, _ = mutual(d)
    keep = midx >= 0
    if filter == FILTER_RATIO_CROSS:
        rq, _ = O.ratio_filter(*top2(d), ratio)
        passed = np.zeros(len(midx), bool)
        passed[rq] = True
        keep &= passed
    gq = np.nonzero(keep)[0].astype(np.int32)
    return gq, midx[gq]


def expected_problem(O, kind, qd, qk, td, tk, filter, max_iters=2000):
    """One problem's record composed on the CPU: the kind's yardstick distances, the filter, the points from
    the keypoints, oracle.find_homography, then the gates of mim.h's status codes."""
    prm = O.default_params(max_iters=max_iters)
    gq, gt = good_matches(O, distances(kind, qd, td), filter, prm.ratio)
    ng = len(gq)
    out = dict(n_good=ng, good_q=gq.copy(), good_t=gt.copy(), n_inl=0, iters=None, H=np.zeros((3, 3)), det=0.0,
               mask=np.zeros(0, np.uint8), status=MIM_FEW_GOOD)
    if ng < prm.min_good:
        return out
    src, dst = np.ascontiguousarray(qk[gq], np.float32), np.ascontiguousarray(tk[gt], np.float32)
    ok, H, mask = O.find_homography(src, dst, prm.ransac_thresh, max_iters, prm.confidence)
    if ng > 4:
        out["iters"] = O.ransac(src, dst, prm.ransac_thresh, prm.confidence, max_iters)["iters"]
    out["mask"] = mask if ok else np.zeros(ng, np.uint8)
    out["n_inl"] = int(out["mask"].sum())
    if not ok:
        out["status"] = MIM_EMPTY_H
    elif out["n_inl"] < prm.min_inliers:
        out["status"] = MIM_FEW_INLIERS
        out["H"] = None  # not compared
    else:
        out["H"] = H
        out["det"] = hamming_ref.det3(H)
        out["status"] = MIM_ACCEPTED if prm.det_lo <= abs(out["det"]) <= prm.det_hi else MIM_BAD_DET
    return out
