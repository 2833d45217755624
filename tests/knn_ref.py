"""CPU yardstick for BFMatcher(norm).knnMatch(q, t, matches, k) on a distance matrix.

OpenCV's top-K insertion (batchDistance with K > 0) scans the train rows in ascending order and, for a
distance d, inserts where `d < dist[K-1]`, shifting entries while `dist[j] > d`.  An equal distance never moves
past an earlier row, so the result is the first k of a stable sort by distance: the k smallest under
(distance, train index), ascending.  The list starts at FLT_MAX, so a distance that is not below FLT_MAX (an
overflowed squared distance, a NaN) is never inserted.

* topk(d, k): that rule on a float32 (nq, nt) matrix, vectorised.  Absent entries (nt < k, or fewer than k
  distances below FLT_MAX) are index -1 with distance FLT_MAX, as cross_ref.top2 and the library write them.
* insertion_loop(d, k): the literal restatement, row by row.

The distance matrices come from cross_ref.distances (the bits DMatch::distance carries per kind).
"""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
MAX_K = 16


def topk(d, k):
    """(idx int32 (nq, k), dist float32 (nq, k)) from the float32 distance matrix d (nq, nt)."""
    d = np.asarray(d, np.float32)
    nq, nt = d.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    m = min(k, nt)
    if nq and m:
        with np.errstate(invalid="ignore"):
            key = np.where(d < FLT_MAX, d, np.float32(np.inf))  # never inserted: behind every finite distance
        order = np.argsort(key, axis=1, kind="stable")[:, :m]
        dd = np.take_along_axis(d, order, axis=1)
        with np.errstate(invalid="ignore"):
            ok = dd < FLT_MAX
        idx[:, :m] = np.where(ok, order, -1)
        dist[:, :m] = np.where(ok, dd, FLT_MAX)
    return idx, dist


def insertion_loop(d, k):
    """The insertion as OpenCV writes it, on every row of d."""
    d = np.asarray(d, np.float32)
    nq = d.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    for i in range(nq):
        bd, bi = [FLT_MAX] * k, [-1] * k
        for j, v in enumerate(d[i]):
            if v < bd[k - 1]:
                p = k - 2
                while p >= 0 and bd[p] > v:
                    bd[p + 1], bi[p + 1] = bd[p], bi[p]
                    p -= 1
                bd[p + 1], bi[p + 1] = v, j
        idx[i], dist[i] = bi, bd
    return idx, dist
