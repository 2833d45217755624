"""CPU yardstick for BFMatcher(norm).radiusMatch(q, t, matches, maxDistance) on a distance matrix.

OpenCV (4.5.4, recalled: this suite cannot call it, so this is unpinned against it) computes the whole distance
matrix with batchDistance(K = 0), pushes for query i every train row j with dist(i, j) <= maxDistance (a float32
compare of DMatch::distance against the float maxDistance) and then std::sorts each query's list by distance.
std::sort leaves the order of equal distances open; the lower train index first is one of the orders it may
produce and the tie rule of every other entry of the library, so that is the order here.  A NaN distance fails
the compare; an overflowed +inf distance passes it only for maxDistance = +inf.

* radius(d, r): that rule on a float32 (nq, nt) matrix, vectorised: the mask d <= float32(r), a stable argsort per
  row.  Returns the CSR triple (offsets int64 (nq + 1), idx int32, dist float32).
* radius_loop(d, r): the literal push-then-sort form with the (distance, index) tie rule.

The distance matrices come from cross_ref.distances (the bits DMatch::distance carries per kind).
"""
import numpy as np


def radius(d, r):
    d = np.asarray(d, np.float32)
    nq = d.shape[0]
    with np.errstate(invalid="ignore"):
        mask = d <= np.float32(r)
    offsets = np.zeros(nq + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=offsets[1:])
    if mask.size == 0:
        return offsets, np.zeros(0, np.int32), np.zeros(0, np.float32)
    order = np.argsort(d, axis=1, kind="stable")  # NaN last: never under the mask
    keep = np.take_along_axis(mask, order, axis=1)
    idx = order[keep].astype(np.int32)  # row-major: query by query, each in sorted order
    dist = np.take_along_axis(d, order, axis=1)[keep].astype(np.float32)
    return offsets, idx, dist


def radius_loop(d, r):
    d = np.asarray(d, np.float32)
    r = np.float32(r)
    offsets, idx, dist = [0], [], []
    for row in d:
        found = []
        for j, v in enumerate(row):
            if v <= r:  # False for a NaN
                found.append((v, j))
        found.sort(key=lambda e: (e[0], e[1]))
        idx += [j for _, j in found]
        dist += [v for v, _ in found]
        offsets.append(len(idx))
    return np.asarray(offsets, np.int64), np.asarray(idx, np.int32), np.asarray(dist, np.float32)
