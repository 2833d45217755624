"""CPU yardstick for knnMatch over a train collection: BFMatcher::add(images) + knnMatch(query, matches, k)
(DESIGN.md §18), on a list of float32 distance matrices (nq, nt_i), one per train image in image order.

BFMatcher::knnMatchImpl calls batchDistance once per image, in order, with update = imgIdx << 18, on the same K
lists: a distance d is inserted where `d < dist[K-1]`, shifting entries while `dist[j] > d`.  An equal distance
never passes an earlier (image, row), so per query row the result is the k smallest under (distance, imgIdx,
trainIdx), ascending.  The lists start at FLT_MAX: a distance not below FLT_MAX (an overflowed squared distance,
a NaN) is never inserted.  Absent entries are trainIdx -1, imgIdx -1, distance FLT_MAX.

* topk_collection(dists, k): vectorised: the columns concatenated in image order, a stable sort, and each column
  mapped back to (image, row).
* update_loop(dists, k): the literal per-image insertion with `update`.
* merge_groups(dists, k, cuts): the collection cut into groups of images, each group's k best merged into what the
  groups before it left (what the library does under a byte budget).

The distance matrices come from cross_ref.distances (the bits DMatch::distance carries per kind).
"""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
IMG_SHIFT = 18
MAX_IMAGES = 8191


def topk_collection(dists, k):
    """(idx, img int32 (nq, k), dist float32 (nq, k))."""
    dists = [np.asarray(d, np.float32) for d in dists]
    nq = dists[0].shape[0]
    idx = np.full((nq, k), -1, np.int32)
    img = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    d = np.concatenate(dists, axis=1)
    col_img = np.concatenate([np.full(x.shape[1], i, np.int32) for i, x in enumerate(dists)])
    col_row = np.concatenate([np.arange(x.shape[1], dtype=np.int32) for x in dists])
    m = min(k, d.shape[1])
    if nq and m:
        with np.errstate(invalid="ignore"):
            key = np.where(d < FLT_MAX, d, np.float32(np.inf))  # never inserted: behind every finite distance
        order = np.argsort(key, axis=1, kind="stable")[:, :m]
        dd = np.take_along_axis(d, order, axis=1)
        with np.errstate(invalid="ignore"):
            ok = dd < FLT_MAX
        idx[:, :m] = np.where(ok, col_row[order], -1)
        img[:, :m] = np.where(ok, col_img[order], -1)
        dist[:, :m] = np.where(ok, dd, FLT_MAX)
    return idx, img, dist


def _insert(bd, bu, v, update, k):
    """batchDistance's insertion of one value: update = (imgIdx << 18) + row."""
    if v < bd[k - 1]:
        p = k - 2
        while p >= 0 and bd[p] > v:
            bd[p + 1], bu[p + 1] = bd[p], bu[p]
            p -= 1
        bd[p + 1], bu[p + 1] = v, update


def update_loop(dists, k, seed=None):
    """The insertion as OpenCV writes it, image by image; seed: (idx, img, dist) lists to start from."""
    dists = [np.asarray(d, np.float32) for d in dists]
    nq = dists[0].shape[0] if dists else seed[0].shape[0]
    idx = np.full((nq, k), -1, np.int32)
    img = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    for i in range(nq):
        bd, bu = [FLT_MAX] * k, [-1] * k
        if seed is not None:
            for s in range(k):
                if seed[0][i, s] >= 0:
                    bd[s], bu[s] = seed[2][i, s], (int(seed[1][i, s]) << IMG_SHIFT) + int(seed[0][i, s])
        for im, d in enumerate(dists):
            base = (im + (seed[3] if seed is not None else 0)) << IMG_SHIFT
            for j, v in enumerate(d[i]):
                _insert(bd, bu, v, base + j, k)
        for s in range(k):
            if bu[s] >= 0:
                idx[i, s], img[i, s], dist[i, s] = bu[s] & ((1 << IMG_SHIFT) - 1), bu[s] >> IMG_SHIFT, bd[s]
    return idx, img, dist


def merge_groups(dists, k, cuts):
    """Groups of images [cuts[g], cuts[g + 1]) taken in order, each started from the lists the previous one left."""
    out = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        out = update_loop(dists[a:b], k, seed=None if out is None else (*out, a))
    return out
