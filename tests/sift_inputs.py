"""Seeded input images for the SIFT tests (a plain module, shared by the CPU and GPU tests).

blobs() of test_sift_gpu.py is smooth and gives a few dozen keypoints; these two are dense, so that
most pyramid pixels matter to some keypoint and every octave holds extrema.
"""
import numpy as np


def multi(seed, r, c):            # noise at six scales: keypoints in every octave
    rng = np.random.default_rng(seed); a = np.zeros((r, c))
    for s in (1, 2, 4, 8, 16, 32):
        n = rng.normal(0, 1, ((r + s - 1) // s + 1, (c + s - 1) // s + 1))
        a += s ** 0.5 * np.kron(n, np.ones((s, s)))[:r, :c]
    a = (a - a.min()) / (a.max() - a.min()) * 255
    return np.rint(a).astype(np.uint8)


def tex(seed, r, c, blur=1):      # dense fine texture: many keypoints per pixel
    a = np.random.default_rng(seed).integers(0, 256, (r, c)).astype(np.float64)
    for _ in range(blur):
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(np.roll(a, 1, 0), 1, 1)) / 4
    a = (a - a.min()) / (a.max() - a.min()) * 255
    return np.rint(a).astype(np.uint8)


# (rows, cols) of the pyramid cases; case i is multi(100 + i, rows, cols)
PYRAMID_SHAPES = (
    (23, 23),    # 0: octave 1 = 529 px (batched), 5 octaves
    (22, 23),    # 1: octave 1 = 506 px (fused), 4 octaves
    (11, 300),   # 2: strip, doubled 22 rows: 12 interior rows in octave 0 only
    (300, 11),   # 3: the same, transposed
    (6, 400),    # 4: doubled 12 rows: tap radius 13 >= rows, reflection wraps twice
    (400, 6),    # 5: the same, transposed
    (5, 400),    # 6: doubled 10 rows: no interior, pyramid only
    (16, 32),    # 7: doubled 32x64: exactly one blur tile
    (32, 64),    # 8: doubled 64x128: whole tiles
    (33, 65),    # 9: one row and two columns past a tile
    (31, 63),    # 10: two short of a tile
    (64, 128),   # 11
    (65, 129),   # 12
    (45, 91),    # 13
    (46, 91),    # 14
    (61, 97),    # 15
    (97, 61),    # 16
    (12, 14),    # 17: test_sift_edge_cases' `tiny`
    (128, 96),   # 18
)


def pyramid_case(i):
    return multi(100 + i, *PYRAMID_SHAPES[i])


def kp_octaves(kps):
    """Octave of each keypoint (-1 for the doubled image), unpacked from cv::KeyPoint::octave."""
    o = kps["octave"] & 255
    return np.where(o < 128, o, o - 256)


def pyramid_diffs(got, want):
    """Compare two pyramids (n_oct, orows[16], ocols[16], flat planes; 6 Gaussian then 5 DoG layers per
    octave) bit for bit.  Returns a list of messages, empty when they are identical: the geometry
    first, then per differing plane its octave, layer, kind, the number of differing pixels and the
    first differing (y, x) with both values."""
    gn, gr, gc, gp = got[:4]
    wn, wr, wc, wp = want[:4]
    if gn != wn or not np.array_equal(gr, wr) or not np.array_equal(gc, wc):
        return [f"geometry: n_oct {gn} / {wn}, rows {list(gr[:max(gn, wn)])} / {list(wr[:max(gn, wn)])}, "
                f"cols {list(gc[:max(gn, wn)])} / {list(wc[:max(gn, wn)])}"]
    if gp.size != wp.size:
        return [f"planes: {gp.size} floats / {wp.size}"]
    out, off = [], 0
    gi, wi = gp.view(np.int32), wp.view(np.int32)
    for o in range(wn):
        r, c = int(wr[o]), int(wc[o])
        for l in range(11):
            a, b = gi[off:off + r * c].reshape(r, c), wi[off:off + r * c].reshape(r, c)
            if not np.array_equal(a, b):
                ys, xs = np.nonzero(a != b)
                y, x = int(ys[0]), int(xs[0])
                kind, layer = ("gauss", l) if l < 6 else ("dog", l - 6)
                out.append(f"octave {o} {kind} layer {layer} ({r}x{c}): {len(ys)} pixels differ, first at "
                           f"(y={y}, x={x}): {gp[off + y * c + x]!r} / {wp[off + y * c + x]!r}")
            off += r * c
    return out


def assert_keypoint_greater_order(k, label=""):
    """A final keypoint list is strictly descending in KeypointGreater order (x, y, size, angle, response,
    octave) and holds no two neighbours equal in x, y, size and angle (removeDuplicatedSorted).  Checked
    on the list alone: an alignment of two lists by their fields does not see a wrong order."""
    order = np.lexsort((-k["octave"].astype(np.int64), -k["response"], -k["angle"], -k["size"], -k["y"], -k["x"]))
    bad = np.nonzero(order != np.arange(len(k)))[0]
    assert bad.size == 0, f"{label}: not in KeypointGreater order from index {bad[0]}: {k[max(bad[0] - 1, 0):bad[0] + 2]}"
    dup = np.ones(max(len(k) - 1, 0), bool)
    for f in ("x", "y", "size", "angle"):
        dup &= k[f][1:] == k[f][:-1]
    assert not dup.any(), f"{label}: duplicate neighbours at {np.nonzero(dup)[0][:5]}"
