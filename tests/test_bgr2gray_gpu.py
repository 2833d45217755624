"""cvtColor(BGR2GRAY) on the device (bgr2gray_u8_kernel: mim_cvt_bgr2gray_u8, mim_sift_scales_sets_image).

The reference converts every scene first (preprocessImage, preprocessing.cpp:11).  The expected values
are the integer formula the fixtures of tests/golden were built with, restated in numpy here:
gray = (R * 4899 + G * 9617 + B * 1868 + (1 << 13)) >> 14 in 32-bit integers.  Equality is exact."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.7, 0.85, 1.0, 1.15, 1.3)  # TestsDetector.cpp:99


def gray_numpy(bgr):
    b, g, r = (bgr[..., k].astype(np.int32) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def test_every_bgr_triple(matcher):
    """One 4096 x 4096 image holding each of the 2^24 (B, G, R) triples once."""
    i = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    got = matcher.cvt_bgr2gray(bgr)
    assert got.shape == (4096, 4096) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, gray_numpy(bgr))


@pytest.mark.parametrize("rows,cols,pad", [(1, 1, 0), (3, 5, 0), (7, 13, 5), (2, 641, 0)])
def test_shapes_and_row_step(matcher, rows, cols, pad):
    """Fewer than four pixels, pixel counts that are no multiple of four (the byte-wise tail), a row
    step larger than 3 * cols (7 x 13 with step 3 * 13 + 5), more than one block (2 x 641)."""
    rng = np.random.default_rng(rows * 1000 + cols)
    step = 3 * cols + pad
    buf = rng.integers(0, 256, (rows, step), dtype=np.uint8)
    bgr = np.lib.stride_tricks.as_strided(buf, (rows, cols, 3), (step, 3, 1))
    assert bgr.strides[0] == step
    got = matcher.cvt_bgr2gray(bgr)
    np.testing.assert_array_equal(got, gray_numpy(bgr))


def test_colour_scene_gives_the_gray_scene_sets(matcher):
    """A colour scene through sift_scales_to_sets registers bit for bit the sets of its numpy gray
    conversion: row counts, descriptors and keypoint positions at all five scales."""
    with np.load(os.path.join(ROOT, "tests", "golden", "c1_sugar_box.npz")) as z:
        g = z[sorted(k for k in z.files if k.startswith("scene/"))[0]]
    bgr = np.stack([g, g[:, ::-1], np.roll(g, 17, axis=0)], axis=2)
    assert bgr.shape == g.shape + (3,)
    matcher.clear_sets()
    try:
        ids_c, n_c, _ = matcher.sift_scales_to_sets(bgr, SCALES)
        ids_g, n_g, _ = matcher.sift_scales_to_sets(gray_numpy(bgr), SCALES)
        assert len(ids_c) == len(ids_g) == len(SCALES)
        assert n_c == n_g and min(n_c) > 0
        for a, b in zip(ids_c, ids_g):
            da, ka = matcher.set_rows(a)
            db, kb = matcher.set_rows(b)
            assert da.shape == db.shape and ka.shape == kb.shape
            assert da.tobytes() == db.tobytes()
            assert ka.tobytes() == kb.tobytes()
    finally:
        matcher.clear_sets()


def _image_call(matcher, arr, channels, step):
    from computervision_objectdetection_featurematching_amd import _lib
    sc = np.asarray(SCALES, np.float32)
    ids, n = np.zeros(5, np.int32), np.zeros(5, np.int32)
    img = _lib.Image(C.c_void_p(arr.ctypes.data), arr.shape[0], arr.shape[1] // max(channels, 1), channels, step)
    st = matcher.L.mim_sift_scales_sets_image(matcher.ctx, C.byref(img), 5, C.c_void_p(sc.ctypes.data),
                                              C.c_void_p(ids.ctypes.data), C.c_void_p(n.ctypes.data), 0, None)
    return st, matcher.L.mim_last_error(matcher.ctx).decode()


def test_bad_arguments(matcher):
    from computervision_objectdetection_featurematching_amd import _lib
    matcher.clear_sets()
    arr = np.zeros((16, 48), np.uint8)
    for ch in (2, 4):
        st, msg = _image_call(matcher, arr, ch, 48)
        assert st == _lib.MIM_EINVAL and "channels" in msg, (st, msg)
    st, msg = _image_call(matcher, arr, 3, 3 * 16 - 1)  # 16 x 16 x 3 with a step one byte short
    assert st == _lib.MIM_EINVAL and "step" in msg, (st, msg)
    out = np.zeros((16, 16), np.uint8)
    st = matcher.L.mim_cvt_bgr2gray_u8(matcher.ctx, C.c_void_p(arr.ctypes.data), 16, 16, 3 * 16 - 1,
                                       C.c_void_p(out.ctypes.data))
    msg = matcher.L.mim_last_error(matcher.ctx).decode()
    assert st == _lib.MIM_EINVAL and "step" in msg, (st, msg)
    assert matcher.sets_info()[0] == 0  # nothing was registered by the refused calls
    with pytest.raises(_lib.MimError) as e:  # the Python entry hands the channel count to the library
        matcher.sift_scales_to_sets(np.zeros((16, 16, 4), np.uint8), SCALES)
    assert e.value.code == _lib.MIM_EINVAL
