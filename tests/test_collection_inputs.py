"""CPU checks of tests/collection_inputs.py: from the yardsticks alone, the flags and sqrtf cases of
tests/test_collection_gpu.py are not vacuous."""
import numpy as np

import collection_inputs as CI
import collection_ref as CR
import cross_ref as X
import flagged_inputs as FI
import float_ref as F


def test_flagged_image_differs_from_the_i8_arithmetic():
    """Read as the integers the i8 path would take them for, the jittered image gives other lists."""
    qs, imgs = CI.flag_sets()
    assert (imgs[1] != np.rint(imgs[1])).any(axis=1).all()
    assert all((x == np.rint(x)).all() and x.min() >= 0 and x.max() <= 255 for x in (imgs[0], imgs[2], qs["QI"]))
    assert (qs["QR"] != np.rint(qs["QR"])).any(axis=1).all()
    d = [X.distances("f32", qs["QI"], t) for t in imgs]
    wrong = list(d)
    wrong[1] = X.distances("f32", qs["QI"], FI.as_i8_path(imgs[1]))
    a, b = CR.topk_collection(d, 2), CR.topk_collection(wrong, 2)
    assert {0, 1, 2} <= set(np.unique(a[1]))  # every image is among the nearest of some query
    assert not np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    # a jittered query against the integer images too
    dq = [X.distances("f32", qs["QR"], t) for t in imgs]
    wq = [X.distances("f32", FI.as_i8_path(qs["QR"]), t) for t in imgs]
    assert not np.array_equal(CR.topk_collection(dq, 2)[2].view(np.int32), CR.topk_collection(wq, 2)[2].view(np.int32))


def test_sqrt_rows_collide_and_the_orders_disagree():
    rows, far = CI.sqrt_rows()
    zero = np.zeros((1, 128), np.float32)
    d2 = {n: int(F.l2sqr(zero, r[None])[0, 0]) for n, r in rows.items()}
    assert (d2["A"], d2["B"], d2["C"], d2["N"]) == (8000001, 8000000, 8000005, 7999752)
    assert all(np.float32(v) == v for v in d2.values())  # exact in float
    sq = {n: int(np.sqrt(np.float32(v)).view(np.int32)) for n, v in d2.items()}
    assert sq["A"] == sq["B"] and sq["N"] < sq["A"] < sq["C"]
    img0, img1 = CI.sqrt_images()
    d = [X.distances("f32", zero, img0), X.distances("f32", zero, img1)]
    idx, img, _ = CR.topk_collection(d, 9)
    assert list(zip(img[0], idx[0])) == CI.SQRT_ORDER
    # a ranking on (d^2, image, row) differs at every cut from 3 to 7
    ridx, rimg, _ = CR.topk_collection([F.l2sqr(zero, img0), F.l2sqr(zero, img1)], 9)
    assert list(zip(rimg[0], ridx[0])) == CI.SQRT_ORDER_ON_D2
    for k in range(3, 8):
        assert CI.SQRT_ORDER[:k] != CI.SQRT_ORDER_ON_D2[:k]
    half = lambda r: (r % 8) // 4  # accumulator g of lane half h is row (g & 3) + 8 (g >> 2) + 4 h of the half tile
    assert {half(r) for r in (5, 13, 21, 29)} == {1} and half(9) == 0 and {r // 32 for r in (5, 9, 13, 21, 29)} == {0}
    assert 5 // 512 != 600 // 512  # two splits of the schedule
