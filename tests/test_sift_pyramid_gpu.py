"""Every plane of the SIFT scale-space pyramid (csrc/sift.hip: up2, blur_reg, down2 and
small_octaves kernels) against oracle/sift_oracle.c, bit for bit.

The planes use no device transcendental: the Gaussian taps are computed on the host in double, exactly
as the oracle computes them, and both sides add in OpenCV's order (row pass sequential over the taps,
column pass k_a m + sum k_{a+i} (m_+i + m_-i), DoG = next - current, no FMA contraction).  So the
tolerance is zero, on the int32 views of the floats.  The planes are read back from the workspace of
the product call (Matcher.sift_debug_pyramid), nothing is recomputed.

The shapes (sift_inputs.PYRAMID_SHAPES) are the smallest that reach each geometry switch: a plane of
<= 512 px goes to the fused small_octaves_kernel (octave 1 of 23x23 is 529 px, of 22x23 506 px), the
octave count lrint(log2(min side) - 2) + 1 flips at the same pair, strips narrower than the tap radius
reflect more than once, planes of <= 10 px hold no extremum but feed the next octave, and the blur
tiles are 64 columns by 32 rows.  The inputs are multi(): noise at six scales, so every octave holds
keypoints and most plane pixels matter to one.
"""
import numpy as np
import pytest

from sift_inputs import PYRAMID_SHAPES, kp_octaves, pyramid_case, pyramid_diffs
from test_sift_gpu import compare_sift

pytestmark = pytest.mark.gpu

CASES = range(len(PYRAMID_SHAPES))


@pytest.fixture(scope="module")
def oracle_cases(oracle):
    """Per case: the image, the oracle's keypoints / descriptors and its pyramid, computed once."""
    out = []
    for i in CASES:
        img = pyramid_case(i)
        k, d = oracle.sift_detect_compute(img)
        out.append((img, k, d, oracle.sift_pyramid(img)))
    return out


def test_cases_are_not_vacuous(oracle_cases):
    """Checked on the oracle alone: the cases hold keypoints, in every octave the shapes reach."""
    n = [len(k) for _, k, _, _ in oracle_cases]
    print("oracle keypoints per case:", n)
    for i in (2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 16):
        assert n[i] >= 20, (i, n[i])
    assert n[6] == 0 and oracle_cases[6][3][0] > 0  # 5x400: no interior, yet a pyramid to compare
    octs = set(np.concatenate([kp_octaves(k) for _, k, _, _ in oracle_cases]).tolist())
    assert {-1, 0, 1, 2} <= octs, octs
    # the two sides of the fused-octave threshold and of the octave-count flip
    assert oracle_cases[0][3][0] == 5 and oracle_cases[1][3][0] == 4


@pytest.mark.parametrize("i", CASES, ids=[f"{i}-{r}x{c}" for i, (r, c) in enumerate(PYRAMID_SHAPES)])
def test_pyramid_bit_equal(matcher, oracle_cases, i):
    img, ok, od, want = oracle_cases[i]
    gk, gd = matcher.sift_detect_compute(img)
    got = matcher.sift_debug_pyramid(0)
    diffs = pyramid_diffs(got, want)
    assert not diffs, f"case {i} {img.shape}: " + "; ".join(diffs[:6]) + (f" (+{len(diffs) - 6} more)" if len(diffs) > 6 else "")
    assert got[3].size == sum(11 * int(r) * int(c) for r, c in zip(want[1], want[2]))
    print(f"case {i} {img.shape}: {want[0]} octaves, {got[3].size} plane floats equal; counters {got[4]}")
    # at these counts compare_sift's 0.2 % allowance is zero keypoints: the lists are identical (order
    # included, which compare_sift's alignment by fields does not look at)
    assert compare_sift(gk, gd, ok, od, f"multi{100 + i}{img.shape}") == 0
    assert np.array_equal(gk, ok) and np.array_equal(gd, od)
    assert got[4][3] == len(gk)


def test_counters(matcher, oracle_cases):
    for i in (0, 6, 11, 18):
        img = oracle_cases[i][0]
        gk, _ = matcher.sift_detect_compute(img)
        cand, raw, surv, final = matcher.sift_debug_pyramid(0)[4]
        assert final == len(gk), (i, final, len(gk))
        assert raw >= final and cand >= surv >= 0, (i, cand, raw, surv, final)
        if i == 6:
            assert (cand, raw, surv, final) == (0, 0, 0, 0)
        if i in (11, 18):
            assert surv > 0 and final >= 90


def test_errors():
    """MIM_EINVAL with a text: before any SIFT call, for an image the call did not have, and for a
    buffer one float short."""
    import ctypes as C

    from computervision_objectdetection_featurematching_amd import Matcher, _lib
    from computervision_objectdetection_featurematching_amd._lib import MimError
    m = Matcher(0)
    try:
        with pytest.raises(MimError) as e:
            m.sift_debug_pyramid(0)
        assert e.value.code == _lib.MIM_EINVAL and m.L.mim_last_error(m.ctx)
        img = pyramid_case(1)
        k, _ = m.sift_detect_compute(img)
        n_oct, orows, ocols, planes, cnt = m.sift_debug_pyramid(0)
        assert n_oct == 4 and cnt[3] == len(k)
        for bad in (1, -1):
            with pytest.raises(MimError) as e:
                m.sift_debug_pyramid(bad)
            assert e.value.code == _lib.MIM_EINVAL and m.L.mim_last_error(m.ctx)
        # one float short: refused, nothing written, the needed size reported
        buf = np.full(planes.size, -7.0, np.float32)
        n, need = C.c_int32(), C.c_int64()
        r16, c16, c4 = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(4, np.int32)
        args = (C.byref(n), C.c_void_p(r16.ctypes.data), C.c_void_p(c16.ctypes.data), C.c_void_p(buf.ctypes.data))
        st = m.L.mim_sift_debug_pyramid(m.ctx, 0, *args, planes.size - 1, C.byref(need), C.c_void_p(c4.ctypes.data))
        assert st == _lib.MIM_EINVAL and len(m.L.mim_last_error(m.ctx)) > 0
        assert need.value == planes.size and np.all(buf == -7.0)
        st = m.L.mim_sift_debug_pyramid(m.ctx, 0, *args, planes.size, C.byref(need), C.c_void_p(c4.ctypes.data))
        assert st == _lib.MIM_OK and np.array_equal(buf.view(np.int32), planes.view(np.int32))
        # an image with no octave: n_oct = 0, nothing to copy
        k, _ = m.sift_detect_compute(np.full((1, 2), 50, np.uint8))
        n_oct, orows, ocols, planes, cnt = m.sift_debug_pyramid(0)
        assert len(k) == 0 and n_oct == 0 and planes.size == 0 and cnt == (0, 0, 0, 0)
    finally:
        m.close()
