"""Python mirror of the reference's hot-path interface, running on the HIP kernels of libmim.so.

Reference call sites (/root/reference/src/TestsDetector.cpp):
  :36,60   BFMatcher(NORM_L2).knnMatch(view_desc, scene_desc, knn, 2)  -> Matcher.knn_match
  :66-72   ratio test `m[0].distance < 0.9f * m[1].distance`           -> Matcher.ratio_filter
  :78      findHomography(objPts, scenePts, RANSAC, 5.0, inlierMask)   -> Matcher.find_homography
  :58-95   the per-view loop with its gates (:74, :79, :81, :84)       -> Matcher.match_batch
  :33      preprocessImage: cvtColor(BGR2GRAY) (preprocessing.cpp:11)  -> Matcher.cvt_bgr2gray
  :102     resize(scene, scaled, Size(), s, s) (INTER_LINEAR)          -> Matcher.resize_linear
  :106     sift->detectAndCompute(scaled, noArray(), kps, desc)        -> Matcher.sift_detect_compute
  (ModelsDetector.cpp:75, the model views with their masks: the same call with a mask)
Argument meaning and error behaviour follow OpenCV: an empty query gives no rows, n < 4 points
raise (CV_Error StsVecLengthErr), a failed RANSAC returns an empty H (None) and a zero mask.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import MimError, Params, Problem, RESULT_DTYPE

DIM = 128
KNN_MAX_K = 16  # MIM_KNN_MAX_K
# cv::KeyPoint without class_id (mim_keypoint in include/mim.h)
KEYPOINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                           ("response", np.float32), ("octave", np.int32)])


def default_params(**kw) -> Params:
    p = Params()
    _lib.load().mim_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@dataclass
class DMatch:  # cv::DMatch
    queryIdx: int
    trainIdx: int
    imgIdx: int
    distance: float


class Matcher:
    """One GPU context (device + HIP stream).  Not a CPU object: construction fails without a GPU."""

    def __init__(self, device: int = 0):
        self.L = _lib.load()
        self._ctx = C.c_void_p()
        st = self.L.mim_ctx_create(device, C.byref(self._ctx))
        if st != _lib.MIM_OK:
            raise MimError(st, f"mim_ctx_create(device={device}) failed (no HIP device?)")
        self.device = device
        self._borrowed = []  # (set id, tensors) the registered sets read until they are dropped (mim.h)
        self._n_sets = 0
        self._set_rows = {}  # set id -> rows, of the sets registered through this object (match_cross_sets)
        self.sets_generation = 0  # bumped whenever registered sets are dropped
        self._retired = []   # (event on the matcher stream, tensors) kept alive until the event completes

    def close(self):
        if self._ctx and (self._borrowed or self._retired):
            self.L.mim_synchronize(self._ctx)
        self._borrowed, self._retired = [], []
        if self._ctx:
            self.L.mim_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int):
        if st != _lib.MIM_OK:
            raise MimError(st, self.L.mim_last_error(self._ctx).decode())

    @property
    def ctx(self):
        return self._ctx

    def set_stream(self, stream_handle: int | None):
        self._check(self.L.mim_ctx_set_stream(self._ctx, C.c_void_p(stream_handle or 0)))

    def stream_handle(self) -> int:
        """The HIP stream this matcher enqueues on (wrap with torch.cuda.ExternalStream)."""
        return int(self.L.mim_ctx_get_stream(self._ctx) or 0)

    def synchronize(self):
        self._check(self.L.mim_synchronize(self._ctx))

    # ---- descriptor sets ------------------------------------------------------------------
    def add_set(self, desc, kp) -> int:
        """Register one ObjectModel view / scene scale.  numpy (host) or torch (device) arrays.

        Device tensors are borrowed, not copied (mim.h): they must be float32, contiguous, shaped
        (n, 128) and (n, 2), on this matcher's device; the matcher keeps them alive until
        clear_sets() and orders its stream after the stream that is current when they are added."""
        on_dev = int(hasattr(desc, "is_cuda") and desc.is_cuda)
        if not on_dev:
            desc = np.ascontiguousarray(desc, np.float32).reshape(-1, DIM)
            kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
        else:
            import torch
            if not (hasattr(kp, "is_cuda") and kp.is_cuda):
                raise ValueError("add_set: keypoints must be on the device when the descriptors are")
            for name, t, cols in (("descriptors", desc, DIM), ("keypoints", kp, 2)):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != cols:
                    raise ValueError(f"add_set: {name} must be a contiguous float32 (n, {cols}) tensor, got "
                                     f"{t.dtype} {tuple(t.shape)} contiguous={t.is_contiguous()}")
                if t.device.index != self.device:
                    raise ValueError(f"add_set: {name} on {t.device}, matcher on cuda:{self.device}")
            if kp.shape[0] != desc.shape[0]:
                raise ValueError("add_set: descriptor and keypoint row counts differ")
            # the producer stream's work (the tensors' contents) before anything on the matcher's stream
            mine = torch.cuda.ExternalStream(self.stream_handle(), device=desc.device)
            cur = torch.cuda.current_stream(desc.device)
            if cur.cuda_stream != mine.cuda_stream:
                mine.wait_stream(cur)
        n = int(desc.shape[0])
        sid = C.c_int32()
        self._check(self.L.mim_set_create(self._ctx, C.c_void_p(_lib.ptr(desc)), C.c_void_p(_lib.ptr(kp)), n,
                                          int(desc.shape[1]), on_dev, C.byref(sid)))
        if on_dev:
            self._borrowed.append((sid.value, [desc, kp]))
        self._n_sets = sid.value + 1
        self._set_rows[sid.value] = int(desc.shape[0])
        return sid.value

    def add_binary_set(self, desc_u8, kp) -> int:
        """Register a set of binary descriptors (mim_set_create_bin): CV_8U rows of 1..64 bytes (ORB 32,
        BRIEF 16/32/64, AKAZE 61, BRISK/FREAK 64) matched with NORM_HAMMING, and their (n, 2) keypoints.

        numpy arrays (uint8 (n, width), any row stride; float32 keypoints), or torch device tensors (uint8
        (n, width) with unit column stride, contiguous float32 (n, 2)).  The rows are copied, never
        borrowed: device tensors may be released once the matcher's stream has passed the copy."""
        on_dev = int(hasattr(desc_u8, "is_cuda") and desc_u8.is_cuda)
        if not on_dev:
            desc = np.asarray(desc_u8)
            if desc.dtype != np.uint8 or desc.ndim != 2:
                raise ValueError(f"add_binary_set: descriptors must be a uint8 (n, width) array, got {desc.dtype} "
                                 f"{desc.shape}")
            if desc.shape[0] <= 1 or desc.strides[1] != 1 or desc.strides[0] < desc.shape[1]:
                desc = np.ascontiguousarray(desc)  # anything but rows of unit-stride bytes a fixed step apart
            kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
            step = int(desc.strides[0]) if desc.shape[0] > 1 else int(desc.shape[1])  # an empty array's stride may be 0
        else:
            import torch
            desc = desc_u8
            if not (hasattr(kp, "is_cuda") and kp.is_cuda):
                raise ValueError("add_binary_set: keypoints must be on the device when the descriptors are")
            if desc.dtype != torch.uint8 or desc.dim() != 2 or (desc.shape[0] > 1 and desc.stride(1) != 1):
                raise ValueError(f"add_binary_set: descriptors must be a uint8 (n, width) tensor with unit column "
                                 f"stride, got {desc.dtype} {tuple(desc.shape)}")
            if kp.dtype != torch.float32 or not kp.is_contiguous() or kp.dim() != 2 or kp.shape[1] != 2:
                raise ValueError(f"add_binary_set: keypoints must be a contiguous float32 (n, 2) tensor, got "
                                 f"{kp.dtype} {tuple(kp.shape)}")
            for name, t in (("descriptors", desc), ("keypoints", kp)):
                if t.device.index != self.device:
                    raise ValueError(f"add_binary_set: {name} on {t.device}, matcher on cuda:{self.device}")
            step = int(desc.stride(0)) if desc.shape[0] > 1 else int(desc.shape[1])
            mine = torch.cuda.ExternalStream(self.stream_handle(), device=desc.device)
            cur = torch.cuda.current_stream(desc.device)
            if cur.cuda_stream != mine.cuda_stream:
                mine.wait_stream(cur)
        if int(kp.shape[0]) != int(desc.shape[0]):
            raise ValueError("add_binary_set: descriptor and keypoint row counts differ")
        sid = C.c_int32()
        self._check(self.L.mim_set_create_bin(self._ctx, C.c_void_p(_lib.ptr(desc)), step, C.c_void_p(_lib.ptr(kp)),
                                              int(desc.shape[0]), int(desc.shape[1]), on_dev, C.byref(sid)))
        if on_dev:
            # copied on the matcher's stream: kept until that stream has passed the copy
            ev = torch.cuda.Event()
            ev.record(mine)
            self._retired.append((ev, [desc, kp]))
        self._n_sets = sid.value + 1
        self._set_rows[sid.value] = int(desc.shape[0])
        return sid.value

    def add_float_set(self, desc, kp) -> int:
        """Register a set of float descriptors of any dimension 1..512 (mim_set_create_f32): the CV_32F rows
        BFMatcher(NORM_L2) matches (SURF/KAZE 64, VGG, DAISY 200, SuperPoint 256, D2-Net 512, and 128-D rows
        that are not integers: RootSIFT, HardNet), and their (n, 2) keypoints.

        numpy arrays (float32 (n, dim), any row stride that is a multiple of 4 bytes; float32 keypoints), or
        torch device tensors (float32 (n, dim) with unit column stride, contiguous float32 (n, 2)).  The rows
        are copied, never borrowed: device tensors may be released once the matcher's stream has passed the
        copy."""
        on_dev = int(hasattr(desc, "is_cuda") and desc.is_cuda)
        if not on_dev:
            desc = np.asarray(desc)
            if desc.dtype != np.float32 or desc.ndim != 2:
                raise ValueError(f"add_float_set: descriptors must be a float32 (n, dim) array, got {desc.dtype} "
                                 f"{desc.shape}")
            if desc.shape[0] <= 1 or desc.strides[1] != 4 or desc.strides[0] < 4 * desc.shape[1] or desc.strides[0] % 4:
                desc = np.ascontiguousarray(desc)  # anything but rows of unit-stride floats a fixed step apart
            kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
            step = int(desc.strides[0]) if desc.shape[0] > 1 else 4 * int(desc.shape[1])
        else:
            import torch
            if not (hasattr(kp, "is_cuda") and kp.is_cuda):
                raise ValueError("add_float_set: keypoints must be on the device when the descriptors are")
            if desc.dtype != torch.float32 or desc.dim() != 2 or (desc.numel() > 1 and desc.shape[1] > 1 and desc.stride(1) != 1):
                raise ValueError(f"add_float_set: descriptors must be a float32 (n, dim) tensor with unit column "
                                 f"stride, got {desc.dtype} {tuple(desc.shape)}")
            if kp.dtype != torch.float32 or not kp.is_contiguous() or kp.dim() != 2 or kp.shape[1] != 2:
                raise ValueError(f"add_float_set: keypoints must be a contiguous float32 (n, 2) tensor, got "
                                 f"{kp.dtype} {tuple(kp.shape)}")
            for name, t in (("descriptors", desc), ("keypoints", kp)):
                if t.device.index != self.device:
                    raise ValueError(f"add_float_set: {name} on {t.device}, matcher on cuda:{self.device}")
            step = 4 * (int(desc.stride(0)) if desc.shape[0] > 1 else int(desc.shape[1]))
            mine = torch.cuda.ExternalStream(self.stream_handle(), device=desc.device)
            cur = torch.cuda.current_stream(desc.device)
            if cur.cuda_stream != mine.cuda_stream:
                mine.wait_stream(cur)
        if int(kp.shape[0]) != int(desc.shape[0]):
            raise ValueError("add_float_set: descriptor and keypoint row counts differ")
        sid = C.c_int32()
        self._check(self.L.mim_set_create_f32(self._ctx, C.c_void_p(_lib.ptr(desc)), step, C.c_void_p(_lib.ptr(kp)),
                                              int(desc.shape[0]), int(desc.shape[1]), on_dev, C.byref(sid)))
        if on_dev:
            # copied on the matcher's stream: kept until that stream has passed the copy
            ev = torch.cuda.Event()
            ev.record(mine)
            self._retired.append((ev, [desc, kp]))
        self._n_sets = sid.value + 1
        self._set_rows[sid.value] = int(desc.shape[0])
        return sid.value

    def add_sets(self, pairs) -> list[int]:
        """Register several sets in one library call (mim_sets_create), as add_set in order: every pair
        (desc, kp) numpy (host) or every pair torch (device), the same rules per pair; all or nothing."""
        pairs = list(pairs)
        if not pairs:
            return []
        on_dev = int(hasattr(pairs[0][0], "is_cuda") and pairs[0][0].is_cuda)
        descs, kps = [], []
        if on_dev:
            import torch
            for desc, kp in pairs:
                for name, t, cols in (("descriptors", desc, DIM), ("keypoints", kp, 2)):
                    if not (hasattr(t, "is_cuda") and t.is_cuda):
                        raise ValueError("add_sets: every array must be on the device when the first is")
                    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != cols:
                        raise ValueError(f"add_sets: {name} must be a contiguous float32 (n, {cols}) tensor, got "
                                         f"{t.dtype} {tuple(t.shape)} contiguous={t.is_contiguous()}")
                    if t.device.index != self.device:
                        raise ValueError(f"add_sets: {name} on {t.device}, matcher on cuda:{self.device}")
                if kp.shape[0] != desc.shape[0]:
                    raise ValueError("add_sets: descriptor and keypoint row counts differ")
                descs.append(desc)
                kps.append(kp)
            dev = descs[0].device
            mine = torch.cuda.ExternalStream(self.stream_handle(), device=dev)
            cur = torch.cuda.current_stream(dev)
            if cur.cuda_stream != mine.cuda_stream:
                mine.wait_stream(cur)
        else:
            for desc, kp in pairs:
                if hasattr(desc, "is_cuda") and desc.is_cuda:
                    raise ValueError("add_sets: host and device arrays mixed")
                descs.append(np.ascontiguousarray(desc, np.float32).reshape(-1, DIM))
                kps.append(np.ascontiguousarray(kp, np.float32).reshape(-1, 2))
                if kps[-1].shape[0] != descs[-1].shape[0]:
                    raise ValueError("add_sets: descriptor and keypoint row counts differ")
        n = len(pairs)
        dp = (C.c_void_p * n)(*[_lib.ptr(d) for d in descs])
        kpp = (C.c_void_p * n)(*[_lib.ptr(k) for k in kps])
        rows = np.array([int(d.shape[0]) for d in descs], np.int32)
        first = C.c_int32()
        self._check(self.L.mim_sets_create(self._ctx, n, dp, kpp, C.c_void_p(_lib.ptr(rows)), DIM, on_dev, C.byref(first)))
        ids = list(range(first.value, first.value + n))
        if on_dev:
            for sid, d, k in zip(ids, descs, kps):
                self._borrowed.append((sid, [d, k]))
        self._n_sets = first.value + n
        self._set_rows.update(zip(ids, (int(r) for r in rows)))
        return ids

    @property
    def n_sets(self) -> int:
        return self._n_sets

    def _retire(self, keep: int):
        # the dropped sets' tensors stay referenced until the work already enqueued on the matcher's
        # stream (their last readers) has completed: an event per drop, polled at the next drops
        # (not record_stream: the allocator would later record events on this stream after close())
        self._retired = [(ev, ts) for ev, ts in self._retired if not ev.query()]
        gone = [ts for sid, ts in self._borrowed if sid >= keep]
        if gone:
            import torch
            ev = torch.cuda.Event()
            ev.record(torch.cuda.ExternalStream(self.stream_handle(), device=gone[0][0].device))
            self._retired.append((ev, gone))
        self._borrowed = [(sid, ts) for sid, ts in self._borrowed if sid < keep]
        self._n_sets = min(self._n_sets, keep)
        self._set_rows = {sid: r for sid, r in self._set_rows.items() if sid < keep}
        self.sets_generation += 1

    def clear_sets(self):
        self._check(self.L.mim_sets_clear(self._ctx))
        self._retire(0)

    def truncate_sets(self, n_keep: int):
        """Drop the sets registered after the first n_keep (mim_sets_truncate); ids < n_keep stay."""
        self._check(self.L.mim_sets_truncate(self._ctx, int(n_keep)))
        self._retire(int(n_keep))

    # ---- primitives -----------------------------------------------------------------------
    @staticmethod
    def _check_k(k) -> int:
        if int(k) != k or not 1 <= k <= KNN_MAX_K:
            raise ValueError(f"knnMatch: k must be an integer in 1..{KNN_MAX_K} (got {k!r})")
        return int(k)

    @staticmethod
    def _dmatches(idx, dist):
        """knnMatch's list of lists from (nq, k) arrays: absent entries (index -1) are dropped."""
        return [[DMatch(i, int(idx[i, j]), 0, float(dist[i, j])) for j in range(idx.shape[1]) if idx[i, j] >= 0]
                for i in range(idx.shape[0])]

    def knn_match_arrays(self, query, train, k: int = 2):
        """knnMatch(query, train, k) as arrays: idx (nq, k) int32 (-1 absent), dist (nq, k) float32.
        k = 2 is the MFMA path of mim_knn2_l2; any other k in 1..16 is mim_knn_l2."""
        k = self._check_k(k)
        q = np.ascontiguousarray(query, np.float32).reshape(-1, DIM)
        t = np.ascontiguousarray(train, np.float32).reshape(-1, DIM)
        nq = q.shape[0]
        idx = np.full((max(nq, 1), k), -1, np.int32)
        dist = np.zeros((max(nq, 1), k), np.float32)
        if k == 2:
            self._check(self.L.mim_knn2_l2(self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data),
                                           t.shape[0], DIM, C.c_void_p(idx.ctypes.data), C.c_void_p(dist.ctypes.data)))
        else:
            self._check(self.L.mim_knn_l2(self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data),
                                          t.shape[0], DIM, k, C.c_void_p(idx.ctypes.data),
                                          C.c_void_p(dist.ctypes.data)))
        return idx[:nq], dist[:nq]

    def knn_match(self, query, train, k: int = 2):
        """BFMatcher(NORM_L2).knnMatch(query, train, matches, k), k in 1..16 -> list of lists of DMatch."""
        return self._dmatches(*self.knn_match_arrays(query, train, k))

    def knn_match_hamming_arrays(self, query, train, k: int = 2):
        """BFMatcher(NORM_HAMMING).knnMatch(query, train, k), k in 1..16, on uint8 rows of one width (1..64
        bytes), as arrays: idx (nq, k) int32 (-1 absent), dist (nq, k) float32 (the integer distances)."""
        k = self._check_k(k)
        q, t = np.asarray(query), np.asarray(train)
        if q.dtype != np.uint8 or t.dtype != np.uint8 or q.ndim != 2 or t.ndim != 2:
            raise ValueError("knn_match_hamming: uint8 (n, width) arrays are required")
        if q.shape[1] != t.shape[1]:
            raise ValueError(f"knn_match_hamming: query rows of {q.shape[1]} bytes, train rows of {t.shape[1]}")
        q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        nq = q.shape[0]
        idx = np.full((max(nq, 1), k), -1, np.int32)
        dist = np.zeros((max(nq, 1), k), np.float32)
        if k == 2:
            self._check(self.L.mim_knn2_hamming(self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data),
                                                t.shape[0], q.shape[1], C.c_void_p(idx.ctypes.data),
                                                C.c_void_p(dist.ctypes.data)))
        else:
            self._check(self.L.mim_knn_hamming(self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data),
                                               t.shape[0], q.shape[1], k, C.c_void_p(idx.ctypes.data),
                                               C.c_void_p(dist.ctypes.data)))
        return idx[:nq], dist[:nq]

    def knn_match_hamming(self, query, train, k: int = 2):
        """BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, k), k in 1..16 -> list of lists of DMatch."""
        return self._dmatches(*self.knn_match_hamming_arrays(query, train, k))

    def knn_match_float_arrays(self, query, train, k: int = 2):
        """BFMatcher(NORM_L2).knnMatch(query, train, k), k in 1..16, on float32 rows of one dim 1..512
        (mim_knn2_l2_f32 at k = 2, else mim_knn_l2), as arrays: idx (nq, k) int32 (-1 absent), dist (nq, k)
        float32."""
        k = self._check_k(k)
        q, t = np.asarray(query), np.asarray(train)
        if q.dtype != np.float32 or t.dtype != np.float32 or q.ndim != 2 or t.ndim != 2:
            raise ValueError("knn_match_float: float32 (n, dim) arrays are required")
        if q.shape[1] != t.shape[1]:
            raise ValueError(f"knn_match_float: query rows of dim {q.shape[1]}, train rows of dim {t.shape[1]}")
        q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        nq = q.shape[0]
        idx = np.full((max(nq, 1), k), -1, np.int32)
        dist = np.zeros((max(nq, 1), k), np.float32)
        if k == 2:
            self._check(self.L.mim_knn2_l2_f32(self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data),
                                               t.shape[0], q.shape[1], C.c_void_p(idx.ctypes.data),
                                               C.c_void_p(dist.ctypes.data)))
        else:
            self._check(self.L.mim_knn_l2(self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data),
                                          t.shape[0], q.shape[1], k, C.c_void_p(idx.ctypes.data),
                                          C.c_void_p(dist.ctypes.data)))
        return idx[:nq], dist[:nq]

    def knn_match_float(self, query, train, k: int = 2):
        """BFMatcher(NORM_L2).knnMatch(query, train, matches, k), k in 1..16, on float rows of any dim -> lists of
        DMatch."""
        return self._dmatches(*self.knn_match_float_arrays(query, train, k))

    # ---- feature extraction either side of the matcher (ModelsDetector.cpp:75, TestsDetector.cpp:102,106)
    def sift_detect_compute(self, gray, mask=None, max_kp: int = 1 << 18):
        """SIFT::create()->detectAndCompute(gray, mask, kps, desc) on the GPU.

        gray / mask: CV_8UC1 arrays (rows, cols).  Returns (keypoints as a KEYPOINT_DTYPE array,
        descriptors (n, 128) float32).  More than max_kp keypoints raises (no silent truncation)."""
        g = np.ascontiguousarray(gray, np.uint8)
        if g.ndim != 2:
            raise ValueError("sift_detect_compute: a single-channel image is required")
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.shape != g.shape:
                raise ValueError("sift_detect_compute: mask must have the image's size")
        kps = np.zeros(max(max_kp, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(max_kp, 1), DIM), np.float32)
        n = C.c_int32()
        self._check(self.L.mim_sift_detect_compute(
            self._ctx, C.c_void_p(g.ctypes.data), g.shape[0], g.shape[1], g.strides[0],
            None if m is None else C.c_void_p(m.ctypes.data), 0 if m is None else m.strides[0], max_kp,
            C.c_void_p(kps.ctypes.data), C.c_void_p(desc.ctypes.data), C.byref(n)))
        if n.value > max_kp:
            raise ValueError(f"sift_detect_compute: {n.value} keypoints > max_kp={max_kp}")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def sift_detect_compute_scales(self, gray, scales, max_kp: int = 1 << 20):
        """resize(gray, Size(), s, s, INTER_LINEAR) + detectAndCompute at every scale in one call
        (TestsDetector.cpp:99-107).  Returns [(keypoints, descriptors)] per scale, identical to
        resize_linear + sift_detect_compute scale by scale."""
        g = np.ascontiguousarray(gray, np.uint8)
        if g.ndim != 2:
            raise ValueError("sift_detect_compute_scales: a single-channel image is required")
        sc = np.ascontiguousarray(scales, np.float32).reshape(-1)
        kps = np.zeros(max(max_kp, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(max_kp, 1), DIM), np.float32)
        n = np.zeros(len(sc), np.int32)
        self._check(self.L.mim_sift_detect_compute_scales(
            self._ctx, C.c_void_p(g.ctypes.data), g.shape[0], g.shape[1], g.strides[0], len(sc),
            C.c_void_p(sc.ctypes.data), max_kp, C.c_void_p(kps.ctypes.data), C.c_void_p(desc.ctypes.data),
            C.c_void_p(n.ctypes.data)))
        out, o = [], 0
        for c in n:
            out.append((kps[o:o + c].copy(), desc[o:o + c].copy()))
            o += int(c)
        return out

    def sift_debug_pyramid(self, image_index: int = 0):
        """Test support (mim_sift_debug_pyramid): the pyramid the last SIFT call on this matcher left in
        its workspace for image `image_index` (0 after sift_detect_compute, the scale index after
        sift_detect_compute_scales).  Returns (n_oct, orows[16], ocols[16], planes, counters): planes is
        the flat float32 buffer, per octave 6 Gaussian then 5 DoG layers, each dense row-major;
        counters = (candidates, raw keypoints, survivors, final keypoints)."""
        n_oct, need = C.c_int32(), C.c_int64()
        orows, ocols, cnt = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(4, np.int32)
        args = (C.byref(n_oct), C.c_void_p(orows.ctypes.data), C.c_void_p(ocols.ctypes.data))
        self._check(self.L.mim_sift_debug_pyramid(self._ctx, image_index, *args, None, 0, C.byref(need),
                                                  C.c_void_p(cnt.ctypes.data)))
        planes = np.zeros(max(need.value, 1), np.float32)
        self._check(self.L.mim_sift_debug_pyramid(self._ctx, image_index, *args, C.c_void_p(planes.ctypes.data),
                                                  need.value, C.byref(need), C.c_void_p(cnt.ctypes.data)))
        return n_oct.value, orows, ocols, planes[:need.value], tuple(int(v) for v in cnt)

    def cvt_bgr2gray(self, bgr):
        """cv::cvtColor(bgr, gray, COLOR_BGR2GRAY) of an H x W x 3 uint8 image (preprocessImage,
        preprocessing.cpp:11) on the device: (R * 4899 + G * 9617 + B * 1868 + (1 << 13)) >> 14."""
        b = np.asarray(bgr)
        if b.dtype != np.uint8 or b.ndim != 3 or b.shape[2] != 3:
            raise ValueError("cvt_bgr2gray: an H x W x 3 uint8 image (B, G, R) is required")
        if b.strides[2] != 1 or b.strides[1] != 3 or b.strides[0] < 3 * b.shape[1]:
            b = np.ascontiguousarray(b)
        out = np.zeros(b.shape[:2], np.uint8)
        self._check(self.L.mim_cvt_bgr2gray_u8(self._ctx, C.c_void_p(b.ctypes.data), b.shape[0], b.shape[1],
                                               b.strides[0], C.c_void_p(out.ctypes.data)))
        return out

    def sift_scales_to_sets(self, gray, scales, keypoints: bool = False, max_kp: int = 1 << 20):
        """resize + detectAndCompute at every scale (TestsDetector.cpp:99-107) with the descriptors left
        on the device, each scale registered as a set (mim_sift_scales_sets).  `gray` is an H x W uint8
        image, or an H x W x 3 one in B, G, R order (what cv::imread gives), converted to gray on the
        device first (preprocessing.cpp:11, mim_sift_scales_sets_image).  Returns (set ids, n_kp
        per scale, [keypoints per scale] or None); the sets' rows are what sift_detect_compute_scales
        returns, without the round trip through host memory.  With keypoints=True and more than max_kp
        keypoints in all, this call's sets are dropped and the call made again with room for all."""
        g = np.ascontiguousarray(gray, np.uint8)
        if g.ndim not in (2, 3):
            raise ValueError("sift_scales_to_sets: an H x W (gray) or H x W x 3 (BGR) image is required")
        sc = np.ascontiguousarray(scales, np.float32).reshape(-1)
        ids = np.zeros(len(sc), np.int32)
        n = np.zeros(len(sc), np.int32)
        kps = np.zeros(max(max_kp, 1), KEYPOINT_DTYPE) if keypoints else None
        before = self.sets_info()[0]
        if g.ndim == 2:
            st = self.L.mim_sift_scales_sets(
                self._ctx, C.c_void_p(g.ctypes.data), g.shape[0], g.shape[1], g.strides[0], len(sc),
                C.c_void_p(sc.ctypes.data), C.c_void_p(ids.ctypes.data), C.c_void_p(n.ctypes.data),
                max_kp if keypoints else 0, C.c_void_p(kps.ctypes.data) if keypoints else None)
        else:  # the channel count is the library's to check (MIM_EINVAL unless 3)
            img = _lib.Image(C.c_void_p(g.ctypes.data), g.shape[0], g.shape[1], g.shape[2], g.strides[0])
            st = self.L.mim_sift_scales_sets_image(
                self._ctx, C.byref(img), len(sc), C.c_void_p(sc.ctypes.data), C.c_void_p(ids.ctypes.data),
                C.c_void_p(n.ctypes.data), max_kp if keypoints else 0,
                C.c_void_p(kps.ctypes.data) if keypoints else None)
        # the context's set count, whatever happened (MIM_ERANGE for a short host keypoint buffer comes
        # after the sets were registered)
        self._n_sets = self.sets_info()[0]
        if st == _lib.MIM_ERANGE and keypoints and self._n_sets == before + len(sc) and int(n.sum()) > max_kp:
            self.truncate_sets(before)  # drop this call's sets, run again with room for all
            return self.sift_scales_to_sets(gray, scales, True, int(n.sum()))
        self._check(st)
        out = None
        if keypoints:
            out, o = [], 0
            for c in n:
                out.append(kps[o:o + c].copy())
                o += int(c)
        return [int(i) for i in ids], [int(c) for c in n], out

    def sets_info(self):
        """(registered set count, sets generation) of the context (mim_sets_info)."""
        n, gen = C.c_int32(), C.c_int64()
        self._check(self.L.mim_sets_info(self._ctx, C.byref(n), C.byref(gen)))
        return n.value, gen.value

    def set_rows(self, set_id: int):
        """The descriptor rows (n, 128) float32 and keypoint positions (n, 2) of a registered set as the
        kernels read them (mim_set_rows; a debug/test copy-out, e.g. of mim_sift_scales_sets' sets)."""
        n = C.c_int32()
        self._check(self.L.mim_set_rows(self._ctx, int(set_id), 0, None, None, C.byref(n)))
        desc = np.zeros((n.value, DIM), np.float32)
        kp = np.zeros((n.value, 2), np.float32)
        if n.value:
            self._check(self.L.mim_set_rows(self._ctx, int(set_id), n.value, C.c_void_p(desc.ctypes.data),
                                            C.c_void_p(kp.ctypes.data), C.byref(n)))
        return desc, kp

    def resize_linear(self, src, dsize=None, fx: float = 0.0, fy: float = 0.0):
        """cv::resize(src, dst, dsize, fx, fy, INTER_LINEAR) of a CV_8UC1 image.

        dsize = (width, height), or None with fx (and fy, default fx) > 0 as the reference calls it:
        resize(scene, scaled, Size(), scale, scale) with a float scale (TestsDetector.cpp:99-102)."""
        s = np.ascontiguousarray(src, np.uint8)
        if dsize is None:
            if not fx > 0:
                raise ValueError("resize_linear: dsize or fx > 0 required")
            fx = float(np.float32(fx))
            fy = float(np.float32(fy)) if fy else fx
            dcols, drows = int(np.rint(s.shape[1] * fx)), int(np.rint(s.shape[0] * fy))
        else:
            dcols, drows = int(dsize[0]), int(dsize[1])
            fx = fy = 0.0
        dst = np.zeros((max(drows, 1), max(dcols, 1)), np.uint8)
        self._check(self.L.mim_resize_linear_u8(self._ctx, C.c_void_p(s.ctypes.data), s.shape[0], s.shape[1],
                                                s.strides[0], C.c_void_p(dst.ctypes.data), drows, dcols, fx, fy))
        return dst

    def ratio_filter(self, idx, dist, ratio: float = 0.9):
        idx = np.ascontiguousarray(idx, np.int32)
        dist = np.ascontiguousarray(dist, np.float32)
        nq = idx.shape[0]
        qo = np.zeros(max(nq, 1), np.int32)
        to = np.zeros(max(nq, 1), np.int32)
        ng = C.c_int32()
        self._check(self.L.mim_ratio_filter(self._ctx, C.c_void_p(idx.ctypes.data), C.c_void_p(dist.ctypes.data),
                                            nq, ratio, C.c_void_p(qo.ctypes.data), C.c_void_p(to.ctypes.data),
                                            C.byref(ng)))
        return qo[:ng.value], to[:ng.value]

    def find_homography(self, src, dst, thresh: float = 5.0, max_iters: int = 2000, confidence: float = 0.995):
        """cv::findHomography(src, dst, RANSAC, thresh, mask, max_iters, confidence) -> (H or None, mask)."""
        src = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        n = src.shape[0]
        if n < 4 or dst.shape[0] != n:
            raise ValueError("The input arrays should have at least 4 corresponding point sets to calculate Homography")
        H = np.zeros(9, np.float64)
        mask = np.zeros(n, np.uint8)
        st = self.L.mim_find_homography(self._ctx, C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data), n,
                                        thresh, max_iters, confidence, C.c_void_p(H.ctypes.data),
                                        C.c_void_p(mask.ctypes.data))
        if st == _lib.MIM_ENOMODEL:
            return None, mask
        self._check(st)
        return H.reshape(3, 3), mask

    # ---- fused batch ----------------------------------------------------------------------
    FILTERS = {"ratio": 0, "cross": 1, "ratio+cross": 2}  # MIM_FILTER_* (mim_batch_run_filter)

    def match_batch_async(self, problems, params: Params | None = None, filter: str = "ratio"):
        """Enqueue one batch.  filter: "ratio" (Lowe's ratio test, mim_batch_run), "cross" (mutual nearest
        neighbours, BFMatcher(norm, crossCheck=True).match; params.ratio is ignored) or "ratio+cross" (both)."""
        if filter not in self.FILTERS:
            raise ValueError(f"match_batch: filter must be one of {sorted(self.FILTERS)}, got {filter!r}")
        params = params or default_params()
        # an (n, 2) int32 array is mim_problem[n] as it is (no per-problem ctypes objects: ~1 us each)
        arr = problems if isinstance(problems, np.ndarray) else np.asarray(list(problems), np.int32)
        arr = np.ascontiguousarray(arr, np.int32).reshape(-1, 2)
        if filter == "ratio":
            self._check(self.L.mim_batch_run(self._ctx, arr.ctypes.data_as(C.POINTER(Problem)), len(arr),
                                             C.byref(params)))
        else:
            self._check(self.L.mim_batch_run_filter(self._ctx, arr.ctypes.data_as(C.POINTER(Problem)), len(arr),
                                                    C.byref(params), self.FILTERS[filter]))
        return len(arr)

    def batch_results(self, n: int) -> np.ndarray:
        """Waits for the last batch and returns its n records (n must be the batch's problem count;
        n = 0 only waits and collects the kernel timings)."""
        out = np.zeros(n, RESULT_DTYPE)
        self._check(self.L.mim_batch_results(self._ctx, C.c_void_p(out.ctypes.data if n else 0)))
        return out

    def batch_results_copy_to(self, dst_dev):
        """Async device-to-device copy of the last batch's records (for an RCCL gather)."""
        self._check(self.L.mim_batch_results_copy(self._ctx, C.c_void_p(_lib.ptr(dst_dev)), 1))

    def batch_results_dev_ptr(self) -> int:
        return int(self.L.mim_batch_results_dev(self._ctx) or 0)

    def problem_detail(self, i: int, n_good: int):
        q = np.zeros(max(n_good, 1), np.int32)
        t = np.zeros(max(n_good, 1), np.int32)
        m = np.zeros(max(n_good, 1), np.uint8)
        self._check(self.L.mim_batch_problem_detail(self._ctx, i, C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data),
                                                    C.c_void_p(m.ctypes.data)))
        return q[:n_good], t[:n_good], m[:n_good]

    def batch_inlier_points(self, n: int, scales=None):
        """allUnfilteredScenePts of the last batch (mim_batch_inlier_points, TestsDetector.cpp:87-94):
        (offsets (n + 1,) int64, points (offsets[n], 2) float32); problem i's inlier scene points, divided
        by scales[i] when it is not 1, are points[offsets[i]:offsets[i + 1]]."""
        offs = np.zeros(n + 1, np.int64)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        if sc is not None and sc.shape != (n,):
            raise ValueError(f"batch_inlier_points: {sc.shape} scales for {n} problems")
        scp = None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_float))
        op = offs.ctypes.data_as(C.POINTER(C.c_int64))
        # one call into a kept buffer (one wait, one gather); a larger total comes back as MIM_ERANGE with
        # the offsets set, and the call is made again with room for all
        buf = getattr(self, "_inl_buf", None)
        if buf is None:
            buf = self._inl_buf = np.zeros((1 << 16, 2), np.float32)
        st = self.L.mim_batch_inlier_points(self._ctx, scp, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.shape[0], op)
        total = int(offs[n])
        if st == _lib.MIM_ERANGE and total > buf.shape[0]:
            buf = self._inl_buf = np.zeros((2 * total, 2), np.float32)
            st = self.L.mim_batch_inlier_points(self._ctx, scp, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.shape[0], op)
        self._check(st)
        return offs, buf[:total].copy()

    def match_batch(self, problems, params: Params | None = None, filter: str = "ratio") -> np.ndarray:
        n = self.match_batch_async(problems, params, filter)
        return self.batch_results(n)

    def match_cross_sets(self, qset: int, tset: int, nq: int | None = None):
        """BFMatcher(norm, crossCheck=True).match on two registered sets of one kind (mim_match_cross_sets):
        (idx int32[nq], dist float32[nq]), idx[i] the train row matched to query i or -1, dist[i] its distance
        or FLT_MAX.  nq: the query set's rows, needed only for a set this object did not register itself."""
        if nq is None:
            nq = self._set_rows.get(int(qset))
        if nq is None:
            raise ValueError(f"match_cross_sets: the row count of set {qset} is not known here: pass nq")
        idx = np.full(max(nq, 1), -1, np.int32)
        dist = np.zeros(max(nq, 1), np.float32)
        self._check(self.L.mim_match_cross_sets(self._ctx, int(qset), int(tset), C.c_void_p(idx.ctypes.data),
                                                C.c_void_p(dist.ctypes.data)))
        return idx[:nq], dist[:nq]

    def knn_sets_dev(self, qset: int, tset: int, idx_dev, dist_dev, k: int = 2):
        """knnMatch rows of two registered sets into device buffers of k * nq entries, asynchronous: k = 2 is
        mim_knn2_sets_dev, any other k in 1..16 mim_knn_sets_dev."""
        k = self._check_k(k)
        if k == 2:
            self._check(self.L.mim_knn2_sets_dev(self._ctx, qset, tset, C.c_void_p(_lib.ptr(idx_dev)),
                                                 C.c_void_p(_lib.ptr(dist_dev))))
        else:
            self._check(self.L.mim_knn_sets_dev(self._ctx, int(qset), int(tset), k, C.c_void_p(_lib.ptr(idx_dev)),
                                                C.c_void_p(_lib.ptr(dist_dev))))

    def knn_batch_dev(self, problems, k: int, idx_dev, dist_dev):
        """mim_knn_batch_dev: the k nearest rows of every problem (query set, train set) of any mix of kinds in
        one asynchronous call; problem i's rows start at entry k * (rows of the query sets before it) of the
        device buffers.  Every k in 1..16 runs the top-k kernels here, k = 2 included."""
        k = self._check_k(k)
        arr = problems if isinstance(problems, np.ndarray) else np.asarray(list(problems), np.int32)
        arr = np.ascontiguousarray(arr, np.int32).reshape(-1, 2)
        self._check(self.L.mim_knn_batch_dev(self._ctx, arr.ctypes.data_as(C.POINTER(Problem)), len(arr), k,
                                             C.c_void_p(_lib.ptr(idx_dev)), C.c_void_p(_lib.ptr(dist_dev))))

    # ---- knnMatch over a train collection ---------------------------------------
    def knn_collection_dev(self, query_sets, train_sets, k: int, idx_dev, img_dev, dist_dev):
        """mim_knn_collection_dev: every query set against the collection train_sets (image j = train_sets[j]), the k
        nearest rows over all images per query row, asynchronous; query set i's rows start at entry
        k * (rows of the query sets before it) of the three device buffers (trainIdx, imgIdx, distance)."""
        k = self._check_k(k)
        qs = np.ascontiguousarray(np.asarray(list(query_sets), np.int32).reshape(-1))
        ts = np.ascontiguousarray(np.asarray(list(train_sets), np.int32).reshape(-1))
        self._check(self.L.mim_knn_collection_dev(self._ctx, C.c_void_p(qs.ctypes.data), len(qs), C.c_void_p(ts.ctypes.data),
                                                  len(ts), k, C.c_void_p(_lib.ptr(idx_dev)), C.c_void_p(_lib.ptr(img_dev)),
                                                  C.c_void_p(_lib.ptr(dist_dev))))

    def knn_match_collection(self, query_set: int, train_sets, k: int = 2, nq: int | None = None):
        """BFMatcher::add(views) + knnMatch(query, matches, k) on registered sets -> per query row a list of DMatch
        with imgIdx filled (absent entries dropped).  nq: the query set's rows, needed only for a set this object
        did not register itself."""
        import torch
        k = self._check_k(k)
        if nq is None:
            nq = self._set_rows.get(int(query_set))
        if nq is None:
            raise ValueError(f"knn_match_collection: the row count of set {query_set} is not known here: pass nq")
        dev = torch.device("cuda", self.device)
        idx = torch.full((max(nq, 1), k), -1, dtype=torch.int32, device=dev)
        img = torch.full((max(nq, 1), k), -1, dtype=torch.int32, device=dev)
        dist = torch.zeros((max(nq, 1), k), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the fills, before the matcher's stream writes
        self.knn_collection_dev([int(query_set)], train_sets, k, idx, img, dist)
        self.synchronize()
        idx, img, dist = idx.cpu().numpy()[:nq], img.cpu().numpy()[:nq], dist.cpu().numpy()[:nq]
        return [[DMatch(i, int(idx[i, j]), int(img[i, j]), float(dist[i, j])) for j in range(k) if idx[i, j] >= 0]
                for i in range(nq)]

    # ---- radiusMatch ----------------------------------------------------------
    @staticmethod
    def _check_radius(max_distance) -> float:
        r = float(np.float32(max_distance))
        if not r > float(np.finfo(np.float32).eps):  # DescriptorMatcher::radiusMatch's CV_Assert; a NaN fails
            raise ValueError(f"radiusMatch: maxDistance must be above FLT_EPSILON (got {max_distance!r})")
        return r

    def _radius_host(self, fn, q, t, max_distance):
        """Offsets first (idx NULL), then the lists into buffers of exactly that size."""
        r = self._check_radius(max_distance)
        nq = q.shape[0]
        offsets = np.zeros(nq + 1, np.int64)
        args = (self._ctx, C.c_void_p(q.ctypes.data), nq, C.c_void_p(t.ctypes.data), t.shape[0], q.shape[1], r,
                C.c_void_p(offsets.ctypes.data))
        self._check(fn(*args, None, None, 0))
        total = int(offsets[nq])
        idx, dist = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.float32)
        if total:
            self._check(fn(*args, C.c_void_p(idx.ctypes.data), C.c_void_p(dist.ctypes.data), total))
        return offsets, idx[:total], dist[:total]

    @staticmethod
    def _radius_dmatches(offsets, idx, dist):
        """radiusMatch's list of lists from the CSR arrays."""
        return [[DMatch(i, int(idx[j]), 0, float(dist[j])) for j in range(int(offsets[i]), int(offsets[i + 1]))]
                for i in range(len(offsets) - 1)]

    def radius_match_arrays(self, query, train, max_distance):
        """BFMatcher(NORM_L2).radiusMatch(query, train, maxDistance) on 128-D float rows as CSR arrays (mim_radius_l2
        at dim 128: integer-valued rows on the i8 MFMA kernel): offsets int64 (nq + 1), idx int32, dist float32,
        query i's matches at [offsets[i], offsets[i + 1]), ascending in (distance, train index)."""
        q = np.ascontiguousarray(query, np.float32).reshape(-1, DIM)
        t = np.ascontiguousarray(train, np.float32).reshape(-1, DIM)
        return self._radius_host(self.L.mim_radius_l2, q, t, max_distance)

    def radius_match(self, query, train, max_distance):
        """BFMatcher(NORM_L2).radiusMatch(query, train, matches, maxDistance) -> list of lists of DMatch."""
        return self._radius_dmatches(*self.radius_match_arrays(query, train, max_distance))

    def radius_match_hamming_arrays(self, query, train, max_distance):
        """BFMatcher(NORM_HAMMING).radiusMatch on uint8 rows of one width (1..64 bytes) as CSR arrays
        (mim_radius_hamming); outputs as radius_match_arrays."""
        q, t = np.asarray(query), np.asarray(train)
        if q.dtype != np.uint8 or t.dtype != np.uint8 or q.ndim != 2 or t.ndim != 2:
            raise ValueError("radius_match_hamming: uint8 (n, width) arrays are required")
        if q.shape[1] != t.shape[1]:
            raise ValueError(f"radius_match_hamming: query rows of {q.shape[1]} bytes, train rows of {t.shape[1]}")
        return self._radius_host(self.L.mim_radius_hamming, np.ascontiguousarray(q), np.ascontiguousarray(t), max_distance)

    def radius_match_hamming(self, query, train, max_distance):
        """BFMatcher(NORM_HAMMING).radiusMatch(query, train, matches, maxDistance) -> list of lists of DMatch."""
        return self._radius_dmatches(*self.radius_match_hamming_arrays(query, train, max_distance))

    def radius_match_float_arrays(self, query, train, max_distance):
        """BFMatcher(NORM_L2).radiusMatch on float32 rows of one dim 1..512 as CSR arrays (mim_radius_l2); outputs
        as radius_match_arrays."""
        q, t = np.asarray(query), np.asarray(train)
        if q.dtype != np.float32 or t.dtype != np.float32 or q.ndim != 2 or t.ndim != 2:
            raise ValueError("radius_match_float: float32 (n, dim) arrays are required")
        if q.shape[1] != t.shape[1]:
            raise ValueError(f"radius_match_float: query rows of dim {q.shape[1]}, train rows of dim {t.shape[1]}")
        return self._radius_host(self.L.mim_radius_l2, np.ascontiguousarray(q), np.ascontiguousarray(t), max_distance)

    def radius_match_float(self, query, train, max_distance):
        """BFMatcher(NORM_L2).radiusMatch(query, train, matches, maxDistance) on float rows of any dim -> lists of
        DMatch."""
        return self._radius_dmatches(*self.radius_match_float_arrays(query, train, max_distance))

    def radius_batch(self, problems, max_distance):
        """radiusMatch of every problem (query set, train set) of any mix of kinds: mim_radius_count, then the
        allocation, then mim_radius_fill_dev.  Returns (offsets int64, idx int32, dist float32) as device tensors,
        CSR over all queries of all problems in order.  The fill is asynchronous on the matcher's stream; torch's
        current stream is ordered after it, so the tensors can be used there at once."""
        import torch
        r = self._check_radius(max_distance)
        arr = problems if isinstance(problems, np.ndarray) else np.asarray(list(problems), np.int32)
        arr = np.ascontiguousarray(arr, np.int32).reshape(-1, 2)
        nq = 0
        for qs in arr[:, 0]:
            rows = self._set_rows.get(int(qs))
            if rows is None:
                raise ValueError(f"radius_batch: the row count of set {int(qs)} is not known here")
            nq += rows
        dev = torch.device("cuda", self.device)
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the zero fill, before the matcher's stream writes
        total = C.c_int64()
        self._check(self.L.mim_radius_count(self._ctx, arr.ctypes.data_as(C.POINTER(Problem)), len(arr), r,
                                            C.c_void_p(offsets.data_ptr()), C.byref(total)))
        idx = torch.empty(max(total.value, 1), dtype=torch.int32, device=dev)
        dist = torch.empty(max(total.value, 1), dtype=torch.float32, device=dev)
        self._check(self.L.mim_radius_fill_dev(self._ctx, C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()),
                                               total.value))
        torch.cuda.current_stream(dev).wait_stream(torch.cuda.ExternalStream(self.stream_handle(), device=dev))
        return offsets, idx[:total.value], dist[:total.value]

    def radius_sets(self, qset: int, tset: int, max_distance):
        """radius_batch of the one problem (qset, tset)."""
        return self.radius_batch([(int(qset), int(tset))], max_distance)

    def set_sampler_stream(self, on: bool):
        """Second-stream getSubset replay (mim_ctx_set_sampler_stream): on for a batch alone, off when
        several contexts already overlap their batches."""
        self._check(self.L.mim_ctx_set_sampler_stream(self._ctx, int(on)))

    def set_timing(self, on: bool):
        self._check(self.L.mim_set_timing(self._ctx, int(on)))

    def kernel_ms(self, name: str) -> float:
        return float(self.L.mim_last_kernel_ms(self._ctx, name.encode()))
