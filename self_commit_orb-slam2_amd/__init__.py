"""MI355X-native ORB-SLAM2 hot path: Python host side over the C ABI of liborbx.so.

The product is the C-ABI library (include/orbx.h, csrc/*.hip).  This module is the thin
ctypes mirror of the reference's class surfaces used by tests and bench.py:

    ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)   include/ORBextractor.h:92
        .__call__(image) -> (keypoints[n] structured, descriptors[n,32])    ORBextractor.h:110
        .GetLevels() / GetScaleFactors() / ...                               ORBextractor.h:118-158
        .mvImagePyramid(level)                                               ORBextractor.h:161

There is no CPU fallback: constructing an extractor without a HIP device raises.
"""
import ctypes
import importlib.util
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
_spec = importlib.util.spec_from_file_location("orbx_build", _PKG / "build.py")
build_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build_mod)

ORBX_OK = 0
ERR_NAMES = {-1: "ORBX_ERR_ARG", -2: "ORBX_ERR_HIP", -3: "ORBX_ERR_CAPACITY", -4: "ORBX_ERR_NODEVICE", -5: "ORBX_ERR_STATE"}

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28

SYNTH_LOW_TEXTURE = 1
SYNTH_STEREO_RIGHT = 2


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


class ExtractorConfig(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int), ("scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("ini_th_fast", ctypes.c_int), ("min_th_fast", ctypes.c_int),
                ("max_width", ctypes.c_int), ("max_height", ctypes.c_int), ("max_batch", ctypes.c_int),
                ("device", ctypes.c_int), ("gauss_taps", ctypes.c_uint16 * 7), ("reserved_", ctypes.c_uint16)]


_lib = None


def lib_path():
    return build_mod.LIB


def load_library():
    """dlopen liborbx.so (building it first when a compiler is present)."""
    global _lib
    if _lib is not None:
        return _lib
    path = build_mod.build_liborbx(verbose=False)
    L = ctypes.CDLL(str(path))
    L.orbx_last_error.restype = ctypes.c_char_p
    L.orbx_stage_name.restype = ctypes.c_char_p
    L.orbx_stage_name.argtypes = [ctypes.c_int]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_extractor_create.argtypes = [ctypes.POINTER(ExtractorConfig), ctypes.POINTER(vp)]
    L.orbx_extractor_destroy.argtypes = [vp]
    L.orbx_extractor_destroy.restype = None
    L.orbx_extractor_tables.argtypes = [vp] + [vp] * 6
    L.orbx_extractor_capacity.argtypes = [vp]
    L.orbx_extract.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, vp]
    L.orbx_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, vp]
    L.orbx_extract_batch_begin.argtypes = [vp, vp, ci, ci, ci, ci]
    L.orbx_extract_batch_end.argtypes = [vp, vp, vp, ci, vp]
    L.orbx_extract_view_pyramid.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp]
    L.orbx_extractor_expect_partner.argtypes = [vp, vp]
    L.orbx_combiner_stats.argtypes = [vp, vp, vp, vp]
    L.orbx_extract_batch_device.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_size_t]
    L.orbx_batch_results_device.argtypes = [vp, vp, vp, vp, vp]
    L.orbx_batch_download.argtypes = [vp, ci, vp, vp, ci, vp]
    L.orbx_upload_frames.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
    L.orbx_extractor_sync.argtypes = [vp]
    L.orbx_extractor_status.argtypes = [vp, vp]
    L.orbx_batch_status_device.argtypes = [vp, vp, vp]
    L.orbx_pyramid_level_size.argtypes = [vp, ci, ci, ci, vp, vp]
    L.orbx_download_pyramid.argtypes = [vp, ci, ci, ci, vp, ci]
    L.orbx_debug_download_scores.argtypes = [vp, ci, ci, vp, ci]
    L.orbx_extractor_set_debug_taps.argtypes = [vp, ci]
    L.orbx_debug_download_candidates.argtypes = [vp, ci, ci, vp, ci, vp]
    L.orbx_debug_download_level_keypoints.argtypes = [vp, ci, ci, vp, ci, vp]
    L.orbx_extractor_set_profiling.argtypes = [vp, ci]
    L.orbx_extractor_last_timing.argtypes = [vp, vp, vp, vp]
    _lib = L
    return L


_synth = None


def _synth_lib():
    global _synth
    if _synth is None:
        _synth = ctypes.CDLL(str(build_mod.build_synth(verbose=False)))
        _synth.orbx_synth_frame_ex.argtypes = [ctypes.c_uint64] + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    return _synth


def _check(rc):
    if rc != ORBX_OK:
        raise OrbxError(rc, load_library().orbx_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def synth_frame(seed, width, height, flags=0, view=0, dx=0, dy=0):
    """Deterministic synthetic grayscale frame (synth/orbx_synth.cc in liborbx_synth.so: a test / bench helper, not part of liborbx.so)."""
    im = np.empty((height, width), np.uint8)
    if _synth_lib().orbx_synth_frame_ex(ctypes.c_uint64(seed), view, dx, dy, width, height, width, flags, _ptr(im)) != ORBX_OK:
        raise ValueError("bad synthetic frame arguments")
    return im


def synth_sequence(first_seed, count, width, height, views_per_scene=16, step=(3, 1), low_texture_every=16):
    """`count` frames: scenes of `views_per_scene` consecutive views translating by `step` px/view
    (so consecutive frames share corners); every `low_texture_every`-th scene view is low texture."""
    out = []
    for i in range(count):
        scene, view = divmod(i, views_per_scene)
        flags = SYNTH_LOW_TEXTURE if (low_texture_every and i % low_texture_every == low_texture_every - 1) else 0
        out.append(synth_frame(first_seed + scene, width, height, flags, view, view * step[0], view * step[1]))
    return out


class _Handle:
    """What the wrappers of the C-ABI handles share: _L (the library), _h (the handle), close() / __del__ through the class's
    destroy symbol, and the out-parameter plumbing of the *_last_timing calls."""
    _destroy = None            # name of the class's *_destroy symbol
    _keeps_pointer = False     # close() leaves an empty c_void_p in _h (the classes that always did), not None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = ctypes.c_void_p() if self._keeps_pointer else None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _timing(self, symbol, *types):
        """symbol(handle, &out...) with one out-parameter per ctypes type -> the tuple of their values"""
        out = [t() for t in types]
        _check(getattr(self._L, symbol)(self._h, *[ctypes.byref(o) for o in out]))
        return tuple(o.value for o in out)


class HostPyramid(ctypes.Structure):
    """orbx_host_pyramid (include/orbx.h)."""
    _fields_ = [("level", ctypes.c_void_p * 12), ("width", ctypes.c_int * 12), ("height", ctypes.c_int * 12), ("stride", ctypes.c_int * 12), ("nlevels", ctypes.c_int)]


class ORBextractor(_Handle):
    """Mirror of ORB_SLAM2::ORBextractor (reference include/ORBextractor.h:92-161)."""
    _destroy = "orbx_extractor_destroy"
    _keeps_pointer = True

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, max_width=1280, max_height=1024,
                 max_batch=1, device=0, gauss_taps=None):
        self._L = load_library()
        cfg = ExtractorConfig(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, max_width, max_height, max_batch, device)
        if gauss_taps is not None:
            for i in range(7):
                cfg.gauss_taps[i] = int(gauss_taps[i])
        self._h = ctypes.c_void_p()
        _check(self._L.orbx_extractor_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        self.nlevels = nlevels
        self.scaleFactor = float(np.float32(scaleFactor))
        self.max_batch = max_batch
        self.capacity = self._L.orbx_extractor_capacity(self._h)
        self._last_size = None

    # --- getters (ORBextractor.h:118-158) ---
    def _tables(self):
        nl = self.nlevels
        t = [np.zeros(nl, np.float32) for _ in range(4)]
        q = np.zeros(nl, np.int32)
        n = ctypes.c_int()
        _check(self._L.orbx_extractor_tables(self._h, ctypes.byref(n), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]), _ptr(q)))
        return t, q

    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return self.scaleFactor

    def GetScaleFactors(self):
        return self._tables()[0][0]

    def GetInverseScaleFactors(self):
        return self._tables()[0][1]

    def GetScaleSigmaSquares(self):
        return self._tables()[0][2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[0][3]

    def features_per_level(self):
        return self._tables()[1]

    # --- operator() ---
    def __call__(self, image, mask=None):
        """(keypoints, descriptors) of one CV_8UC1 image; `mask` is ignored like in the reference."""
        if image is None or image.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2
        kps, desc, counts = self.extract_batch([image])
        n = int(counts[0])
        return kps[0, :n].copy(), desc[0, :n].copy()

    def extract_with_pyramid(self, image):
        """operator() + the host pyramid of the same call (orbx_extract_view_pyramid): (keypoints, descriptors, [level 0, level 1, ...]);
        the arrays are copies of the handle's pinned views."""
        image = np.ascontiguousarray(image)
        H, W = image.shape
        kp, dp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        pyr = HostPyramid()
        _check(self._L.orbx_extract_view_pyramid(self._h, _ptr(image), W, H, W, ctypes.byref(kp), ctypes.byref(dp), ctypes.byref(n), ctypes.byref(pyr)))
        self._last_size = (W, H)
        cnt = n.value
        kps = np.ctypeslib.as_array(ctypes.cast(kp, ctypes.POINTER(ctypes.c_uint8)), shape=(cnt * KEYPOINT_DTYPE.itemsize,)).view(KEYPOINT_DTYPE).copy() if cnt else np.zeros(0, KEYPOINT_DTYPE)
        desc = np.ctypeslib.as_array(ctypes.cast(dp, ctypes.POINTER(ctypes.c_uint8)), shape=(cnt, 32)).copy() if cnt else np.zeros((0, 32), np.uint8)
        levels = []
        for l in range(pyr.nlevels):
            w, h, st = pyr.width[l], pyr.height[l], pyr.stride[l]
            buf = np.ctypeslib.as_array(ctypes.cast(pyr.level[l], ctypes.POINTER(ctypes.c_uint8)), shape=((h - 1) * st + w,))
            levels.append(np.lib.stride_tricks.as_strided(buf, shape=(h, w), strides=(st, 1)).copy())
        return kps, desc, levels

    def expect_partner(self, other):
        """One-shot hint: `other`'s single-frame call is about to arrive on another thread (orbx_extractor_expect_partner)."""
        _check(self._L.orbx_extractor_expect_partner(self._h, other._h if other is not None else None))

    def combiner_stats(self):
        """(launch sets, frames, engines) served so far for this handle's configuration and image size."""
        b, f, e = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _check(self._L.orbx_combiner_stats(self._h, ctypes.byref(b), ctypes.byref(f), ctypes.byref(e)))
        return b.value, f.value, e.value

    def extract_batch(self, images, out=None):
        """out = (kps, desc, counts) of an earlier call: the result arrays are reused (a caller in a loop; allocating and zeroing 60 bytes x
        capacity x batch per call costs as much as the call)."""
        B = len(images)
        H, W = images[0].shape
        imgs = [np.ascontiguousarray(im) for im in images]
        arr = (ctypes.c_void_p * B)(*[im.ctypes.data for im in imgs])
        cap = self.capacity
        if out is not None and out[0].shape == (B, cap) and out[1].shape == (B, cap, 32) and out[2].shape == (B,):
            kps, desc, counts = out
        else:
            kps = np.zeros((B, cap), KEYPOINT_DTYPE)
            desc = np.zeros((B, cap, 32), np.uint8)
            counts = np.zeros(B, np.int32)
        _check(self._L.orbx_extract_batch(self._h, arr, B, W, H, W, _ptr(kps), _ptr(desc), cap, _ptr(counts)))
        self._last_size = (W, H)
        return kps, desc, counts

    # --- the two-deep pipeline of host batches (orbx_extract_batch_begin / _end) ---
    def extract_batch_begin(self, images):
        """Stage + upload + launch set + read-back of one batch, nothing waited for; at most two batches between a begin and its end."""
        B = len(images)
        H, W = images[0].shape
        arr = (ctypes.c_void_p * B)(*[im.ctypes.data for im in images])      # (the caller keeps `images` alive and contiguous until the call returns)
        _check(self._L.orbx_extract_batch_begin(self._h, arr, B, W, H, images[0].strides[0]))
        self._last_size = (W, H)
        self._pipe_batches = getattr(self, "_pipe_batches", []) + [B]

    def extract_batch_end(self, out=None):
        """Results of the OLDEST begun batch, as extract_batch returns them."""
        if not getattr(self, "_pipe_batches", None):
            raise OrbxError(-5, "no batch has been begun")
        B = self._pipe_batches.pop(0)
        cap = self.capacity
        if out is not None and out[0].shape == (B, cap) and out[1].shape == (B, cap, 32) and out[2].shape == (B,):
            kps, desc, counts = out
        else:
            kps = np.zeros((B, cap), KEYPOINT_DTYPE)
            desc = np.zeros((B, cap, 32), np.uint8)
            counts = np.zeros(B, np.int32)
        _check(self._L.orbx_extract_batch_end(self._h, _ptr(kps), _ptr(desc), cap, _ptr(counts)))
        return kps, desc, counts

    # --- device-resident path used by bench.py ---
    def upload(self, images):
        B = len(images)
        H, W = images[0].shape
        imgs = [np.ascontiguousarray(im) for im in images]
        arr = (ctypes.c_void_p * B)(*[im.ctypes.data for im in imgs])
        dev = ctypes.c_void_p()
        stride = ctypes.c_int()
        fp = ctypes.c_size_t()
        _check(self._L.orbx_upload_frames(self._h, arr, B, W, H, W, ctypes.byref(dev), ctypes.byref(stride), ctypes.byref(fp)))
        return dev, stride.value, fp.value, (B, W, H)

    def run_device(self, dev, stride, frame_pitch, shape):
        B, W, H = shape
        _check(self._L.orbx_extract_batch_device(self._h, dev, B, W, H, stride, frame_pitch))
        self._last_size = (W, H)

    def sync(self):
        _check(self._L.orbx_extractor_sync(self._h))

    def download(self, batch):
        cap = self.capacity
        kps = np.zeros((batch, cap), KEYPOINT_DTYPE)
        desc = np.zeros((batch, cap, 32), np.uint8)
        counts = np.zeros(batch, np.int32)
        _check(self._L.orbx_batch_download(self._h, batch, _ptr(kps), _ptr(desc), cap, _ptr(counts)))
        return kps, desc, counts

    def results_device(self):
        k, d, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        cap = ctypes.c_int()
        _check(self._L.orbx_batch_results_device(self._h, ctypes.byref(k), ctypes.byref(d), ctypes.byref(c), ctypes.byref(cap)))
        return k, d, c, cap.value

    def status(self):
        """Capacity bits of the last batch (0 = complete), without downloading it: orbx_extractor_status."""
        bits = ctypes.c_int32()
        _check(self._L.orbx_extractor_status(self._h, ctypes.byref(bits)))
        return bits.value

    def set_debug_taps(self, on):
        _check(self._L.orbx_extractor_set_debug_taps(self._h, 1 if on else 0))

    def set_profiling(self, on):
        _check(self._L.orbx_extractor_set_profiling(self._h, 1 if on else 0))

    def last_timing(self):
        tot = ctypes.c_float()
        st = (ctypes.c_float * 16)()
        n = ctypes.c_int()
        _check(self._L.orbx_extractor_last_timing(self._h, ctypes.byref(tot), st, ctypes.byref(n)))
        return tot.value, {self._L.orbx_stage_name(i).decode(): st[i] for i in range(n.value)}

    # --- mvImagePyramid and the stage taps ---
    def level_size(self, level, size=None):
        W, H = size or self._last_size
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._L.orbx_pyramid_level_size(self._h, W, H, level, ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def mvImagePyramid(self, level, frame=0, blurred=False):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _check(self._L.orbx_download_pyramid(self._h, frame, level, 1 if blurred else 0, _ptr(out), w))
        return out

    def debug_scores(self, level, frame=0):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _check(self._L.orbx_debug_download_scores(self._h, frame, level, _ptr(out), w))
        return out

    def debug_candidates(self, level, frame=0, cap=1 << 16):
        out = np.zeros(cap, np.uint32)
        n = ctypes.c_int()
        _check(self._L.orbx_debug_download_candidates(self._h, frame, level, _ptr(out), cap, ctypes.byref(n)))
        return out[:min(n.value, cap)].copy(), n.value

    def debug_level_keypoints(self, level, frame=0):
        out = np.zeros(4096, KEYPOINT_DTYPE)
        n = ctypes.c_int()
        _check(self._L.orbx_debug_download_level_keypoints(self._h, frame, level, _ptr(out), 4096, ctypes.byref(n)))
        return out[:n.value].copy()


# =====================================================================================
# ORBmatcher (Hamming paths) over the C ABI
# =====================================================================================
class FeatureSet(ctypes.Structure):
    _fields_ = [("keypoints", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("groups", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("capacity", ctypes.c_int), ("nframes", ctypes.c_int)]


class ProjectionFrame(ctypes.Structure):
    _fields_ = [("keypoints_un", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("u_right", ctypes.c_void_p), ("occupied", ctypes.c_void_p),
                ("counts", ctypes.c_void_p), ("capacity", ctypes.c_int), ("nframes", ctypes.c_int), ("min_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("grid_width_inv", ctypes.c_float), ("grid_height_inv", ctypes.c_float)]


class ProjectionPoints(ctypes.Structure):
    _fields_ = [("proj_x", ctypes.c_void_p), ("proj_y", ctypes.c_void_p), ("proj_xr", ctypes.c_void_p), ("scale_level", ctypes.c_void_p),
                ("view_cos", ctypes.c_void_p), ("in_view", ctypes.c_void_p), ("has_observations", ctypes.c_void_p), ("descriptors", ctypes.c_void_p),
                ("counts", ctypes.c_void_p), ("capacity", ctypes.c_int)]


class ProjectionLast(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_void_p), ("world_pos", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("has_observations", ctypes.c_void_p),
                ("octave", ctypes.c_void_p), ("angle", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("capacity", ctypes.c_int),
                ("tcw_current", ctypes.c_void_p), ("tcw_last", ctypes.c_void_p), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("mbf", ctypes.c_float), ("mb", ctypes.c_float), ("max_x", ctypes.c_float), ("max_y", ctypes.c_float)]


class BowParams(ctypes.Structure):
    _fields_ = [("nn_ratio", ctypes.c_float), ("check_orientation", ctypes.c_int), ("mode", ctypes.c_int)]


class TrackMotionResult(ctypes.Structure):      # orbx_track_motion_result
    _fields_ = [("matches", ctypes.c_void_p), ("search_matches", ctypes.c_void_p), ("discarded", ctypes.c_void_p), ("pose", ctypes.c_void_p)] + \
               [(k, ctypes.c_int32) for k in ("nmatches_search", "wide", "n_correspondences", "pose_inliers", "nmatches", "nmatches_map", "ran_pose")] + \
               [("stats", ctypes.c_double * 8)]


class ReferenceKeyFrame(ctypes.Structure):      # orbx_reference_keyframe
    _fields_ = [("features", ctypes.POINTER(FeatureSet)), ("world_pos", ctypes.c_void_p), ("has_observations", ctypes.c_void_p)]


class ReferenceFrame(ctypes.Structure):         # orbx_reference_frame
    _fields_ = [("features", ctypes.POINTER(FeatureSet)), ("keypoints_un", ctypes.c_void_p), ("u_right", ctypes.c_void_p), ("tcw", ctypes.c_void_p)] + \
               [(k, ctypes.c_float) for k in ("fx", "fy", "cx", "cy", "mbf")] + [("inv_level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


class TrackReferenceResult(ctypes.Structure):   # orbx_track_reference_result
    _fields_ = [("matches", ctypes.c_void_p), ("search_matches", ctypes.c_void_p), ("discarded", ctypes.c_void_p), ("pose", ctypes.c_void_p)] + \
               [(k, ctypes.c_int32) for k in ("nmatches_search", "n_correspondences", "pose_inliers", "nmatches", "nmatches_map", "ran_pose")] + \
               [("stats", ctypes.c_double * 8)]


class RelocMatchFrame(ctypes.Structure):        # orbx_reloc_match_frame
    _fields_ = [("features", ctypes.POINTER(FeatureSet)), ("keypoints_un", ctypes.c_void_p), ("level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


class RelocMatchKeyFrame(ctypes.Structure):     # orbx_reloc_match_keyframe
    _fields_ = [("features", ctypes.POINTER(FeatureSet)), ("world_pos", ctypes.c_void_p), ("is_bad", ctypes.c_int)]


class RelocMatchResult(ctypes.Structure):       # orbx_reloc_match_result
    _fields_ = [(k, ctypes.c_void_p) for k in ("matches", "key_index", "p2d", "sigma2", "p3dw", "n", "nmatches", "discarded")]


class TrackLocalResult(ctypes.Structure):       # orbx_track_local_result
    _fields_ = [(k, ctypes.c_void_p) for k in ("assigned", "in_view", "proj_x", "proj_y", "proj_xr", "scale_level", "view_cos", "pose", "outlier", "found", "cleared")] + \
               [(k, ctypes.c_int32) for k in ("nmatches", "n_correspondences", "pose_inliers", "inliers_map", "inliers_all")] + [("stats", ctypes.c_double * 8)]


def _bind_matcher(L):
    if getattr(L, "_matcher_bound", False):
        return
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_descriptor_distance.argtypes = [vp, vp]
    L.orbx_matcher_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_matcher_destroy.argtypes = [vp]
    L.orbx_matcher_destroy.restype = None
    L.orbx_search_by_bow_device.argtypes = [vp, ctypes.POINTER(FeatureSet), ctypes.POINTER(FeatureSet), vp, vp, ci, ctypes.POINTER(BowParams), vp]
    L.orbx_search_for_triangulation.argtypes = [vp, ctypes.POINTER(FeatureSet), ctypes.POINTER(FeatureSet), vp, vp, vp]
    L.orbx_stereo_match_device.argtypes = [vp, ctypes.POINTER(FeatureSet), ctypes.POINTER(FeatureSet), vp, vp, ci, vp, ci, ctypes.c_float, vp]
    L.orbx_matcher_results_device.argtypes = [vp, vp, vp, vp, vp]
    L.orbx_compute_stereo_matches_device.argtypes = [vp, vp, vp, vp, vp, ci, ctypes.c_float, ctypes.c_float]
    L.orbx_stereo_results_device.argtypes = [vp, vp, vp, vp]
    L.orbx_stereo_download.argtypes = [vp, ci, vp, vp, ci]
    L.orbx_stereo_frame.argtypes = [vp, vp, vp, ctypes.c_float, ctypes.c_float, vp, vp, ci]
    L.orbx_matcher_download.argtypes = [vp, ci, vp, vp, ci, vp]
    L.orbx_matcher_sync.argtypes = [vp]
    L.orbx_search_by_bow.argtypes = [vp, ctypes.POINTER(FeatureSet), ctypes.POINTER(FeatureSet), ctypes.POINTER(BowParams), vp, vp]
    L.orbx_stereo_match.argtypes = [vp, ctypes.POINTER(FeatureSet), ctypes.POINTER(FeatureSet), vp, ci, ctypes.c_float, vp, vp]
    L.orbx_matcher_last_timing.argtypes = [vp, vp]
    L.orbx_search_by_projection_last.argtypes = [vp, ctypes.POINTER(ProjectionFrame), ctypes.POINTER(ProjectionLast), vp, ci, ctypes.c_float, ci, ci, vp, vp]
    L.orbx_search_by_projection.argtypes = [vp, ctypes.POINTER(ProjectionFrame), ctypes.POINTER(ProjectionPoints), vp, ci, ctypes.c_float, ctypes.c_float, vp, vp]
    L.orbx_matcher_last_kernel_timing.argtypes = [vp, vp, vp]
    L._matcher_bound = True


def DescriptorDistance(a, b):
    """ORBmatcher::DescriptorDistance (reference include/ORBmatcher.h:65)."""
    L = load_library()
    _bind_matcher(L)
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    return L.orbx_descriptor_distance(_ptr(a), _ptr(b))


def _host_set(kps, desc, groups=None, valid=None):
    """One frame of host features -> (FeatureSet, keepalive)."""
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8)
    n = np.array([len(kps)], np.int32)
    keep = [kps, desc, n]
    g = v = None
    if groups is not None:
        g = np.ascontiguousarray(groups, np.int32)
        keep.append(g)
    if valid is not None:
        v = np.ascontiguousarray(valid, np.uint8)
        keep.append(v)
    fs = FeatureSet(kps.ctypes.data, desc.ctypes.data, n.ctypes.data, g.ctypes.data if g is not None else None,
                    v.ctypes.data if v is not None else None, max(len(kps), 1), 1)
    return fs, keep


class FusePoints(ctypes.Structure):
    _fields_ = [("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("ur", ctypes.c_void_p), ("level", ctypes.c_void_p), ("radius", ctypes.c_void_p),
                ("active", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("capacity", ctypes.c_int),
                ("kf_min_x", ctypes.c_float), ("kf_min_y", ctypes.c_float)]


class AreaQueries(ctypes.Structure):
    _fields_ = [("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("radius", ctypes.c_void_p), ("min_level", ctypes.c_void_p), ("max_level", ctypes.c_void_p),
                ("active", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("capacity", ctypes.c_int),
                ("window_min_x", ctypes.c_float), ("window_min_y", ctypes.c_float)]


class FrustumFrame(ctypes.Structure):
    _fields_ = [("tcw", ctypes.c_void_p), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("mbf", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float), ("max_y", ctypes.c_float), ("ratio_thresholds", ctypes.c_void_p),
                ("nlevels", ctypes.c_int), ("nframes", ctypes.c_int)]


class MapPoints(ctypes.Structure):
    _fields_ = [("world_pos", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("max_distance", ctypes.c_void_p), ("min_distance", ctypes.c_void_p),
                ("counts", ctypes.c_void_p), ("capacity", ctypes.c_int)]


class LocalPoints(ctypes.Structure):
    _fields_ = [("world_pos", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("max_distance", ctypes.c_void_p), ("min_distance", ctypes.c_void_p),
                ("descriptors", ctypes.c_void_p), ("has_observations", ctypes.c_void_p), ("count", ctypes.c_int)]


def predict_scale_thresholds(log_scale_factor, nlevels):
    """orbx_predict_scale_thresholds: the float ratios at which MapPoint::PredictScale changes level (host, libm log)."""
    L = load_library()
    out = np.zeros(max(nlevels - 1, 1), np.float32)
    L.orbx_predict_scale_thresholds.argtypes = [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    _check(L.orbx_predict_scale_thresholds(ctypes.c_float(log_scale_factor), nlevels, _ptr(out)))
    return out[:nlevels - 1]


class KeyFrameGeom(ctypes.Structure):
    """orbx_keyframe_geom: pose and calibration of one KeyFrame (host)."""
    _fields_ = [("tcw", ctypes.c_float * 12), ("center", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("invfx", ctypes.c_float), ("invfy", ctypes.c_float), ("mb", ctypes.c_float), ("mbf", ctypes.c_float), ("scale_factor", ctypes.c_float),
                ("scale_factors", ctypes.c_void_p), ("level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


class KeyFrameObs(ctypes.Structure):
    _fields_ = [("keys_un", ctypes.c_void_p), ("keys_raw", ctypes.c_void_p), ("u_right", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("count", ctypes.c_int)]


class TriangulatePairs(ctypes.Structure):
    _fields_ = [("npairs", ctypes.c_int), ("match_offset", ctypes.c_void_p), ("idx1", ctypes.c_void_p), ("idx2", ctypes.c_void_p), ("geom1", ctypes.c_void_p),
                ("geom2", ctypes.c_void_p), ("obs1", ctypes.c_void_p), ("obs2", ctypes.c_void_p)]


class NewPointsParams(ctypes.Structure):
    _fields_ = [("geom1", ctypes.c_void_p), ("geom2", ctypes.c_void_p), ("f12", ctypes.c_void_p), ("epipole", ctypes.c_void_p), ("keys_raw1", ctypes.c_void_p),
                ("u_right1", ctypes.c_void_p), ("depth1", ctypes.c_void_p), ("keys_raw2", ctypes.c_void_p), ("u_right2", ctypes.c_void_p), ("depth2", ctypes.c_void_p),
                ("check_orientation", ctypes.c_int), ("profile_kernels", ctypes.c_int)]


class NewPointsResult(ctypes.Structure):
    _fields_ = [("created", ctypes.c_void_p), ("created_capacity", ctypes.c_int), ("count", ctypes.c_void_p), ("nmatches", ctypes.c_void_p), ("pairs_done", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("matches", ctypes.c_void_p), ("x3d", ctypes.c_void_p)]


NEW_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("path", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
assert NEW_POINT_DTYPE.itemsize == 28


def _geom(g, keep):
    """dict(tcw (3,4), center, fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factor, scale_factors, level_sigma2) -> KeyFrameGeom"""
    sf, s2 = np.ascontiguousarray(g["scale_factors"], np.float32), np.ascontiguousarray(g["level_sigma2"], np.float32)
    keep += [sf, s2]
    out = KeyFrameGeom()
    out.tcw[:] = [float(x) for x in np.asarray(g["tcw"], np.float32).reshape(-1)[:12]]
    out.center[:] = [float(x) for x in np.asarray(g["center"], np.float32).reshape(3)]
    for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf", "scale_factor"):
        setattr(out, k, float(np.float32(g[k])))
    out.scale_factors, out.level_sigma2, out.nlevels = sf.ctypes.data, s2.ctypes.data, min(len(sf), len(s2))
    return out


def _obs(o, keep):
    """dict(kps (mvKeysUn), raw (n,2) or None, u_right, depth (None = monocular)) -> KeyFrameObs"""
    k = np.ascontiguousarray(o["kps"], KEYPOINT_DTYPE)
    arrs = [k]
    for name, shape in (("raw", (-1, 2)), ("u_right", (-1,)), ("depth", (-1,))):
        a = o.get(name)
        arrs.append(None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape)))
    keep += arrs
    return KeyFrameObs(*[a.ctypes.data if a is not None else None for a in arrs], len(k))


class TriangulationParams(ctypes.Structure):
    _fields_ = [("f12", ctypes.c_void_p), ("epipole", ctypes.c_void_p), ("stereo_a", ctypes.c_void_p), ("stereo_b", ctypes.c_void_p),
                ("scale_factors", ctypes.c_void_p), ("level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int), ("check_orientation", ctypes.c_int)]


class FuseKeyFrame(ctypes.Structure):
    _fields_ = [("slot", ctypes.c_int), ("num_features", ctypes.c_int), ("keys_un", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("u_right", ctypes.c_void_p),
                ("kf_point", ctypes.c_void_p), ("tcw", ctypes.c_float * 12), ("ow", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("mbf", ctypes.c_float), ("grid_min_x", ctypes.c_float), ("grid_min_y", ctypes.c_float), ("grid_width_inv", ctypes.c_float),
                ("grid_height_inv", ctypes.c_float), ("min_x", ctypes.c_int), ("max_x", ctypes.c_int), ("min_y", ctypes.c_int), ("max_y", ctypes.c_int),
                ("scale_factors", ctypes.c_void_p), ("inv_level_sigma2", ctypes.c_void_p), ("log_scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int)]


class FuseSlice(ctypes.Structure):
    _fields_ = [("num_keyframes", ctypes.c_int), ("kf_rank", ctypes.c_void_p), ("kf_bad", ctypes.c_void_p), ("num_searchable", ctypes.c_int), ("searchable", ctypes.c_void_p),
                ("num_points", ctypes.c_int), ("num_obs", ctypes.c_int), ("pos", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("min_distance", ctypes.c_void_p),
                ("max_distance", ctypes.c_void_p), ("raw_max_distance", ctypes.c_void_p), ("descriptors", ctypes.c_void_p), ("point_bad", ctypes.c_void_p),
                ("visible", ctypes.c_void_p), ("found", ctypes.c_void_p), ("obs_offset", ctypes.c_void_p), ("obs_kf", ctypes.c_void_p), ("obs_idx", ctypes.c_void_p),
                ("obs_stereo", ctypes.c_void_p), ("obs_descriptors", ctypes.c_void_p), ("th", ctypes.c_float), ("profile_kernels", ctypes.c_int)]


class FuseResult(ctypes.Structure):
    _fields_ = [("log", ctypes.c_void_p), ("log_capacity", ctypes.c_int), ("log_count", ctypes.c_void_p), ("nfused", ctypes.c_void_p), ("candidates", ctypes.c_void_p),
                ("candidates_capacity", ctypes.c_int), ("candidates_count", ctypes.c_void_p), ("kf_point", ctypes.c_void_p), ("point_bad", ctypes.c_void_p),
                ("replaced", ctypes.c_void_p), ("point_obs", ctypes.c_void_p), ("visible", ctypes.c_void_p), ("found", ctypes.c_void_p), ("descriptors", ctypes.c_void_p),
                ("obs_offset", ctypes.c_void_p), ("obs_kf", ctypes.c_void_p), ("obs_idx", ctypes.c_void_p), ("obs_stereo", ctypes.c_void_p), ("obs_capacity", ctypes.c_int),
                ("full_stride", ctypes.c_int), ("active", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("ur", ctypes.c_void_p), ("level", ctypes.c_void_p),
                ("radius", ctypes.c_void_p), ("best_idx", ctypes.c_void_p), ("best_dist", ctypes.c_void_p)]


FUSE_DECISION_DTYPE = np.dtype([("call", "<i4"), ("position", "<i4"), ("point", "<i4"), ("feature", "<i4"), ("kind", "<i4"), ("other", "<i4")])
FUSE_ADDED, FUSE_REPLACED_BY_HOLDER, FUSE_REPLACED_HOLDER, FUSE_HOLDER_BAD = 0, 1, 2, 3      # ORBX_FUSE_*

_FUSE_POINT_ARRAYS = (("pos", np.float32, 3), ("normal", np.float32, 3), ("min_dist", np.float32, 1), ("max_dist", np.float32, 1), ("raw_max_dist", np.float32, 1),
                      ("desc", np.uint8, 32), ("bad", np.uint8, 1), ("visible", np.int32, 1), ("found", np.int32, 1))
_FUSE_OBS_ARRAYS = (("obs_kf", np.int32, 1), ("obs_idx", np.int32, 1), ("obs_stereo", np.uint8, 1), ("obs_desc", np.uint8, 32))


def fuse_slice(searchable, points, other_obs=(), num_keyframes=None, ranks=None, kf_bad=None, th=3.0):
    """The arrays of orbx_fuse_slice.  searchable: one dict per searchable keyframe (slot, kps (mvKeysUn), desc, u_right, kf_point (mvpMapPoints as point ids
    or -1), Tcw (3x4 or 4x4), ow, cam = (fx, fy, cx, cy, mbf), bounds = (min_x, min_y, max_x, max_y) of the Frame, scale_factors, inv_level_sigma2,
    log_scale_factor); points: dict(pos, normal, min_dist, max_dist (the getters' values), raw_max_dist, desc, bad, visible, found).  The observations of the
    searchable keyframes follow from their kf_point; other_obs = (point, keyframe slot, feature, stereo, descriptor[32]) tuples of the keyframes that are not
    searchable.  Every point's observations are put in ascending rank.  ranks default to the slot numbers, kf_bad to 0."""
    NK = int(num_keyframes) if num_keyframes is not None else 1 + max([int(k["slot"]) for k in searchable] + [int(o[1]) for o in other_obs])
    rk = np.arange(NK, dtype=np.int32) if ranks is None else np.ascontiguousarray(ranks, np.int32)
    pts = {k: np.ascontiguousarray(points[k], dt).reshape((-1, w) if w > 1 else (-1,)) for k, dt, w in _FUSE_POINT_ARRAYS}
    P = len(pts["bad"])
    per = [[] for _ in range(P)]
    for k in searchable:
        ur, d = np.asarray(k["u_right"], np.float32), np.asarray(k["desc"], np.uint8)
        for f, p in enumerate(np.asarray(k["kf_point"], np.int32)):
            if p >= 0:
                per[int(p)].append((int(rk[int(k["slot"])]), int(k["slot"]), f, 1 if ur[f] >= 0 else 0, d[f]))
    for p, kf, f, st, d in other_obs:
        per[int(p)].append((int(rk[int(kf)]), int(kf), int(f), 1 if st else 0, np.asarray(d, np.uint8)))
    for o in per:
        o.sort(key=lambda t: t[0])
    flat = [t for o in per for t in o]
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in per])
    out = dict(pts, kf_rank=rk, kf_bad=np.zeros(NK, np.uint8) if kf_bad is None else np.ascontiguousarray(kf_bad, np.uint8), searchable=list(searchable), obs_offset=off,
               obs_kf=np.array([t[1] for t in flat], np.int32).reshape(-1), obs_idx=np.array([t[2] for t in flat], np.int32).reshape(-1),
               obs_stereo=np.array([t[3] for t in flat], np.uint8).reshape(-1), obs_desc=np.array([t[4] for t in flat], np.uint8).reshape(-1, 32), th=float(th))
    return out


def fuse_marshal(map_slice, keep, profile_kernels=False):
    """orbx_fuse_slice of a dict (fuse_slice's keys); what the struct points to is appended to `keep`, which must outlive the call"""
    a = {k: np.ascontiguousarray(map_slice[k], dt).reshape(-1) for k, dt in (("kf_rank", np.int32), ("kf_bad", np.uint8), ("obs_offset", np.int32))}
    for k, dt, _ in _FUSE_POINT_ARRAYS + _FUSE_OBS_ARRAYS:
        a[k] = np.ascontiguousarray(map_slice[k], dt).reshape(-1)
    NK, P, T0 = len(a["kf_rank"]), len(a["bad"]), len(a["obs_kf"])
    if len(a["kf_bad"]) != NK or len(a["obs_offset"]) != P + 1 or any(len(a[k]) != P * w for k, _, w in _FUSE_POINT_ARRAYS) or any(len(a[k]) != T0 * w for k, _, w in _FUSE_OBS_ARRAYS):
        raise ValueError("fuse slice: array sizes do not agree")
    S = len(map_slice["searchable"])
    tab = (FuseKeyFrame * max(S, 1))()
    for i, k in enumerate(map_slice["searchable"]):
        kp, d = np.ascontiguousarray(k["kps"], KEYPOINT_DTYPE), np.ascontiguousarray(k["desc"], np.uint8).reshape(-1)
        ur, kfp = np.ascontiguousarray(k["u_right"], np.float32).reshape(-1), np.ascontiguousarray(k["kf_point"], np.int32).reshape(-1)
        sf, s2 = np.ascontiguousarray(k["scale_factors"], np.float32).reshape(-1), np.ascontiguousarray(k["inv_level_sigma2"], np.float32).reshape(-1)
        n = len(kp)
        if len(d) != 32 * n or len(ur) != n or len(kfp) != n or len(s2) != len(sf):
            raise ValueError("fuse slice: searchable keyframe %d: array sizes do not agree" % i)
        keep.append((kp, d, ur, kfp, sf, s2))
        T = np.asarray(k["Tcw"], np.float32).reshape(-1, 4)[:3].reshape(12)
        minx, miny, maxx, maxy = (np.float32(b) for b in k["bounds"])
        fx, fy, cx, cy, mbf = (float(np.float32(c)) for c in k["cam"])
        tab[i] = FuseKeyFrame(int(k["slot"]), n, kp.ctypes.data, d.ctypes.data, ur.ctypes.data, kfp.ctypes.data, (ctypes.c_float * 12)(*T.tolist()),
                              (ctypes.c_float * 3)(*np.asarray(k["ow"], np.float32).reshape(3).tolist()), fx, fy, cx, cy, mbf, float(minx), float(miny),
                              float(np.float32(64) / (maxx - minx)), float(np.float32(48) / (maxy - miny)), int(minx), int(maxx), int(miny), int(maxy), sf.ctypes.data, s2.ctypes.data,
                              float(np.float32(k["log_scale_factor"])), len(sf))
    keep.append((a, tab))
    p = {k: v.ctypes.data for k, v in a.items()}
    return FuseSlice(NK, p["kf_rank"], p["kf_bad"], S, ctypes.addressof(tab), P, T0, p["pos"], p["normal"], p["min_dist"], p["max_dist"], p["raw_max_dist"], p["desc"], p["bad"],
                     p["visible"], p["found"], p["obs_offset"], p["obs_kf"], p["obs_idx"], p["obs_stereo"], p["obs_desc"], float(map_slice.get("th", 3.0)),
                     1 if profile_kernels else 0), a


def fuse_next_slice(map_slice, result):
    """The slice as a SearchInNeighbors / FuseApply call left it (its result dict): what the next call, orbx_mappoint_refresh or orbx_covis_update_connections
    starts from.  An observation keeps the descriptor of its feature."""
    sidx = {int(k["slot"]): i for i, k in enumerate(map_slice["searchable"])}
    old = {(int(kf), int(f)): d for kf, f, d in zip(np.asarray(map_slice["obs_kf"]).reshape(-1), np.asarray(map_slice["obs_idx"]).reshape(-1),
                                                     np.asarray(map_slice["obs_desc"], np.uint8).reshape(-1, 32))}
    desc = [np.asarray(map_slice["searchable"][sidx[int(kf)]]["desc"], np.uint8).reshape(-1, 32)[int(f)] if int(kf) in sidx else old[(int(kf), int(f))]
            for kf, f in zip(result["obs_kf"], result["obs_idx"])]
    out = dict(map_slice, bad=result["point_bad"].copy(), visible=result["visible"].copy(), found=result["found"].copy(), desc=result["desc"].copy(),
               obs_offset=result["obs_offset"].copy(), obs_kf=result["obs_kf"].copy(), obs_idx=result["obs_idx"].copy(), obs_stereo=result["obs_stereo"].copy(),
               obs_desc=np.array(desc, np.uint8).reshape(-1, 32))
    out["searchable"] = [dict(k, kf_point=result["kf_point"][i].copy()) for i, k in enumerate(map_slice["searchable"])]
    return out


class RelocFrame(ctypes.Structure):            # orbx_reloc_frame
    _fields_ = [("frame", ProjectionFrame)] + [(k, ctypes.c_float) for k in ("fx", "fy", "cx", "cy", "mbf", "max_x", "max_y")] + \
               [("scale_factors", ctypes.c_void_p), ("ratio_thresholds", ctypes.c_void_p), ("inv_level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int),
                ("check_orientation", ctypes.c_int)]


class RelocCandidate(ctypes.Structure):        # orbx_reloc_candidate
    _fields_ = [("npoints", ctypes.c_int)] + [(k, ctypes.c_void_p) for k in ("valid", "world_pos", "max_distance", "min_distance", "descriptors", "kf_angle", "bow_match")]


class RelocHypotheses(ctypes.Structure):       # orbx_reloc_hypotheses
    _fields_ = [("count", ctypes.c_int), ("candidate", ctypes.c_void_p), ("tcw", ctypes.c_void_p), ("inliers", ctypes.c_void_p), ("sequence", ctypes.c_void_p),
                ("sequence_length", ctypes.c_int), ("pnp", ctypes.c_void_p), ("record", ctypes.c_void_p), ("keypoint_index", ctypes.c_void_p),
                ("keypoint_count", ctypes.c_void_p)]


class RelocResult(ctypes.Structure):           # orbx_reloc_result
    _fields_ = [(k, ctypes.c_void_p) for k in ("stage", "success", "ngood", "nadditional", "n_correspondences", "pose", "stats", "map_point", "outlier")] + \
               [(k, ctypes.c_int32) for k in ("winner", "hypothesis", "candidate")]


RELOC_MAX_HYPOTHESES = 64      # ORBX_RELOC_MAX_HYPOTHESES
RELOC_MAX_SEQUENCE = 4096      # ORBX_RELOC_MAX_SEQUENCE


def reloc_sequence(pnp_results, max_its=None, n_iterations=5, max_hypotheses=RELOC_MAX_HYPOTHESES, max_sequence=RELOC_MAX_SEQUENCE):
    """The order in which Tracking::Relocalization's loop (reference src/Tracking.cc:2105-2226) receives poses from its PnP solvers: round-robin over the
    undiscarded candidates, iterate(5) on each (src/PnPsolver.cc:247-330, replayed from what the device solved: count / record_of / record_iteration /
    refined_count per candidate, with n, min_inliers and the solver's iteration limit), a candidate discarded when iterate reports bNoMore.
    pnp_results: per candidate an object or dict with n, min_inliers, count[its], record_of[its], refined_count[records] and mRansacMaxIts (or max_its here).
    Returns dict(hypotheses = the distinct (candidate, record, final) in order of first appearance - final = 0: the refined pose and mask of the record
    (:292-309), 1: the record's own pose and mask returned with bNoMore when the iterations run out (:318-327) -, sequence = indices into them, truncated =
    the hypothesis or sequence limit cut the order short, exhausted = a candidate ran past the iterations that were solved (the caller solves more and
    asks again).  Where the reference's loop would stop is not known here: the device's `winner` tells."""
    def get(r, k, d=None):
        return r.get(k, d) if isinstance(r, dict) else getattr(r, k, d)
    K = len(pnp_results)
    st = []
    for r in pnp_results:
        mx = get(r, "mRansacMaxIts", max_its)
        if mx is None:
            raise ValueError("no iteration limit: pass max_its")
        st.append(dict(n=int(get(r, "n")), min_inliers=int(get(r, "min_inliers")), count=np.asarray(get(r, "count")), record_of=np.asarray(get(r, "record_of")),
                       refined_count=np.asarray(get(r, "refined_count")), max_its=int(mx), it=0))
    discarded = [False] * K
    ncand = K
    hyps, index, seq = [], {}, []
    truncated = exhausted = False
    while ncand > 0 and not truncated and not exhausted:
        for i in range(K):
            if discarded[i]:
                continue
            c = st[i]
            ret, no_more = None, False
            if c["n"] < c["min_inliers"]:                                      # :251-255
                no_more = True
            else:
                cur = 0
                while c["it"] < c["max_its"] or cur < n_iterations:            # :266
                    if c["it"] >= len(c["count"]):
                        exhausted = True
                        break
                    cur += 1
                    it = c["it"]
                    c["it"] += 1
                    if c["count"][it] >= c["min_inliers"]:                     # :283-309
                        rec = int(c["record_of"][it])
                        if c["refined_count"][rec] > c["min_inliers"]:
                            ret = (i, rec, 0)
                            break
                if exhausted:
                    break
                if ret is None and c["it"] >= c["max_its"]:                    # :318-327
                    no_more = True
                    rec = int(c["record_of"][c["it"] - 1])
                    if rec >= 0:
                        ret = (i, rec, 1)
            if no_more:                                                        # src/Tracking.cc:2128-2132
                discarded[i] = True
                ncand -= 1
            if ret is not None:
                if ret not in index:
                    if len(hyps) >= max_hypotheses:
                        truncated = True
                        break
                    index[ret] = len(hyps)
                    hyps.append(ret)
                if len(seq) >= max_sequence:
                    truncated = True
                    break
                seq.append(index[ret])
    return dict(hypotheses=hyps, sequence=np.asarray(seq, np.int32), truncated=truncated, exhausted=exhausted)


def reloc_hypotheses(pnp_candidates, triples):
    """The hypotheses of ORBmatcher.RelocalizeRefine from solved PnPCandidate objects: for every (candidate, record, final) of reloc_sequence what
    PnPCandidate.iterate returns for it - the record's refined pose and mask (final = 0) or its own pose and mask (final = 1) - with the mask over the
    frame's features (through mvKeyPointIndices)."""
    out = []
    for c, rec, final in triples:
        r = pnp_candidates[c]
        vb = np.zeros(r.mN, np.uint8)
        if final:
            vb[r.indices[np.asarray(r.record_masks[rec], bool)]] = 1
            T = r.Tcw(int(r.record_iteration[rec]))
        else:
            vb[r.indices[np.asarray(r.refined_masks[rec], bool)]] = 1
            T = r._tcw(r.refined_tcw[rec])
        out.append(dict(candidate=int(c), Tcw=T, inliers=vb))
    return out


class LoopSim3KeyFrame(ctypes.Structure):      # orbx_loop_sim3_keyframe
    _fields_ = [("frame", ProjectionFrame), ("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3)] + \
               [(k, ctypes.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y")] + \
               [("scale_factors", ctypes.c_void_p), ("ratio_thresholds", ctypes.c_void_p), ("inv_level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("valid", "world_pos", "max_distance", "min_distance", "descriptors", "bow_match")]


class LoopSim3Hypotheses(ctypes.Structure):    # orbx_loop_sim3_hypotheses
    _fields_ = [("count", ctypes.c_int)] + [(k, ctypes.c_void_p) for k in ("candidate", "r12", "t12", "s12", "inliers", "solver", "iteration", "index1", "index1_count")]


_LOOP_REFINE_ARRAYS = ("status", "n_found", "n_pairs", "n_inliers", "n_bad", "quat", "t", "s", "scw", "matches12", "query_u", "query_v", "query_radius", "query_level",
                       "query_active", "match1", "match2")


class LoopRefineResult(ctypes.Structure):      # orbx_loop_refine_result
    _fields_ = [(k, ctypes.c_void_p) for k in _LOOP_REFINE_ARRAYS] + [(k, ctypes.c_int32) for k in ("winner", "hypothesis", "candidate")]


LOOP_SIM3_MAX_HYPOTHESES = 64      # ORBX_LOOP_SIM3_MAX_HYPOTHESES


def loop_sim3_sequence(candidates, nIterations=5):
    """The order in which LoopClosing::ComputeSim3's loop (reference src/LoopClosing.cc:403-482) receives Sim3 estimates from its solvers: round-robin over
    the undiscarded candidates, iterate(nIterations) on each (src/Sim3Solver.cc:199-285, replayed from what the device solved: count per iteration with n,
    min_inliers and the iterations that were run), a candidate discarded when iterate reports bNoMore (:428-432).  candidates: Sim3Candidate objects (their
    own iterate state is not touched) or dicts with n, min_inliers, count.  Returns the events in walk order as a list of dict(candidate, iteration); every
    event occurs once.  Where the reference's loop would stop is not known here: the device's `winner` tells."""
    def get(r, k):
        return r[k] if isinstance(r, dict) else getattr(r, k)
    st = [dict(n=int(get(r, "n")), min_inliers=int(get(r, "min_inliers")), count=np.asarray(get(r, "count")), it=0, best=0) for r in candidates]
    K = len(st)
    discarded, left, events = [False] * K, K, []
    while left > 0:
        for i in range(K):
            if discarded[i]:
                continue
            c = st[i]
            event, no_more = None, False
            if c["n"] < c["min_inliers"]:                                      # src/Sim3Solver.cc:206-210
                no_more = True
            else:
                cur = 0
                while c["it"] < len(c["count"]) and cur < nIterations:         # :219
                    it = c["it"]
                    cur += 1
                    c["it"] += 1
                    if c["count"][it] >= c["best"]:                            # :258-277
                        c["best"] = int(c["count"][it])
                        if c["count"][it] > c["min_inliers"]:
                            event = it
                            break
                if event is None and c["it"] >= len(c["count"]):               # :281-282
                    no_more = True
            if no_more:
                discarded[i] = True
                left -= 1
            if event is not None:
                events.append(dict(candidate=i, iteration=int(event)))
    return events


def loop_sim3_hypotheses(candidates, events):
    """Form (a) of ORBmatcher.LoopRefineSim3's hypotheses from solved Sim3Candidate objects: for every (candidate, iteration) of loop_sim3_sequence the
    iteration's R12 / t12 / s12 and its mask over KF1's features (through mvnIndices1), as Sim3Solver::iterate returns them."""
    out = []
    for e in events:
        r, it = candidates[e["candidate"]], int(e["iteration"])
        vb = np.zeros(r.mN1, np.uint8)
        vb[r.indices1[r.inliers(it)]] = 1
        out.append(dict(candidate=int(e["candidate"]), R12=r.r12[it].copy(), t12=r.t12[it].copy(), s12=np.float32(r.s12[it]), inliers=vb))
    return out


class ORBmatcher(_Handle):
    """Mirror of the Hamming paths of ORB_SLAM2::ORBmatcher (reference include/ORBmatcher.h:57-215)."""
    _destroy = "orbx_matcher_destroy"
    _keeps_pointer = True
    TH_LOW = 50
    TH_HIGH = 100
    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True, max_features=4096, max_pairs=1, device=0):
        self._L = load_library()
        _bind_matcher(self._L)
        self.nnratio, self.checkOri = float(nnratio), bool(checkOri)
        self.max_features, self.max_pairs = max_features, max_pairs
        self._h = ctypes.c_void_p()
        _check(self._L.orbx_matcher_create(device, max_features, max_pairs, ctypes.byref(self._h)))

    # ---- single pair, host arrays ----
    def SearchByBoW(self, kpsA, descA, kpsB, descB, groupsA=None, groupsB=None, validA=None, validB=None, mode=0):
        """mode 0: (KeyFrame, Frame) -> matches indexed by B;  mode 1: (KF1, KF2) -> indexed by A."""
        fa, ka = _host_set(kpsA, descA, groupsA, validA)
        fb, kb = _host_set(kpsB, descB, groupsB, validB)
        nout = len(kpsB) if mode == 0 else len(kpsA)
        out = np.full(max(nout, 1), -1, np.int32)
        nm = ctypes.c_int32()
        prm = BowParams(self.nnratio, 1 if self.checkOri else 0, mode)
        _check(self._L.orbx_search_by_bow(self._h, ctypes.byref(fa), ctypes.byref(fb), ctypes.byref(prm), _ptr(out), ctypes.byref(nm)))
        return nm.value, out[:nout]

    def SearchForTriangulation(self, kf1, kf2, F12, epipole, scale_factors, level_sigma2, only_stereo=False):
        """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (reference
        src/ORBmatcher.cc:810-1017).  kf*: dict(kps (structured mvKeysUn), desc, groups (mFeatVec node ids),
        has_mp (feature holds a MapPoint), u_right (mvuRight)); epipole = (ex, ey) of :817-826;
        scale_factors / level_sigma2 of pKF2.  Returns (nmatches, matches12[n1]) with matches12[i] = KF2 feature or -1."""
        sets, keep, flags = [], [], []
        for kf in (kf1, kf2):
            ur = np.asarray(kf["u_right"], np.float32)
            st = np.ascontiguousarray(ur >= 0, np.uint8)
            ok = np.asarray(kf["has_mp"], np.uint8) == 0
            if only_stereo:
                ok = ok & (st != 0)
            fs, k = _host_set(kf["kps"], kf["desc"], kf["groups"], ok.astype(np.uint8))
            sets.append(fs); keep.append(k); flags.append(st)
        f12 = np.ascontiguousarray(F12, np.float32).reshape(9)
        epi = np.ascontiguousarray(epipole, np.float32).reshape(2)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        prm = TriangulationParams(f12.ctypes.data, epi.ctypes.data, flags[0].ctypes.data, flags[1].ctypes.data, sf.ctypes.data, s2.ctypes.data,
                                   len(sf), 1 if self.checkOri else 0)
        n1 = len(kf1["kps"])
        out = np.full(max(n1, 1), -1, np.int32)
        nm = ctypes.c_int32()
        _check(self._L.orbx_search_for_triangulation(self._h, ctypes.byref(sets[0]), ctypes.byref(sets[1]), ctypes.byref(prm), _ptr(out), ctypes.byref(nm)))
        return nm.value, out[:n1]

    def TriangulateMatches(self, pairs):
        """The per-match geometry of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:423-596) on explicit match lists.
        pairs: list of dict(g1, g2 (keyframe geometry, see _geom), o1, o2 (observations, see _obs), idx1, idx2).  Returns dict(status (M) uint8,
        x3d (M,3) float32, offset (K+1)) over the concatenated matches."""
        L = self._L
        L.orbx_triangulate_matches.argtypes = [ctypes.c_void_p, ctypes.POINTER(TriangulatePairs), ctypes.c_void_p, ctypes.c_void_p]
        K = len(pairs)
        keep = []
        off = np.zeros(K + 1, np.int32)
        off[1:] = np.cumsum([len(p["idx1"]) for p in pairs])
        M = int(off[K])
        i1 = np.ascontiguousarray(np.concatenate([np.asarray(p["idx1"], np.int32) for p in pairs] + [np.zeros(0, np.int32)]), np.int32)
        i2 = np.ascontiguousarray(np.concatenate([np.asarray(p["idx2"], np.int32) for p in pairs] + [np.zeros(0, np.int32)]), np.int32)
        G1, G2 = (KeyFrameGeom * max(K, 1))(), (KeyFrameGeom * max(K, 1))()
        O1, O2 = (KeyFrameObs * max(K, 1))(), (KeyFrameObs * max(K, 1))()
        for k, p in enumerate(pairs):
            G1[k], G2[k], O1[k], O2[k] = _geom(p["g1"], keep), _geom(p["g2"], keep), _obs(p["o1"], keep), _obs(p["o2"], keep)
        tp = TriangulatePairs(K, off.ctypes.data, i1.ctypes.data, i2.ctypes.data, ctypes.addressof(G1), ctypes.addressof(G2), ctypes.addressof(O1), ctypes.addressof(O2))
        status, x3d = np.zeros(max(M, 1), np.uint8), np.zeros((max(M, 1), 3), np.float32)
        _check(L.orbx_triangulate_matches(self._h, ctypes.byref(tp), _ptr(status), _ptr(x3d)))
        return dict(status=status[:M], x3d=x3d[:M], offset=off)

    def CreateNewMapPoints(self, kf1, neighbours, stop_flag=None, capacity2=None, full=True, profile_kernels=False, created_capacity=None, capacity1=None):
        """The neighbour loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:350-624) as one call: per neighbour in order
        SearchForTriangulation on KF1's current eligibility mask, the geometry of its matches, the mask update; the created points in the
        reference's creation order.  kf1: dict(kps, desc, groups, has_mp, g (geometry)[, raw, u_right, depth]); neighbours: list of the same
        plus F12, epipole.  stop_flag: None or a uint8 array of one element (CheckNewKeyFrames()).  Returns dict(created (structured),
        count, nmatches (K), pairs_done[, status (K,n1), matches (K,n1), x3d (K,n1,3)])."""
        return self.new_points_prepare(kf1, neighbours, stop_flag, capacity2, full, profile_kernels, created_capacity, capacity1)()

    def new_points_prepare(self, kf1, neighbours, stop_flag=None, capacity2=None, full=True, profile_kernels=False, created_capacity=None, capacity1=None):
        """CreateNewMapPoints in two steps: the arrays marshalled once, and a function that makes the C call on them and returns the result dict;
        its attribute `raw` makes the C call alone and returns the status code (what tools/latency_new_points.py times).  capacity1 / capacity2:
        capacity of KF1's / the neighbours' feature set when it is to exceed the feature count (the per-slot arrays are laid out by it)."""
        L = self._L
        L.orbx_create_new_map_points.argtypes = [ctypes.c_void_p, ctypes.POINTER(FeatureSet), ctypes.POINTER(FeatureSet), ctypes.POINTER(NewPointsParams), ctypes.c_void_p,
                                                 ctypes.POINTER(NewPointsResult)]
        K = len(neighbours)
        keep = []
        n1 = len(kf1["kps"])
        fs1, k1 = _host_set(kf1["kps"], kf1["desc"], kf1.get("groups"), (np.asarray(kf1["has_mp"], np.uint8) == 0).astype(np.uint8))
        keep.append(k1)
        if capacity1:
            fs1.capacity = capacity1
        cap2 = capacity2 or max([len(nb["kps"]) for nb in neighbours] + [1])
        kp2, d2 = np.zeros((max(K, 1), cap2), KEYPOINT_DTYPE), np.zeros((max(K, 1), cap2, 32), np.uint8)
        cnt2, gr2, va2 = np.zeros(max(K, 1), np.int32), np.full((max(K, 1), cap2), -1, np.int32), np.zeros((max(K, 1), cap2), np.uint8)
        stereo2 = any(nb.get("u_right") is not None for nb in neighbours)
        raw2, ur2, dp2 = np.zeros((max(K, 1), cap2, 2), np.float32), np.full((max(K, 1), cap2), -1, np.float32), np.full((max(K, 1), cap2), -1, np.float32)
        G2 = (KeyFrameGeom * max(K, 1))()
        f12, epi = np.zeros((max(K, 1), 9), np.float32), np.zeros((max(K, 1), 2), np.float32)
        for k, nb in enumerate(neighbours):
            m = len(nb["kps"])
            cnt2[k] = m
            kp2[k, :m], d2[k, :m], va2[k, :m] = nb["kps"], nb["desc"], np.asarray(nb["has_mp"], np.uint8) == 0
            gr2[k, :m] = nb["groups"] if nb.get("groups") is not None else 0
            raw2[k, :m] = nb["raw"] if nb.get("raw") is not None else np.stack([nb["kps"]["x"], nb["kps"]["y"]], 1)
            if nb.get("u_right") is not None:
                ur2[k, :m], dp2[k, :m] = nb["u_right"], nb["depth"]
            G2[k] = _geom(nb["g"], keep)
            f12[k], epi[k] = np.asarray(nb["F12"], np.float32).reshape(9), np.asarray(nb["epipole"], np.float32).reshape(2)
        fs2 = FeatureSet(kp2.ctypes.data, d2.ctypes.data, cnt2.ctypes.data, gr2.ctypes.data, va2.ctypes.data, cap2, K)
        G1 = _geom(kf1["g"], keep)
        o1 = _obs(kf1, keep)
        prm = NewPointsParams(ctypes.addressof(G1), ctypes.addressof(G2), f12.ctypes.data, epi.ctypes.data, o1.keys_raw, o1.u_right, o1.depth,
                              raw2.ctypes.data, ur2.ctypes.data if stereo2 else None, dp2.ctypes.data if stereo2 else None, 1 if self.checkOri else 0, 1 if profile_kernels else 0)
        ccap = n1 if created_capacity is None else created_capacity
        created = np.zeros(max(ccap, 1), NEW_POINT_DTYPE)
        count, done, nm = ctypes.c_int32(), ctypes.c_int32(), np.zeros(max(K, 1), np.int32)
        c1 = capacity1 or max(n1, 1)
        status = np.zeros((max(K, 1), c1), np.uint8) if full else None
        matches = np.full((max(K, 1), c1), -1, np.int32) if full else None
        x3d = np.zeros((max(K, 1), c1, 3), np.float32) if full else None
        res = NewPointsResult(created.ctypes.data, ccap, ctypes.addressof(count), nm.ctypes.data, ctypes.addressof(done),
                              status.ctypes.data if full else None, matches.ctypes.data if full else None, x3d.ctypes.data if full else None)
        sf = None if stop_flag is None else np.ascontiguousarray(stop_flag, np.uint8)
        keep += [fs1, fs2, G1, G2, o1, f12, epi, kp2, d2, cnt2, gr2, va2, raw2, ur2, dp2, prm, res, sf]

        def raw():
            return L.orbx_create_new_map_points(self._h, ctypes.byref(fs1), ctypes.byref(fs2), ctypes.byref(prm), None if sf is None else sf.ctypes.data, ctypes.byref(res))

        def call():
            _check(raw())
            out = dict(created=created[:count.value].copy(), count=count.value, nmatches=nm[:K].copy(), pairs_done=done.value)
            if full:
                out.update(status=status[:K, :n1].copy(), matches=matches[:K, :n1].copy(), x3d=x3d[:K, :n1].copy())
            return out
        call.keep, call.raw = keep, raw
        return call

    def new_points_last_timing(self):
        """(device ms of the last chain, kernel launches, ms inside k_triangulate - 0 unless profile_kernels)"""
        self._L.orbx_new_points_last_timing.argtypes = [ctypes.c_void_p] * 4
        return self._timing("orbx_new_points_last_timing", ctypes.c_float, ctypes.c_int, ctypes.c_float)

    def _fuse_results(self, S, calls, lmax, full, log_capacity, candidates_capacity, obs_capacity):
        """the result arrays of a SearchInNeighbors / FuseApply call at their worst-case sizes (or the given capacities) -> (dict, FuseResult, counters)"""
        sk = [S.searchable_n[i] for i in range(S.num_searchable)]
        empty = S.empty_features
        P, i4, u1, f4 = S.num_points, np.int32, np.uint8, np.float32
        lc = int(S.log_worst if log_capacity is None else log_capacity)
        cc = int(S.cand_worst if candidates_capacity is None else candidates_capacity)
        oc = int(S.num_obs + empty if obs_capacity is None else obs_capacity)
        o = dict(log=np.zeros(max(lc, 1), FUSE_DECISION_DTYPE), nfused=np.zeros(max(calls, 1), i4), candidates=np.zeros(max(cc, 1), i4), kf_point=np.zeros(max(sum(sk), 1), i4),
                 point_bad=np.zeros(max(P, 1), u1), replaced=np.zeros(max(P, 1), i4), point_obs=np.zeros(max(P, 1), i4), visible=np.zeros(max(P, 1), i4), found=np.zeros(max(P, 1), i4),
                 desc=np.zeros((max(P, 1), 32), u1), obs_offset=np.zeros(P + 1, i4), obs_kf=np.zeros(max(oc, 1), i4), obs_idx=np.zeros(max(oc, 1), i4), obs_stereo=np.zeros(max(oc, 1), u1))
        nlog, ncand = ctypes.c_int32(), ctypes.c_int32()
        fl = {}
        if full:
            fl = dict(active=np.zeros((calls, lmax), u1), u=np.zeros((calls, lmax), f4), v=np.zeros((calls, lmax), f4), ur=np.zeros((calls, lmax), f4), level=np.zeros((calls, lmax), i4),
                      radius=np.zeros((calls, lmax), f4), best_idx=np.zeros((calls, lmax), i4), best_dist=np.zeros((calls, lmax), i4))
        R = FuseResult(o["log"].ctypes.data, lc, ctypes.addressof(nlog), o["nfused"].ctypes.data, o["candidates"].ctypes.data, cc, ctypes.addressof(ncand), o["kf_point"].ctypes.data,
                       o["point_bad"].ctypes.data, o["replaced"].ctypes.data, o["point_obs"].ctypes.data, o["visible"].ctypes.data, o["found"].ctypes.data, o["desc"].ctypes.data,
                       o["obs_offset"].ctypes.data, o["obs_kf"].ctypes.data, o["obs_idx"].ctypes.data, o["obs_stereo"].ctypes.data, oc, lmax,
                       *[fl[k].ctypes.data if full else None for k in ("active", "u", "v", "ur", "level", "radius", "best_idx", "best_dist")])
        o.update(fl)
        return o, R, (nlog, ncand, sk)

    @staticmethod
    def _fuse_finish(o, S, calls, cnt, full, list_lengths):
        nlog, ncand, sk = cnt
        P, nobs = S.num_points, int(o["obs_offset"][S.num_points])
        out = dict(log=o["log"][:nlog.value].copy(), nfused=o["nfused"][:calls].copy(), candidates=o["candidates"][:ncand.value].copy(),
                   kf_point=[o["kf_point"][sum(sk[:i]):sum(sk[:i + 1])].copy() for i in range(len(sk))], obs_offset=o["obs_offset"].copy(),
                   obs_kf=o["obs_kf"][:nobs].copy(), obs_idx=o["obs_idx"][:nobs].copy(), obs_stereo=o["obs_stereo"][:nobs].copy())
        for k in ("point_bad", "replaced", "point_obs", "visible", "found", "desc"):
            out[k] = o[k][:P].copy()
        if full:
            lens = list_lengths + [ncand.value]
            for k in ("active", "u", "v", "ur", "level", "radius", "best_idx", "best_dist"):
                out[k] = [o[k][c, :lens[c]].copy() for c in range(calls)]
        return out

    @staticmethod
    def _fuse_shape(S, a, map_slice, n_cur, targets):
        """sizes the wrappers allocate by: the features of the searchable keyframes, their empty features, the worst-case log and candidate list"""
        sn = [len(np.asarray(k["kf_point"]).reshape(-1)) for k in map_slice["searchable"]]
        by_slot = {int(k["slot"]): n for k, n in zip(map_slice["searchable"], sn)}
        S.searchable_n = sn
        S.empty_features = int(sum((np.asarray(k["kf_point"]).reshape(-1) < 0).sum() for k in map_slice["searchable"]))
        tl = [] if targets is None else [int(t) for t in targets]
        S.cand_worst = min(S.num_points, sum(by_slot.get(t, 0) for t in tl))
        S.log_worst = len(tl) * n_cur + S.cand_worst if targets is not None else n_cur

    def SearchInNeighbors(self, map_slice, current, targets, full=False, profile_kernels=False, log_capacity=None, candidates_capacity=None, obs_capacity=None):
        """Steps 2 and 3 of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:666-713) as one call: ORBmatcher::Fuse of every target keyframe on the
        current keyframe's points, in order, then of the current keyframe on the points the targets hold then.  map_slice: fuse_slice(); current, targets:
        keyframe slots.  Returns dict(log (FUSE_DECISION_DTYPE, execution order), nfused (T+1), candidates, kf_point (one array per searchable keyframe),
        point_bad, replaced, point_obs, visible, found, desc, obs_offset, obs_kf, obs_idx, obs_stereo[, per call: active, u, v, ur, level, radius, best_idx,
        best_dist]).  The capacities default to the worst case."""
        return self.search_in_neighbors_prepare(map_slice, current, targets, full, profile_kernels, log_capacity, candidates_capacity, obs_capacity)()

    def search_in_neighbors_prepare(self, map_slice, current, targets, full=False, profile_kernels=False, log_capacity=None, candidates_capacity=None, obs_capacity=None):
        """SearchInNeighbors in two steps: the arrays marshalled once, and a function that makes the C call on them and returns the result dict; its attribute `raw`
        makes the C call alone and returns the status code (what tools/latency_search_in_neighbors.py times)."""
        L = self._L
        L.orbx_search_in_neighbors.argtypes = [ctypes.c_void_p, ctypes.POINTER(FuseSlice), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(FuseResult)]
        keep = []
        S, a = fuse_marshal(map_slice, keep, profile_kernels)
        tg = np.ascontiguousarray(targets, np.int32).reshape(-1)
        T = len(tg)
        n_cur = max([len(np.asarray(k["kf_point"]).reshape(-1)) for k in map_slice["searchable"] if int(k["slot"]) == int(current)] + [0])
        self._fuse_shape(S, a, map_slice, n_cur, tg)
        lmax = max(n_cur, S.cand_worst, 1)
        o, R, cnt = self._fuse_results(S, T + 1, lmax, full, log_capacity, candidates_capacity, obs_capacity)
        keep += [tg, o, R, cnt]

        def raw():
            return L.orbx_search_in_neighbors(self._h, ctypes.byref(S), int(current), tg.ctypes.data, T, ctypes.byref(R))

        def call():
            _check(raw())
            return self._fuse_finish(o, S, T + 1, cnt, full, [n_cur] * T)
        call.keep, call.raw = keep, raw
        return call

    def FuseApply(self, map_slice, kf, points, active, best_idx, best_dist, log_capacity=None, obs_capacity=None):
        """The apply stage of one ORBmatcher::Fuse call (reference src/ORBmatcher.cc:1150-1171) for keyframe slot kf on search results the caller supplies:
        points (the list, -1 = NULL), active, best_idx, best_dist per entry.  Returns SearchInNeighbors' dict with one call."""
        L = self._L
        L.orbx_fuse_apply.argtypes = [ctypes.c_void_p, ctypes.POINTER(FuseSlice), ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.POINTER(FuseResult)]
        keep = []
        S, a = fuse_marshal(map_slice, keep)
        lst, act = np.ascontiguousarray(points, np.int32).reshape(-1), np.ascontiguousarray(active, np.uint8).reshape(-1)
        bi, bd = np.ascontiguousarray(best_idx, np.int32).reshape(-1), np.ascontiguousarray(best_dist, np.int32).reshape(-1)
        n = len(lst)
        if len(act) != n or len(bi) != n or len(bd) != n:
            raise ValueError("FuseApply: the list arrays differ in length")
        self._fuse_shape(S, a, map_slice, n, None)
        S.cand_worst, S.log_worst = 0, n
        o, R, cnt = self._fuse_results(S, 1, max(n, 1), False, log_capacity, 0, obs_capacity)
        _check(L.orbx_fuse_apply(self._h, ctypes.byref(S), int(kf), lst.ctypes.data, act.ctypes.data, bi.ctypes.data, bd.ctypes.data, n, ctypes.byref(R)))
        return self._fuse_finish(o, S, 1, cnt, False, [n])

    def search_in_neighbors_last_timing(self):
        """(device ms of the last chain, kernel launches, ms inside the apply kernels - 0 unless profile_kernels)"""
        self._L.orbx_search_in_neighbors_last_timing.argtypes = [ctypes.c_void_p] * 4
        return self._timing("orbx_search_in_neighbors_last_timing", ctypes.c_float, ctypes.c_int, ctypes.c_float)

    def FuseSearch(self, kf, points, chi2_gate=True):
        """Steps 2-3 of ORBmatcher::Fuse (reference src/ORBmatcher.cc:1093-1146 / 1258-1276): per map point the KeyFrame
        feature of minimum Hamming distance inside GetFeaturesInArea(u, v, radius) that passes the level gate and
        (first overload, chi2_gate) the reprojection gate.  kf: dict(kps (mvKeysUn), desc, u_right, inv_level_sigma2,
        width, height[, min_x, min_y, max_x, max_y]); points: dict(u, v, ur, level, radius, active, desc).
        Returns (best_idx[m], best_dist[m]); the caller fuses where best_dist <= TH_LOW."""
        k = np.ascontiguousarray(kf["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d = np.ascontiguousarray(kf["desc"], np.uint8)
        ur = np.ascontiguousarray(kf["u_right"], np.float32)
        s2 = np.ascontiguousarray(kf["inv_level_sigma2"], np.float32)
        minx, miny = np.float32(kf.get("min_x", 0.0)), np.float32(kf.get("min_y", 0.0))
        maxx, maxy = np.float32(kf.get("max_x", kf["width"])), np.float32(kf.get("max_y", kf["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pu, pv, pur, prad = f32(points["u"]), f32(points["v"]), f32(points["ur"]), f32(points["radius"])
        m = len(pu)
        lvl = np.ascontiguousarray(points["level"], np.int32)
        act = np.ascontiguousarray(points["active"], np.uint8)
        pd = np.ascontiguousarray(points["desc"], np.uint8)
        cn, cm = np.array([n], np.int32), np.array([m], np.int32)
        fr = ProjectionFrame(k.ctypes.data, d.ctypes.data, ur.ctypes.data, None, cn.ctypes.data, max(n, 1), 1, minx, miny, gw, gh)
        pt = FusePoints(pu.ctypes.data, pv.ctypes.data, pur.ctypes.data, lvl.ctypes.data, prad.ctypes.data, act.ctypes.data, pd.ctypes.data, cm.ctypes.data,
                        max(m, 1), float(np.float32(int(minx))), float(np.float32(int(miny))))
        bi, bd = np.full(max(m, 1), -1, np.int32), np.full(max(m, 1), 256, np.int32)
        self._L.orbx_fuse_search.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _check(self._L.orbx_fuse_search(self._h, ctypes.byref(fr), ctypes.byref(pt), _ptr(s2), len(s2), 1 if chi2_gate else 0, _ptr(bi), _ptr(bd)))
        return bi[:m], bd[:m]

    def AreaSearchGreedy(self, frame, queries, max_dist):
        """The search loops of ORBmatcher::SearchByProjection(pKF, Scw, ...) (loop closing, reference src/ORBmatcher.cc:453-510)
        and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (relocalisation, :1790-1826).
        frame: dict(kps (mvKeysUn), desc, blocked, width, height[, min_x, ...]); queries: dict(u, v, radius, min_level,
        max_level, active, desc[, window_int_bounds]).  Returns (nmatches, assigned[m], dists[m])."""
        k = np.ascontiguousarray(frame["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d = np.ascontiguousarray(frame["desc"], np.uint8)
        blk = np.ascontiguousarray(frame["blocked"], np.uint8)
        minx, miny = np.float32(frame.get("min_x", 0.0)), np.float32(frame.get("min_y", 0.0))
        maxx, maxy = np.float32(frame.get("max_x", frame["width"])), np.float32(frame.get("max_y", frame["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        qu, qv, qr = f32(queries["u"]), f32(queries["v"]), f32(queries["radius"])
        m = len(qu)
        lo, hi = np.ascontiguousarray(queries["min_level"], np.int32), np.ascontiguousarray(queries["max_level"], np.int32)
        act = np.ascontiguousarray(queries["active"], np.uint8)
        qd = np.ascontiguousarray(queries["desc"], np.uint8)
        cn, cm = np.array([n], np.int32), np.array([m], np.int32)
        wx, wy = (np.float32(int(minx)), np.float32(int(miny))) if queries.get("window_int_bounds") else (minx, miny)
        fr = ProjectionFrame(k.ctypes.data, d.ctypes.data, None, blk.ctypes.data, cn.ctypes.data, max(n, 1), 1, minx, miny, gw, gh)
        q = AreaQueries(qu.ctypes.data, qv.ctypes.data, qr.ctypes.data, lo.ctypes.data, hi.ctypes.data, act.ctypes.data, qd.ctypes.data, cm.ctypes.data,
                        max(m, 1), float(wx), float(wy))
        asg, dst = np.full(max(m, 1), -1, np.int32), np.full(max(m, 1), 256, np.int32)
        nm = ctypes.c_int32()
        self._L.orbx_area_search_greedy.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
        _check(self._L.orbx_area_search_greedy(self._h, ctypes.byref(fr), ctypes.byref(q), int(max_dist), _ptr(asg), _ptr(dst), ctypes.byref(nm)))
        return nm.value, asg[:m], dst[:m]

    def SearchForInitialization(self, f1, f2, prev_matched, window_size=10):
        """ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (reference src/ORBmatcher.cc:515-654).
        f1 / f2: dict(kps (mvKeysUn), desc); f2 also width, height[, min_x, ...]; prev_matched: (n1, 2) float array (updated copy returned).
        Returns (nmatches, vnMatches12, vbPrevMatched)."""
        fs1, keep1 = _host_set(f1["kps"], f1["desc"])
        k2 = np.ascontiguousarray(f2["kps"], KEYPOINT_DTYPE)
        d2 = np.ascontiguousarray(f2["desc"], np.uint8)
        n1, n2 = len(f1["kps"]), len(k2)
        minx, miny = np.float32(f2.get("min_x", 0.0)), np.float32(f2.get("min_y", 0.0))
        maxx, maxy = np.float32(f2.get("max_x", f2["width"])), np.float32(f2.get("max_y", f2["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        cn = np.array([n2], np.int32)
        fr = ProjectionFrame(k2.ctypes.data, d2.ctypes.data, None, None, cn.ctypes.data, max(n2, 1), 1, minx, miny, gw, gh)
        prev = np.ascontiguousarray(prev_matched, np.float32).reshape(-1, 2).copy()
        out = np.full(max(n1, 1), -1, np.int32)
        nm = ctypes.c_int32()
        self._L.orbx_search_for_initialization.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _check(self._L.orbx_search_for_initialization(self._h, ctypes.byref(fs1), ctypes.byref(fr), _ptr(prev), int(window_size), self.nnratio,
                                                      1 if self.checkOri else 0, _ptr(out), ctypes.byref(nm)))
        out = out[:n1]
        ok = out >= 0
        prev[ok, 0], prev[ok, 1] = k2["x"][out[ok]], k2["y"][out[ok]]          # :646-650
        return nm.value, out, prev

    def isInFrustum(self, Tcw, cam, bounds, log_scale_factor, nlevels, points, viewing_cos_limit):
        """Frame::isInFrustum (reference src/Frame.cc:608-742) for a list of map points.  cam = (fx, fy, cx, cy, mbf), bounds = (mnMinX, mnMaxX,
        mnMinY, mnMaxY), points: dict(pos (n,3), normal (n,3), max_distance, min_distance).  Returns dict(in_view, proj_x, proj_y, proj_xr, level, view_cos)."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        th = predict_scale_thresholds(log_scale_factor, nlevels)
        pos, nrm = np.ascontiguousarray(points["pos"], np.float32), np.ascontiguousarray(points["normal"], np.float32)
        mx, mn = np.ascontiguousarray(points["max_distance"], np.float32), np.ascontiguousarray(points["min_distance"], np.float32)
        n = len(mx)
        cnt = np.array([n], np.int32)
        fr = FrustumFrame(T.ctypes.data, cam[0], cam[1], cam[2], cam[3], cam[4], bounds[0], bounds[1], bounds[2], bounds[3], th.ctypes.data, nlevels, 1)
        mp = MapPoints(pos.ctypes.data, nrm.ctypes.data, mx.ctypes.data, mn.ctypes.data, cnt.ctypes.data, max(n, 1))
        f = lambda: np.zeros(max(n, 1), np.float32)
        px, py, pxr, vc, lvl, iv = f(), f(), f(), f(), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        self._L.orbx_is_in_frustum.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_float] + [ctypes.c_void_p] * 6
        _check(self._L.orbx_is_in_frustum(self._h, ctypes.byref(fr), ctypes.byref(mp), ctypes.c_float(viewing_cos_limit), _ptr(px), _ptr(py), _ptr(pxr), _ptr(lvl),
                                          _ptr(vc), _ptr(iv)))
        return dict(in_view=iv[:n], proj_x=px[:n], proj_y=py[:n], proj_xr=pxr[:n], level=lvl[:n], view_cos=vc[:n])

    def SearchByProjection(self, frame, points, th, nnratio=None):
        """ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (reference src/ORBmatcher.cc:70-175).
        frame: dict(kps (structured mvKeysUn), desc, u_right, occupied, scale_factors, width, height[, min_x, min_y]);
        points: dict(proj_x, proj_y, proj_xr, level, view_cos, in_view, has_obs, desc).
        Returns (nmatches, assigned[n]) with assigned[i] = index of the point put into mvpMapPoints[i] or -1."""
        k = np.ascontiguousarray(frame["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d = np.ascontiguousarray(frame["desc"], np.uint8)
        ur = np.ascontiguousarray(frame["u_right"], np.float32)
        occ = np.ascontiguousarray(frame["occupied"], np.uint8)
        sf = np.ascontiguousarray(frame["scale_factors"], np.float32)
        minx, miny = np.float32(frame.get("min_x", 0.0)), np.float32(frame.get("min_y", 0.0))
        maxx, maxy = np.float32(frame.get("max_x", frame["width"])), np.float32(frame.get("max_y", frame["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)      # src/Frame.cc:181-182
        cn, cm = np.array([n], np.int32), np.array([len(points["proj_x"])], np.int32)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        px, py, pxr, vc = f32(points["proj_x"]), f32(points["proj_y"]), f32(points["proj_xr"]), f32(points["view_cos"])
        lvl = np.ascontiguousarray(points["level"], np.int32)
        inv, obs = np.ascontiguousarray(points["in_view"], np.uint8), np.ascontiguousarray(points["has_obs"], np.uint8)
        md = np.ascontiguousarray(points["desc"], np.uint8)
        F = ProjectionFrame(_ptr(k).value, _ptr(d).value, _ptr(ur).value, _ptr(occ).value, _ptr(cn).value, n, 1, float(minx), float(miny), float(gw), float(gh))
        P = ProjectionPoints(_ptr(px).value, _ptr(py).value, _ptr(pxr).value, _ptr(lvl).value, _ptr(vc).value, _ptr(inv).value, _ptr(obs).value,
                             _ptr(md).value, _ptr(cm).value, int(cm[0]))
        out = np.full(max(n, 1), -1, np.int32)
        nm = ctypes.c_int32()
        _check(self._L.orbx_search_by_projection(self._h, ctypes.byref(F), ctypes.byref(P), _ptr(sf), len(sf), ctypes.c_float(th),
                                                 ctypes.c_float(self.nnratio if nnratio is None else nnratio), _ptr(out), ctypes.byref(nm)))
        return nm.value, out[:n]

    def SearchLocalPoints(self, frame, Tcw, cam, log_scale_factor, points, th, nnratio=None, viewing_cos_limit=0.5):
        """Tracking::SearchLocalPoints (reference src/Tracking.cc:1760-1830) as one device chain (orbx_search_local_points): Frame::isInFrustum over
        `points` (dict pos, normal, max_distance, min_distance, desc, has_obs) and SearchByProjection(F, points, th) on the frame (dict as in
        SearchByProjection); cam = (fx, fy, cx, cy, mbf).  Returns (nmatches, assigned[n], dict(in_view, proj_x, proj_y, proj_xr, level, view_cos))."""
        k = np.ascontiguousarray(frame["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d = np.ascontiguousarray(frame["desc"], np.uint8)
        ur = np.ascontiguousarray(frame["u_right"], np.float32)
        occ = np.ascontiguousarray(frame["occupied"], np.uint8)
        sf = np.ascontiguousarray(frame["scale_factors"], np.float32)
        minx, miny = np.float32(frame.get("min_x", 0.0)), np.float32(frame.get("min_y", 0.0))
        maxx, maxy = np.float32(frame.get("max_x", frame["width"])), np.float32(frame.get("max_y", frame["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        cn = np.array([n], np.int32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        thr = predict_scale_thresholds(log_scale_factor, len(sf))
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mx, mn = f32(points["pos"]), f32(points["normal"]), f32(points["max_distance"]), f32(points["min_distance"])
        md, obs = np.ascontiguousarray(points["desc"], np.uint8), np.ascontiguousarray(points["has_obs"], np.uint8)
        m = len(mx)
        F = ProjectionFrame(_ptr(k).value, _ptr(d).value, _ptr(ur).value, _ptr(occ).value, _ptr(cn).value, max(n, 1), 1, float(minx), float(miny), float(gw), float(gh))
        fr = FrustumFrame(T.ctypes.data, cam[0], cam[1], cam[2], cam[3], cam[4], float(minx), float(maxx), float(miny), float(maxy), thr.ctypes.data, len(sf), 1)
        P = LocalPoints(pos.ctypes.data, nrm.ctypes.data, mx.ctypes.data, mn.ctypes.data, md.ctypes.data, obs.ctypes.data, m)
        out, nm = np.full(max(n, 1), -1, np.int32), ctypes.c_int32()
        z = lambda dt: np.zeros(max(m, 1), dt)
        iv, px, py, pxr, lvl, vc = z(np.uint8), z(np.float32), z(np.float32), z(np.float32), z(np.int32), z(np.float32)
        self._L.orbx_search_local_points.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 8
        _check(self._L.orbx_search_local_points(self._h, ctypes.byref(F), ctypes.byref(fr), ctypes.byref(P), _ptr(sf), len(sf), ctypes.c_float(viewing_cos_limit),
                                                ctypes.c_float(th), ctypes.c_float(self.nnratio if nnratio is None else nnratio), _ptr(out), ctypes.byref(nm),
                                                _ptr(iv), _ptr(px), _ptr(py), _ptr(pxr), _ptr(lvl), _ptr(vc)))
        return nm.value, out[:n], dict(in_view=iv[:m], proj_x=px[:m], proj_y=py[:m], proj_xr=pxr[:m], level=lvl[:m], view_cos=vc[:m])

    def SearchByProjectionLast(self, frame, last, th, mono):
        """ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (reference
        src/ORBmatcher.cc:1569-1728).  frame: as SearchByProjection plus Tcw (4x4) and cam (fx, fy, cx, cy, bf);
        last: dict(Tcw, valid, pos, desc, has_obs, kps (structured; octave of mvKeys, angle of mvKeysUn)).
        Returns (nmatches, assigned[n]): assigned[i2] = last-frame feature whose MapPoint is in mvpMapPoints[i2], or -1."""
        k = np.ascontiguousarray(frame["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d = np.ascontiguousarray(frame["desc"], np.uint8)
        ur = np.ascontiguousarray(frame["u_right"], np.float32)
        occ = np.ascontiguousarray(frame["occupied"], np.uint8)
        sf = np.ascontiguousarray(frame["scale_factors"], np.float32)
        minx, miny = np.float32(frame.get("min_x", 0.0)), np.float32(frame.get("min_y", 0.0))
        maxx, maxy = np.float32(frame.get("max_x", frame["width"])), np.float32(frame.get("max_y", frame["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        lk = np.ascontiguousarray(last["kps"], KEYPOINT_DTYPE)
        nl = len(lk)
        cn, cl = np.array([n], np.int32), np.array([nl], np.int32)
        valid = np.ascontiguousarray(last["valid"], np.uint8)
        pos = np.ascontiguousarray(last["pos"], np.float32)
        ld = np.ascontiguousarray(last["desc"], np.uint8)
        obs = np.ascontiguousarray(last["has_obs"], np.uint8)
        octv = np.ascontiguousarray(lk["octave"], np.int32)
        ang = np.ascontiguousarray(lk["angle"], np.float32)
        tc, tl = np.ascontiguousarray(frame["Tcw"], np.float32), np.ascontiguousarray(last["Tcw"], np.float32)
        fx, fy, cx, cy, bf = [np.float32(v) for v in frame["cam"]]
        F = ProjectionFrame(_ptr(k).value, _ptr(d).value, _ptr(ur).value, _ptr(occ).value, _ptr(cn).value, n, 1, float(minx), float(miny), float(gw), float(gh))
        Ls = ProjectionLast(_ptr(valid).value, _ptr(pos).value, _ptr(ld).value, _ptr(obs).value, _ptr(octv).value, _ptr(ang).value, _ptr(cl).value, nl,
                            _ptr(tc).value, _ptr(tl).value, float(fx), float(fy), float(cx), float(cy), float(bf), float(bf / fx), float(maxx), float(maxy))
        out = np.full(max(n, 1), -1, np.int32)
        nm = ctypes.c_int32()
        _check(self._L.orbx_search_by_projection_last(self._h, ctypes.byref(F), ctypes.byref(Ls), _ptr(sf), len(sf), ctypes.c_float(th), 1 if mono else 0,
                                                      1 if self.checkOri else 0, _ptr(out), ctypes.byref(nm)))
        return nm.value, out[:n]

    def _frame_arrays(self, frame):
        """The frame side of the projection searches as (ProjectionFrame, keep-alive list, n, scale factors, (minx, maxx, miny, maxy))."""
        k = np.ascontiguousarray(frame["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d = np.ascontiguousarray(frame["desc"], np.uint8)
        ur = np.ascontiguousarray(frame["u_right"], np.float32)
        occ = None if frame.get("occupied") is None else np.ascontiguousarray(frame["occupied"], np.uint8)
        sf = np.ascontiguousarray(frame["scale_factors"], np.float32)
        minx, miny = np.float32(frame.get("min_x", 0.0)), np.float32(frame.get("min_y", 0.0))
        maxx, maxy = np.float32(frame.get("max_x", frame["width"])), np.float32(frame.get("max_y", frame["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        cn = np.array([n], np.int32)
        F = ProjectionFrame(_ptr(k).value, _ptr(d).value, _ptr(ur).value, None if occ is None else _ptr(occ).value, _ptr(cn).value, max(n, 1), 1, float(minx), float(miny),
                            float(gw), float(gh))
        return F, [k, d, ur, occ, cn], n, sf, (float(minx), float(maxx), float(miny), float(maxy))

    def TrackWithMotionModel(self, frame, last, th, mono, inv_level_sigma2):
        return self.track_motion_prepare(frame, last, th, mono, inv_level_sigma2)()

    def track_motion_prepare(self, frame, last, th, mono, inv_level_sigma2):
        """Tracking::TrackWithMotionModel (reference src/Tracking.cc:1370-1421) as one device chain with one host wait (orbx_track_with_motion_model):
        SearchByProjection(Current, Last, th), again with 2 * th if it found < 20, PoseOptimization from frame["Tcw"] (= mVelocity * mLastFrame.mTcw),
        the discard loop.  frame / last as in SearchByProjectionLast (occupied may be None); inv_level_sigma2 = mvInvLevelSigma2.
        Returns a prepared call: call() -> dict(matches, search_matches, discarded, pose, nmatches_search, wide, n_correspondences, pose_inliers, nmatches,
        nmatches_map, ran_pose, stats); call.raw() is the C call alone on the marshalled arrays (tools/latency_track_chain.py), call.result() the dict."""
        F, keep, n, sf, (minx, maxx, miny, maxy) = self._frame_arrays(frame)
        lk = np.ascontiguousarray(last["kps"], KEYPOINT_DTYPE)
        nl = len(lk)
        cl = np.array([nl], np.int32)
        valid = np.ascontiguousarray(last["valid"], np.uint8)
        pos = np.ascontiguousarray(last["pos"], np.float32)
        ld = np.ascontiguousarray(last["desc"], np.uint8)
        obs = None if last.get("has_obs") is None else np.ascontiguousarray(last["has_obs"], np.uint8)
        octv = np.ascontiguousarray(lk["octave"], np.int32)
        ang = np.ascontiguousarray(lk["angle"], np.float32)
        tc, tl = np.ascontiguousarray(frame["Tcw"], np.float32), np.ascontiguousarray(last["Tcw"], np.float32)
        fx, fy, cx, cy, bf = [np.float32(v) for v in frame["cam"]]
        is2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
        if len(is2) != len(sf):
            raise ValueError("inv_level_sigma2 and scale_factors must have one entry per level")
        Ls = ProjectionLast(_ptr(valid).value, _ptr(pos).value, _ptr(ld).value, None if obs is None else _ptr(obs).value, _ptr(octv).value, _ptr(ang).value,
                            _ptr(cl).value, max(nl, 1), _ptr(tc).value, _ptr(tl).value, float(fx), float(fy), float(cx), float(cy), float(bf), float(bf / fx), maxx, maxy)
        m1 = max(n, 1)
        mt, sm, dc, po = np.full(m1, -1, np.int32), np.full(m1, -1, np.int32), np.zeros(m1, np.uint8), np.zeros(16, np.float32)
        R = TrackMotionResult(_ptr(mt).value, _ptr(sm).value, _ptr(dc).value, _ptr(po).value)
        self._L.orbx_track_with_motion_model.argtypes = [ctypes.c_void_p, ctypes.POINTER(ProjectionFrame), ctypes.POINTER(ProjectionLast), ctypes.c_void_p, ctypes.c_int,
                                                         ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.POINTER(TrackMotionResult)]
        fn, h, psf, pis, cth, cm, co = self._L.orbx_track_with_motion_model, self._h, _ptr(sf), _ptr(is2), ctypes.c_float(th), 1 if mono else 0, 1 if self.checkOri else 0

        def raw():
            return fn(h, ctypes.byref(F), ctypes.byref(Ls), psf, len(sf), pis, cth, cm, co, ctypes.byref(R))

        def result():
            return dict(matches=mt[:n].copy(), search_matches=sm[:n].copy(), discarded=dc[:n].copy(), pose=po.reshape(4, 4).copy(), nmatches_search=R.nmatches_search,
                        wide=R.wide, n_correspondences=R.n_correspondences, pose_inliers=R.pose_inliers, nmatches=R.nmatches, nmatches_map=R.nmatches_map,
                        ran_pose=R.ran_pose, stats=np.array(R.stats[:], np.float64))

        def call():
            _check(raw())
            return result()
        call.raw, call.result, call.F, call.Ls, call.sf = raw, result, F, Ls, sf
        call.keep = [keep, lk, cl, valid, pos, ld, obs, octv, ang, tc, tl, is2, mt, sm, dc, po, R]
        return call

    def TrackLocalMap(self, frame, Tcw, cam, log_scale_factor, points, th, held, held_pos, inv_level_sigma2, sensor_stereo, nnratio=None, viewing_cos_limit=0.5):
        return self.track_local_prepare(frame, Tcw, cam, log_scale_factor, points, th, held, held_pos, inv_level_sigma2, sensor_stereo, nnratio, viewing_cos_limit)()

    def track_local_prepare(self, frame, Tcw, cam, log_scale_factor, points, th, held, held_pos, inv_level_sigma2, sensor_stereo, nnratio=None, viewing_cos_limit=0.5):
        """Tracking::TrackLocalMap (reference src/Tracking.cc:1454-1489) as one device chain with one host wait (orbx_track_local_map): SearchLocalPoints
        (arguments as SearchLocalPoints), PoseOptimization from Tcw over the features that are held (held[n] = 1, position held_pos[n, 3]) or newly
        assigned, the statistics loop.  frame["occupied"][i] = 1 where the held point has observations (may be None).
        Returns a prepared call (as track_motion_prepare): call() -> dict(assigned, nmatches, frustum=dict(in_view, ..), pose, outlier, found, cleared,
        n_correspondences, pose_inliers, inliers_map, inliers_all, stats)."""
        F, keep, n, sf, (minx, maxx, miny, maxy) = self._frame_arrays(frame)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        thr = predict_scale_thresholds(log_scale_factor, len(sf))
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mx, mn = f32(points["pos"]), f32(points["normal"]), f32(points["max_distance"]), f32(points["min_distance"])
        md = np.ascontiguousarray(points["desc"], np.uint8)
        obs = None if points.get("has_obs") is None else np.ascontiguousarray(points["has_obs"], np.uint8)
        m = len(mx)
        hd, hp, is2 = np.ascontiguousarray(held, np.uint8), f32(held_pos), f32(inv_level_sigma2)
        if len(hd) != n or hp.size != 3 * n or len(is2) != len(sf):
            raise ValueError("held / held_pos need one entry per feature, inv_level_sigma2 one per level")
        fr = FrustumFrame(T.ctypes.data, cam[0], cam[1], cam[2], cam[3], cam[4], minx, maxx, miny, maxy, thr.ctypes.data, len(sf), 1)
        P = LocalPoints(pos.ctypes.data, nrm.ctypes.data, mx.ctypes.data, mn.ctypes.data, md.ctypes.data, None if obs is None else obs.ctypes.data, m)
        n1, m1 = max(n, 1), max(m, 1)
        z = lambda dt: np.zeros(m1, dt)
        iv, px, py, pxr, lvl, vc = z(np.uint8), z(np.float32), z(np.float32), z(np.float32), z(np.int32), z(np.float32)
        asg, po = np.full(n1, -1, np.int32), np.zeros(16, np.float32)
        outl, fnd, clr = np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros(n1, np.uint8)
        R = TrackLocalResult(_ptr(asg).value, _ptr(iv).value, _ptr(px).value, _ptr(py).value, _ptr(pxr).value, _ptr(lvl).value, _ptr(vc).value, _ptr(po).value,
                             _ptr(outl).value, _ptr(fnd).value, _ptr(clr).value)
        self._L.orbx_track_local_map.argtypes = [ctypes.c_void_p, ctypes.POINTER(ProjectionFrame), ctypes.POINTER(FrustumFrame), ctypes.POINTER(LocalPoints), ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.POINTER(TrackLocalResult)]
        fn, h, psf, phd, php, pis = self._L.orbx_track_local_map, self._h, _ptr(sf), _ptr(hd), _ptr(hp), _ptr(is2)
        cvc, cth, cnn, cst = ctypes.c_float(viewing_cos_limit), ctypes.c_float(th), ctypes.c_float(self.nnratio if nnratio is None else nnratio), 1 if sensor_stereo else 0

        def raw():
            return fn(h, ctypes.byref(F), ctypes.byref(fr), ctypes.byref(P), psf, len(sf), cvc, cth, cnn, phd, php, pis, cst, ctypes.byref(R))

        def result():
            c = lambda a, k: a[:k].copy()
            return dict(assigned=c(asg, n), nmatches=R.nmatches, frustum=dict(in_view=c(iv, m), proj_x=c(px, m), proj_y=c(py, m), proj_xr=c(pxr, m), level=c(lvl, m), view_cos=c(vc, m)),
                        pose=po.reshape(4, 4).copy(), outlier=c(outl, n), found=c(fnd, n), cleared=c(clr, n), n_correspondences=R.n_correspondences,
                        pose_inliers=R.pose_inliers, inliers_map=R.inliers_map, inliers_all=R.inliers_all, stats=np.array(R.stats[:], np.float64))

        def call():
            _check(raw())
            return result()
        call.raw, call.result, call.F, call.fr, call.P, call.sf = raw, result, F, fr, P, sf
        call.keep = [keep, T, thr, pos, nrm, mx, mn, md, obs, hd, hp, is2, iv, px, py, pxr, lvl, vc, asg, po, outl, fnd, clr, R]
        return call

    def TrackReferenceKeyFrame(self, keyframe, frame, nnratio=None):
        return self.track_reference_prepare(keyframe, frame, nnratio)()

    def track_reference_prepare(self, keyframe, frame, nnratio=None):
        """Tracking::TrackReferenceKeyFrame (reference src/Tracking.cc:1189-1238) as one device chain with one host wait (orbx_track_reference_keyframe):
        SearchByBoW(pKF, F) with nnratio (default the handle's; 0.7 at :1189) and the handle's checkOri, PoseOptimization from frame["Tcw"]
        (= mLastFrame.mTcw) if it found >= 15, the discard loop.
        keyframe: dict(kps (mvKeysUn), desc, pos (n, 3) world positions of the slots' points[, groups, valid, has_obs]);
        frame: dict(kps (mvKeys), desc, kps_un (mvKeysUn), u_right, Tcw, cam (fx, fy, cx, cy, bf), inv_level_sigma2[, groups]).
        Returns a prepared call (as track_motion_prepare): call() -> dict(matches, search_matches, discarded, pose, nmatches_search, n_correspondences,
        pose_inliers, nmatches, nmatches_map, ran_pose, stats); matches name keyframe slots."""
        fa, ka = _host_set(keyframe["kps"], keyframe["desc"], keyframe.get("groups"), keyframe.get("valid"))
        fb, kb = _host_set(frame["kps"], frame["desc"], frame.get("groups"))
        na, n = len(ka[0]), len(kb[0])
        pos = np.ascontiguousarray(keyframe["pos"], np.float32)
        obs = None if keyframe.get("has_obs") is None else np.ascontiguousarray(keyframe["has_obs"], np.uint8)
        ku = np.ascontiguousarray(frame["kps_un"], KEYPOINT_DTYPE)
        ur = np.ascontiguousarray(frame["u_right"], np.float32)
        tc = np.ascontiguousarray(frame["Tcw"], np.float32).reshape(16)
        is2 = np.ascontiguousarray(frame["inv_level_sigma2"], np.float32)
        if pos.size != 3 * na or len(ku) != n or len(ur) != n or (obs is not None and len(obs) != na):
            raise ValueError("pos / has_obs need one entry per keyframe feature, kps_un / u_right one per frame feature")
        fx, fy, cx, cy, bf = [float(np.float32(v)) for v in frame["cam"]]
        KF = ReferenceKeyFrame(ctypes.pointer(fa), _ptr(pos).value, None if obs is None else _ptr(obs).value)
        FR = ReferenceFrame(ctypes.pointer(fb), _ptr(ku).value, _ptr(ur).value, _ptr(tc).value, fx, fy, cx, cy, bf, _ptr(is2).value, len(is2))
        m1 = max(n, 1)
        mt, sm, dc, po = np.full(m1, -1, np.int32), np.full(m1, -1, np.int32), np.zeros(m1, np.uint8), np.zeros(16, np.float32)
        R = TrackReferenceResult(_ptr(mt).value, _ptr(sm).value, _ptr(dc).value, _ptr(po).value)
        self._L.orbx_track_reference_keyframe.argtypes = [ctypes.c_void_p, ctypes.POINTER(ReferenceKeyFrame), ctypes.POINTER(ReferenceFrame), ctypes.c_float, ctypes.c_int,
                                                          ctypes.POINTER(TrackReferenceResult)]
        fn, h, cnn, co = self._L.orbx_track_reference_keyframe, self._h, ctypes.c_float(self.nnratio if nnratio is None else nnratio), 1 if self.checkOri else 0

        def raw():
            return fn(h, ctypes.byref(KF), ctypes.byref(FR), cnn, co, ctypes.byref(R))

        def result():
            return dict(matches=mt[:n].copy(), search_matches=sm[:n].copy(), discarded=dc[:n].copy(), pose=po.reshape(4, 4).copy(), nmatches_search=R.nmatches_search,
                        n_correspondences=R.n_correspondences, pose_inliers=R.pose_inliers, nmatches=R.nmatches, nmatches_map=R.nmatches_map, ran_pose=R.ran_pose,
                        stats=np.array(R.stats[:], np.float64))

        def call():
            _check(raw())
            return result()
        call.raw, call.result, call.KF, call.FR = raw, result, KF, FR
        call.keep = [fa, ka, fb, kb, pos, obs, ku, ur, tc, is2, mt, sm, dc, po, R]
        return call

    def RelocMatchCandidates(self, frame, keyframes, nnratio=None):
        return self.reloc_match_prepare(frame, keyframes, nnratio)()

    def reloc_match_prepare(self, frame, keyframes, nnratio=None):
        """The head of Tracking::Relocalization (reference src/Tracking.cc:2063-2095) as one device chain with one host wait (orbx_reloc_match_candidates):
        SearchByBoW(pKF, F) for every candidate keyframe with nnratio (default the handle's; 0.75 at :2048) and the handle's checkOri, the < 15 decision, and
        the arrays the PnPsolver constructor collects (src/PnPsolver.cc:120-167).
        frame: dict(kps (mvKeys), desc, kps_un (mvKeysUn), level_sigma2 (mvLevelSigma2)[, groups, cam (fx, fy, cx, cy, ..)]);
        keyframes: list of dict(kps, desc, pos[, groups, valid, bad]) - a bad keyframe needs nothing but bad=True.
        Returns a prepared call: call() -> dict(matches (K, N), nmatches (K), discarded (K), n (K), key_index / p2d / sigma2 / p3dw: lists of K arrays with
        n[k] rows, problems: one dict(candidate, K, p2d, sigma2, p3d, indices, mN) per kept candidate - PnPsolver.Solve takes the list as its candidates
        (K is there if the frame names cam), with the caller's sets or its own)."""
        fb, kb = _host_set(frame["kps"], frame["desc"], frame.get("groups"))
        n = len(kb[0])
        ku = np.ascontiguousarray(frame["kps_un"], KEYPOINT_DTYPE)
        s2 = np.ascontiguousarray(frame["level_sigma2"], np.float32)
        if len(ku) != n:
            raise ValueError("kps_un needs one entry per frame feature")
        K = len(keyframes)
        kfs, keep = (RelocMatchKeyFrame * max(K, 1))(), []
        for k, kf in enumerate(keyframes):
            if kf.get("bad"):
                kfs[k] = RelocMatchKeyFrame(None, None, 1)
                continue
            fa, ka = _host_set(kf["kps"], kf["desc"], kf.get("groups"), kf.get("valid"))
            pos = np.ascontiguousarray(kf["pos"], np.float32)
            if pos.size != 3 * len(ka[0]):
                raise ValueError("pos needs one row per keyframe feature")
            keep.append((fa, ka, pos))
            kfs[k] = RelocMatchKeyFrame(ctypes.pointer(fa), _ptr(pos).value, 0)
        FR = RelocMatchFrame(ctypes.pointer(fb), _ptr(ku).value, _ptr(s2).value, len(s2))
        k1, n1 = max(K, 1), max(n, 1)
        mt, ki = np.full((k1, n1), -1, np.int32), np.full((k1, n1), -1, np.int32)
        p2, sg, p3 = np.zeros((k1, n1, 2), np.float32), np.zeros((k1, n1), np.float32), np.zeros((k1, n1, 3), np.float32)
        nn, nm, dc = np.zeros(k1, np.int32), np.zeros(k1, np.int32), np.zeros(k1, np.uint8)
        if n == 0:
            mt = np.full((k1, 0), -1, np.int32)
        R = RelocMatchResult(*[_ptr(a).value if a.size else None for a in (mt, ki, p2, sg, p3, nn, nm, dc)])
        self._L.orbx_reloc_match_candidates.argtypes = [ctypes.c_void_p, ctypes.POINTER(RelocMatchFrame), ctypes.POINTER(RelocMatchKeyFrame), ctypes.c_int, ctypes.c_float,
                                                        ctypes.c_int, ctypes.POINTER(RelocMatchResult)]
        fn, h, cnn, co = self._L.orbx_reloc_match_candidates, self._h, ctypes.c_float(self.nnratio if nnratio is None else nnratio), 1 if self.checkOri else 0
        cam = frame.get("cam")

        def raw():
            return fn(h, ctypes.byref(FR), kfs, K, cnn, co, ctypes.byref(R))

        def result():
            cut = lambda a: [a[k, :nn[k]].copy() for k in range(K)]
            out = dict(matches=mt[:K, :n].copy(), nmatches=nm[:K].copy(), discarded=dc[:K].copy(), n=nn[:K].copy(), key_index=cut(ki), p2d=cut(p2), sigma2=cut(sg), p3dw=cut(p3))
            out["problems"] = [dict(candidate=k, p2d=out["p2d"][k], sigma2=out["sigma2"][k], p3d=out["p3dw"][k], indices=out["key_index"][k], mN=n,
                                    **({} if cam is None else {"K": tuple(cam[:4])})) for k in range(K) if not dc[k]]
            return out

        def call():
            _check(raw())
            return result()
        call.raw, call.result, call.FR, call.kfs = raw, result, FR, kfs
        call.keep = [fb, kb, ku, s2, keep, mt, ki, p2, sg, p3, nn, nm, dc, R]
        return call

    def track_kernel_times(self, on=None):
        """profile_kernels tap of the chains above: track_kernel_times(True / False) switches the events between their launches on or off;
        track_kernel_times() returns the device milliseconds between the launches of the last profiled call."""
        self._L.orbx_track_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self._L.orbx_track_last_kernel_times.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        if on is not None:
            _check(self._L.orbx_track_set_profiling(self._h, 1 if on else 0))
            return None
        ms, cnt = np.zeros(8, np.float32), ctypes.c_int()
        _check(self._L.orbx_track_last_kernel_times(self._h, _ptr(ms), 8, ctypes.byref(cnt)))
        return ms[:cnt.value].copy()

    def StereoHamming(self, kpsL, descL, kpsR, descR, scale_factors, max_disparity=float("inf")):
        fl, kl = _host_set(kpsL, descL)
        fr, kr = _host_set(kpsR, descR)
        n = len(kpsL)
        bd = np.zeros(max(n, 1), np.int32)
        bi = np.zeros(max(n, 1), np.int32)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        _check(self._L.orbx_stereo_match(self._h, ctypes.byref(fl), ctypes.byref(fr), _ptr(sf), len(sf), ctypes.c_float(max_disparity), _ptr(bd), _ptr(bi)))
        return bd[:n], bi[:n]

    # ---- batched, device resident: features straight from an extractor's last batch ----
    @staticmethod
    def features_of(extractor, nframes):
        k, d, c, cap = extractor.results_device()
        return FeatureSet(k.value, d.value, c.value, None, None, cap, nframes)

    def search_by_bow_device(self, fsA, fsB, pairsA, pairsB, mode=0, after=None):
        pa = np.ascontiguousarray(pairsA, np.int32)
        pb = np.ascontiguousarray(pairsB, np.int32)
        prm = BowParams(self.nnratio, 1 if self.checkOri else 0, mode)
        _check(self._L.orbx_search_by_bow_device(self._h, ctypes.byref(fsA), ctypes.byref(fsB), _ptr(pa), _ptr(pb), len(pa), ctypes.byref(prm),
                                                 after._h if after is not None else None))

    def stereo_match_device(self, fsL, fsR, pairsL, pairsR, scale_factors, max_disparity=float("inf"), after=None):
        pl = np.ascontiguousarray(pairsL, np.int32)
        pr = np.ascontiguousarray(pairsR, np.int32)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        _check(self._L.orbx_stereo_match_device(self._h, ctypes.byref(fsL), ctypes.byref(fsR), _ptr(pl), _ptr(pr), len(pl), _ptr(sf), len(sf),
                                                ctypes.c_float(max_disparity), after._h if after is not None else None))

    def compute_stereo_matches_device(self, ext_left, ext_right, frames_l, frames_r, mbf, mb=0.0):
        """Frame::ComputeStereoMatches (reference src/Frame.cc:1026-1420), complete, on the last batches
        of two extractor handles (may be the same handle).  mb=0 is what the reference's stereo
        constructor has when the function runs (src/Frame.cc:125)."""
        fl = np.ascontiguousarray(frames_l, np.int32)
        fr = np.ascontiguousarray(frames_r, np.int32)
        _check(self._L.orbx_compute_stereo_matches_device(self._h, ext_left._h, ext_right._h, _ptr(fl), _ptr(fr), len(fl),
                                                          ctypes.c_float(mbf), ctypes.c_float(mb)))

    def stereo_frame(self, ext_left, ext_right, mbf, mb=0.0, n=None):
        """Frame::ComputeStereoMatches of ONE stereo frame, after the two extractors' single-frame calls (orbx_stereo_frame): (mvuRight, mvDepth)."""
        n = self.max_features if n is None else int(n)
        u = np.full(n, -1.0, np.float32)
        z = np.full(n, -1.0, np.float32)
        _check(self._L.orbx_stereo_frame(self._h, ext_left._h, ext_right._h, ctypes.c_float(mbf), ctypes.c_float(mb), _ptr(u), _ptr(z), n))
        return u, z

    def download_stereo(self, npairs, stride=None):
        """(mvuRight, mvDepth) per pair, -1 where the reference leaves -1."""
        stride = stride or self.max_features
        u = np.zeros((npairs, stride), np.float32)
        z = np.zeros((npairs, stride), np.float32)
        _check(self._L.orbx_stereo_download(self._h, npairs, _ptr(u), _ptr(z), stride))
        return u, z

    def sync(self):
        _check(self._L.orbx_matcher_sync(self._h))

    def download(self, npairs, stride=None):
        stride = stride or self.max_features
        m = np.zeros((npairs, stride), np.int32)
        d = np.zeros((npairs, stride), np.int32)
        n = np.zeros(npairs, np.int32)
        _check(self._L.orbx_matcher_download(self._h, npairs, _ptr(m), _ptr(d), stride, _ptr(n)))
        return m, d, n

    def last_timing(self):
        return self._timing("orbx_matcher_last_timing", ctypes.c_float)[0]

    def last_kernel_timing(self):
        """(distance kernels ms, greedy replay ms) of the SearchByBoW calls averaged by the last last_timing()."""
        return self._timing("orbx_matcher_last_kernel_timing", ctypes.c_float, ctypes.c_float)

    def _reloc_frame(self, frame, inv_level_sigma2=None, features=True):
        """orbx_reloc_frame from frame = dict(cam = (fx, fy, cx, cy, bf), scale_factors, log_scale_factor, width, height[, min_x ..][, kps, desc, u_right])."""
        sf = np.ascontiguousarray(frame["scale_factors"], np.float32)
        minx, miny = np.float32(frame.get("min_x", 0.0)), np.float32(frame.get("min_y", 0.0))
        maxx, maxy = np.float32(frame.get("max_x", frame["width"])), np.float32(frame.get("max_y", frame["height"]))
        gw, gh = np.float32(64) / (maxx - minx), np.float32(48) / (maxy - miny)
        keep = [sf]
        if features:
            k = np.ascontiguousarray(frame["kps"], KEYPOINT_DTYPE)
            n = len(k)
            d, ur, cn = np.ascontiguousarray(frame["desc"], np.uint8), np.ascontiguousarray(frame["u_right"], np.float32), np.array([n], np.int32)
            F = ProjectionFrame(_ptr(k).value, _ptr(d).value, _ptr(ur).value, None, _ptr(cn).value, max(n, 1), 1, float(minx), float(miny), float(gw), float(gh))
            keep += [k, d, ur, cn]
        else:
            n = 0
            F = ProjectionFrame(None, None, None, None, None, 1, 1, float(minx), float(miny), float(gw), float(gh))
        rt = np.ascontiguousarray(np.concatenate([predict_scale_thresholds(frame["log_scale_factor"], len(sf)), np.zeros(1, np.float32)]), np.float32)
        is2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        if is2 is not None and len(is2) != len(sf):
            raise ValueError("inv_level_sigma2 and scale_factors must have one entry per level")
        fx, fy, cx, cy, bf = [float(np.float32(v)) for v in frame["cam"]]
        R = RelocFrame(F, fx, fy, cx, cy, bf, float(maxx), float(maxy), _ptr(sf).value, _ptr(rt).value, None if is2 is None else _ptr(is2).value, len(sf),
                       1 if self.checkOri else 0)
        keep += [rt, is2, F]
        return R, keep, n

    @staticmethod
    def _reloc_candidate(c, n=None):
        """orbx_reloc_candidate from dict(valid, pos, max_distance (mfMaxDistance), min_distance[, desc, kf_angle, bow_match])."""
        valid = np.ascontiguousarray(c["valid"], np.uint8)
        npts = len(valid)
        pos = np.ascontiguousarray(np.asarray(c["pos"], np.float32).reshape(-1, 3))
        mx, mn = np.ascontiguousarray(c["max_distance"], np.float32), np.ascontiguousarray(c["min_distance"], np.float32)
        d = None if c.get("desc") is None else np.ascontiguousarray(c["desc"], np.uint8)
        ang = None if c.get("kf_angle") is None else np.ascontiguousarray(c["kf_angle"], np.float32)
        bow = None if c.get("bow_match") is None else np.ascontiguousarray(c["bow_match"], np.int32)
        if bow is not None and n is not None and len(bow) != n:
            raise ValueError("bow_match must have one entry per frame feature")
        if len(pos) != npts or len(mx) != npts or len(mn) != npts or (d is not None and len(d) != npts) or (ang is not None and len(ang) != npts):
            raise ValueError("the arrays of a candidate must have one entry per slot")
        opt = lambda a: None if a is None else _ptr(a).value
        return RelocCandidate(npts, _ptr(valid).value, _ptr(pos).value, _ptr(mx).value, _ptr(mn).value, opt(d), opt(ang), opt(bow)), [valid, pos, mx, mn, d, ang, bow]

    def RelocProject(self, frame, cand, Tcw, found, th):
        """The projection stage of the relocalisation chain on explicit inputs (orbx_reloc_project; reference src/ORBmatcher.cc:1735-1790): per keyframe slot the
        query of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist).  found: [npoints] flags or None.
        Returns dict(u, v, radius, min_level, max_level, active)."""
        R, keep, _ = self._reloc_frame(frame, features=False)
        C, keepc = self._reloc_candidate(cand)
        T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
        fnd = None if found is None else np.ascontiguousarray(found, np.uint8)
        m = max(C.npoints, 1)
        u, v, r = np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32)
        lo, hi, act = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
        self._L.orbx_reloc_project.argtypes = [ctypes.c_void_p, ctypes.POINTER(RelocFrame), ctypes.POINTER(RelocCandidate), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float] + \
                                              [ctypes.c_void_p] * 6
        _check(self._L.orbx_reloc_project(self._h, ctypes.byref(R), ctypes.byref(C), _ptr(T), None if fnd is None else _ptr(fnd), ctypes.c_float(th), _ptr(u), _ptr(v), _ptr(r),
                                          _ptr(lo), _ptr(hi), _ptr(act)))
        k = C.npoints
        return dict(u=u[:k], v=v[:k], radius=r[:k], min_level=lo[:k], max_level=hi[:k], active=act[:k])

    def RelocalizeRefine(self, frame, cands, hyps, sequence, inv_level_sigma2, pnp=None, keypoint_index=None):
        return self.reloc_prepare(frame, cands, hyps, sequence, inv_level_sigma2, pnp, keypoint_index)()

    def reloc_prepare(self, frame, cands, hyps, sequence, inv_level_sigma2, pnp=None, keypoint_index=None):
        """The refine loop of Tracking::Relocalization (reference src/Tracking.cc:2135-2223) for all hypotheses of all candidates as one device chain with one
        host wait (orbx_relocalize_refine).  frame: dict(kps, desc, u_right, scale_factors, log_scale_factor, cam, width, height[, min_x ..]); cands: list of
        dict(valid, pos, max_distance, min_distance, desc, kf_angle, bow_match[N]); hyps: list of dict(candidate, Tcw, inliers[N]); sequence: indices into hyps.
        Returns a prepared call: call() -> dict(stage[H], success[H], ngood[H, 3], nadditional[H, 2], n_correspondences[H, 3], pose[H, 4, 4], stats[H, 3, 8],
        map_point[N], outlier[N], winner, hypothesis, candidate); call.raw() is the C call alone on the marshalled arrays.
        pnp = a PnPsolver whose last Solve was over these candidates, in this order: hyps is then a list of dict(candidate, record) and every hypothesis' pose and
        mask are the record's refined ones, read where that solve left them on the device (no mask crosses to the host); keypoint_index[c] = mvKeyPointIndices of
        candidate c (compacted match -> frame feature; None for a candidate no hypothesis names)."""
        R, keep, n = self._reloc_frame(frame, inv_level_sigma2)
        cs = [self._reloc_candidate(c, n) for c in cands]
        CA = (RelocCandidate * max(len(cs), 1))(*[c[0] for c in cs])
        H = len(hyps)
        hc = np.ascontiguousarray([int(h["candidate"]) for h in hyps], np.int32)
        sq = np.ascontiguousarray(sequence, np.int32)
        if pnp is None:
            ht = np.ascontiguousarray(np.stack([np.asarray(h["Tcw"], np.float32).reshape(-1)[:12] for h in hyps]) if H else np.zeros((0, 12), np.float32))
            hm = np.ascontiguousarray(np.stack([np.asarray(h["inliers"], np.uint8) for h in hyps]) if H else np.zeros((0, n), np.uint8))
            if H and hm.shape[1] != n:
                raise ValueError("inliers must have one entry per frame feature")
            HY = RelocHypotheses(H, _ptr(hc).value, _ptr(ht).value, _ptr(hm).value, _ptr(sq).value, len(sq), None, None, None, None)
        else:
            ht = np.ascontiguousarray([int(h["record"]) for h in hyps], np.int32)
            ki = [None if k is None else np.ascontiguousarray(k, np.int32) for k in (keypoint_index if keypoint_index is not None else [None] * len(cs))]
            if len(ki) != len(cs):
                raise ValueError("keypoint_index must have one entry per candidate")
            kp = (ctypes.c_void_p * max(len(ki), 1))(*[None if k is None else _ptr(k).value for k in ki])
            hm = [ki, kp, np.ascontiguousarray([0 if k is None else len(k) for k in ki], np.int32), pnp]
            HY = RelocHypotheses(H, _ptr(hc).value, None, None, _ptr(sq).value, len(sq), pnp._h, _ptr(ht).value, ctypes.cast(kp, ctypes.c_void_p), _ptr(hm[2]).value)
        h1, n1 = max(H, 1), max(n, 1)
        stage, succ, ng, na, nc = np.zeros(h1, np.int32), np.zeros(h1, np.int32), np.zeros((h1, 3), np.int32), np.zeros((h1, 2), np.int32), np.zeros((h1, 3), np.int32)
        pose, stats, mp, outl = np.zeros((h1, 4, 4), np.float32), np.zeros((h1, 3, 8), np.float64), np.full(n1, -1, np.int32), np.zeros(n1, np.uint8)
        RS = RelocResult(*[_ptr(a).value for a in (stage, succ, ng, na, nc, pose, stats, mp, outl)])
        self._L.orbx_relocalize_refine.argtypes = [ctypes.c_void_p, ctypes.POINTER(RelocFrame), ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RelocHypotheses),
                                                   ctypes.POINTER(RelocResult)]
        fn, hnd, nca = self._L.orbx_relocalize_refine, self._h, len(cs)

        def raw():
            return fn(hnd, ctypes.byref(R), ctypes.cast(CA, ctypes.c_void_p), nca, ctypes.byref(HY), ctypes.byref(RS))

        def result():
            return dict(stage=stage[:H].copy(), success=succ[:H].copy(), ngood=ng[:H].copy(), nadditional=na[:H].copy(), n_correspondences=nc[:H].copy(), pose=pose[:H].copy(),
                        stats=stats[:H].copy(), map_point=mp[:n].copy(), outlier=outl[:n].copy(), winner=RS.winner, hypothesis=RS.hypothesis, candidate=RS.candidate)

        def call():
            _check(raw())
            return result()
        call.raw, call.result = raw, result
        call.keep = [keep, cs, CA, hc, ht, hm, sq, HY, stage, succ, ng, na, nc, pose, stats, mp, outl, RS, R]
        return call

    @staticmethod
    def _loop_keyframe(kf, n1=None):
        """orbx_loop_sim3_keyframe from dict(kps, desc, Rcw (3,3), tcw (3), cam = (fx, fy, cx, cy), scale_factors, log_scale_factor, inv_level_sigma2, width, height
        [, min_x ..], valid, pos, max_distance (mfMaxDistance), min_distance, point_desc[, bow_match [N1]])."""
        f4 = np.float32
        k = np.ascontiguousarray(kf["kps"], KEYPOINT_DTYPE)
        n = len(k)
        d, cn = np.ascontiguousarray(kf["desc"], np.uint8), np.array([n], np.int32)
        sf, is2 = np.ascontiguousarray(kf["scale_factors"], f4), np.ascontiguousarray(kf["inv_level_sigma2"], f4)
        if len(is2) != len(sf):
            raise ValueError("inv_level_sigma2 and scale_factors must have one entry per level")
        rt = np.ascontiguousarray(np.concatenate([predict_scale_thresholds(kf["log_scale_factor"], len(sf)), np.zeros(1, f4)]), f4)
        minx, miny = f4(kf.get("min_x", 0.0)), f4(kf.get("min_y", 0.0))
        maxx, maxy = f4(kf.get("max_x", kf["width"])), f4(kf.get("max_y", kf["height"]))
        gw, gh = f4(64) / (maxx - minx), f4(48) / (maxy - miny)
        valid = np.ascontiguousarray(kf["valid"], np.uint8)
        pos = np.ascontiguousarray(np.asarray(kf["pos"], f4).reshape(-1, 3))
        mx, mn = np.ascontiguousarray(kf["max_distance"], f4), np.ascontiguousarray(kf["min_distance"], f4)
        pd = np.ascontiguousarray(kf["point_desc"], np.uint8)
        bow = None if kf.get("bow_match") is None else np.ascontiguousarray(kf["bow_match"], np.int32)
        if not (len(valid) == len(pos) == len(mx) == len(mn) == len(pd) == len(d) == n):
            raise ValueError("the arrays of a keyframe must have one entry per slot")
        if bow is not None and n1 is not None and len(bow) != n1:
            raise ValueError("bow_match must have one entry per feature of the first keyframe")
        F = ProjectionFrame(_ptr(k).value, _ptr(d).value, None, None, _ptr(cn).value, max(n, 1), 1, float(minx), float(miny), float(gw), float(gh))
        K = LoopSim3KeyFrame()
        K.frame = F
        K.rcw = (ctypes.c_float * 9)(*np.asarray(kf["Rcw"], f4).reshape(-1))
        K.tcw = (ctypes.c_float * 3)(*np.asarray(kf["tcw"], f4).reshape(-1))
        K.fx, K.fy, K.cx, K.cy = [float(f4(v)) for v in kf["cam"][:4]]
        K.min_x, K.max_x, K.min_y, K.max_y = [float(f4(int(v))) for v in (minx, maxx, miny, maxy)]      # KeyFrame keeps the bounds as int
        K.scale_factors, K.ratio_thresholds, K.inv_level_sigma2, K.nlevels = _ptr(sf).value, _ptr(rt).value, _ptr(is2).value, len(sf)
        K.valid, K.world_pos, K.max_distance, K.min_distance, K.descriptors = [_ptr(a).value for a in (valid, pos, mx, mn, pd)]
        K.bow_match = None if bow is None else _ptr(bow).value
        return K, [k, d, cn, sf, is2, rt, valid, pos, mx, mn, pd, bow], n

    def LoopRefineSim3(self, kf1, cands, hyps, sim3=None, index1=None, th=7.5, th2=10, fix_scale=False, full=False):
        return self.loop_refine_prepare(kf1, cands, hyps, sim3, index1, th, th2, fix_scale, full)()

    def loop_refine_prepare(self, kf1, cands, hyps, sim3=None, index1=None, th=7.5, th2=10, fix_scale=False, full=False):
        """The refine step of LoopClosing::ComputeSim3 (reference src/LoopClosing.cc:435-480) for all Sim3Solver events of all candidates as one device chain with
        one host wait (orbx_loop_refine_sim3).  kf1 / cands: dicts as _loop_keyframe takes them (cands with bow_match [N1]); hyps: the events in walk order
        (loop_sim3_sequence), each dict(candidate, R12 (3,3), t12 (3), s12, inliers [N1]) (loop_sim3_hypotheses).
        sim3 = a Sim3Solver whose last Solve was over these candidates, in this order: hyps is then a list of dict(candidate, iteration), every model and mask
        is read where that solve left it on the device, and index1[c] = mvnIndices1 of candidate c (None for a candidate no hypothesis names).
        Returns a prepared call: call() -> dict(status [H] (0 failed, 1 success, 2 more than 1024 pairs), n_found, n_pairs, n_inliers, n_bad [H], quat [H, 4], t [H, 3],
        s [H], scw [H, 4, 4], matches12 [N1] of the winner, winner, hypothesis, candidate; full=True adds query_u / query_v / query_radius / query_level /
        query_active [H, 2, NP] and match1 / match2 [H, NP]); call.raw() is the C call alone and returns its code, call.result() reads the arrays."""
        K1, keep1, n1 = self._loop_keyframe(kf1)
        cs = [self._loop_keyframe(c, n1) for c in cands]
        CA = (LoopSim3KeyFrame * max(len(cs), 1))(*[c[0] for c in cs])
        H = len(hyps)
        NP = max([n1] + [c[2] for c in cs] + [1])
        hc = np.ascontiguousarray([int(h["candidate"]) for h in hyps], np.int32)
        HY = LoopSim3Hypotheses()
        HY.count, HY.candidate = H, _ptr(hc).value
        if sim3 is None:
            hr = np.ascontiguousarray(np.stack([np.asarray(h["R12"], np.float32).reshape(9) for h in hyps]) if H else np.zeros((0, 9), np.float32))
            ht = np.ascontiguousarray(np.stack([np.asarray(h["t12"], np.float32).reshape(3) for h in hyps]) if H else np.zeros((0, 3), np.float32))
            hs = np.ascontiguousarray([np.float32(h["s12"]) for h in hyps], np.float32)
            hm = np.ascontiguousarray(np.stack([np.asarray(h["inliers"], np.uint8) for h in hyps]) if H else np.zeros((0, n1), np.uint8))
            if H and hm.shape[1] != n1:
                raise ValueError("inliers must have one entry per feature of the first keyframe")
            HY.r12, HY.t12, HY.s12, HY.inliers = _ptr(hr).value, _ptr(ht).value, _ptr(hs).value, _ptr(hm).value
            hk = [hr, ht, hs, hm]
        else:
            hi = np.ascontiguousarray([int(h["iteration"]) for h in hyps], np.int32)
            ix = [None if k is None else np.ascontiguousarray(k, np.int32) for k in (index1 if index1 is not None else [None] * len(cs))]
            if len(ix) != len(cs):
                raise ValueError("index1 must have one entry per candidate")
            ip = (ctypes.c_void_p * max(len(ix), 1))(*[None if k is None else _ptr(k).value for k in ix])
            ic = np.ascontiguousarray([0 if k is None else len(k) for k in ix], np.int32)
            HY.solver, HY.iteration, HY.index1, HY.index1_count = sim3._h, _ptr(hi).value, ctypes.cast(ip, ctypes.c_void_p), _ptr(ic).value
            hk = [hi, ix, ip, ic, sim3]
        h1, m1 = max(H, 1), max(n1, 1)
        i4, f4, f8, u1 = np.int32, np.float32, np.float64, np.uint8
        o = dict(status=np.zeros(h1, i4), n_found=np.zeros(h1, i4), n_pairs=np.zeros(h1, i4), n_inliers=np.zeros(h1, i4), n_bad=np.zeros(h1, i4), quat=np.zeros((h1, 4), f8),
                 t=np.zeros((h1, 3), f8), s=np.zeros(h1, f8), scw=np.zeros((h1, 4, 4), f4), matches12=np.full(m1, -1, i4))
        if full:
            o.update(query_u=np.zeros((h1, 2, NP), f4), query_v=np.zeros((h1, 2, NP), f4), query_radius=np.zeros((h1, 2, NP), f4), query_level=np.zeros((h1, 2, NP), i4),
                     query_active=np.zeros((h1, 2, NP), u1), match1=np.full((h1, NP), -1, i4), match2=np.full((h1, NP), -1, i4))
        RS = LoopRefineResult(*[_ptr(o[k]).value if k in o else None for k in _LOOP_REFINE_ARRAYS])
        fn, hnd, nca = self._L.orbx_loop_refine_sim3, self._h, len(cs)
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(LoopSim3KeyFrame), ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(LoopSim3Hypotheses), ctypes.c_float, ctypes.c_float,
                       ctypes.c_int, ctypes.POINTER(LoopRefineResult)]
        cth, cth2, cfix = ctypes.c_float(th), ctypes.c_float(th2), 1 if fix_scale else 0

        def raw():
            return fn(hnd, ctypes.byref(K1), ctypes.cast(CA, ctypes.c_void_p), nca, ctypes.byref(HY), cth, cth2, cfix, ctypes.byref(RS))

        def result():
            r = {k: (v[:n1].copy() if k == "matches12" else v[:H].copy()) for k, v in o.items()}
            r.update(winner=RS.winner, hypothesis=RS.hypothesis, candidate=RS.candidate)
            return r

        def call():
            _check(raw())
            return result()
        call.raw, call.result = raw, result
        call.keep = [keep1, cs, CA, hc, hk, HY, o, RS, K1]
        return call

    def loop_refine_last_timing(self):
        """(device ms of the last LoopRefineSim3 chain, kernel launches)"""
        return self._timing("orbx_loop_sim3_last_timing", ctypes.c_float, ctypes.c_int)


# =====================================================================================
# Optimizer::LocalBundleAdjustment numerical core over the C ABI
# =====================================================================================
class Vocabulary(_Handle):
    """DBoW2 vocabulary tree on the device: transform() == TemplatedVocabulary::transform
    (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1262), i.e. Frame::ComputeBoW."""
    _destroy = "orbx_vocabulary_destroy"

    @staticmethod
    def _bind(L):
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_vocabulary_create.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, ctypes.POINTER(vp)]
        L.orbx_vocabulary_destroy.argtypes = [vp]
        L.orbx_vocabulary_destroy.restype = None
        L.orbx_vocabulary_words.argtypes = [vp]
        L.orbx_bow_transform_device.argtypes = [vp, vp, ci]
        L.orbx_bow_results_device.argtypes = [vp, vp, vp, vp, vp]
        L.orbx_bow_download.argtypes = [vp, vp, ci, vp, vp, vp]
        L.orbx_bow_transform.argtypes = [vp, vp, ci, ci, vp, vp, vp]

    def __init__(self, voc, device=0):
        self._L = load_library()
        L = self._L
        vp = ctypes.c_void_p
        self._bind(L)
        self._h = vp()
        par = np.ascontiguousarray(voc["parent"], np.int32)
        leaf = np.ascontiguousarray(voc["is_leaf"], np.uint8)
        desc = np.ascontiguousarray(voc["desc"], np.uint8)
        wt = np.ascontiguousarray(voc["weight"], np.float64)
        _check(L.orbx_vocabulary_create(device, int(voc["k"]), int(voc["L"]), len(par), _ptr(par), _ptr(leaf), _ptr(desc), _ptr(wt), ctypes.byref(self._h)))

    @classmethod
    def from_text(cls, path_or_bytes, device=0):
        """ORBVocabulary::loadFromTextFile on the device (orbx_vocabulary_load_text / _load_text_buffer): a path, or the text itself as bytes.
        .text_info: the header, the node and word counts, final_newline, host_lines, launches, waits and the times of the load."""
        v = cls.__new__(cls)
        v._L = load_library()
        cls._bind(v._L)
        _bind_voc_text(v._L)
        v._h = ctypes.c_void_p()
        info = VocTextInfo()
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            data = bytes(path_or_bytes)
            rc = v._L.orbx_vocabulary_load_text_buffer(device, data, len(data), ctypes.byref(v._h), ctypes.byref(info))
        else:
            rc = v._L.orbx_vocabulary_load_text(device, os.fsencode(path_or_bytes), ctypes.byref(v._h), ctypes.byref(info))
        v.text_info = info.as_dict()
        if rc != ORBX_OK:
            e = OrbxError(rc, v._L.orbx_last_error().decode("utf-8", "replace"))
            e.text_info = v.text_info
            raise e
        return v

    def tree(self):
        """the tree of this vocabulary - loaded, created or trained - as voc_synth's dict (orbx_vocabulary_tree)"""
        _bind_voc_text(self._L)
        k, L, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(self._L.orbx_vocabulary_tree(self._h, ctypes.byref(k), ctypes.byref(L), ctypes.byref(n), None, None, None, None))
        par, leaf, desc, wt = np.zeros(n.value, np.int32), np.zeros(n.value, np.uint8), np.zeros((n.value, 32), np.uint8), np.zeros(n.value, np.float64)
        _check(self._L.orbx_vocabulary_tree(self._h, None, None, None, _ptr(par), _ptr(leaf), _ptr(desc), _ptr(wt)))
        return dict(k=k.value, L=L.value, parent=par, is_leaf=leaf, desc=desc, weight=wt, num_nodes=n.value)

    def close(self):
        if getattr(self, "_job", None) is not None and self._job.value:      # (a job only reads the vocabulary and must go first)
            self._L.orbx_bow_job_destroy(self._job)
            self._job = None
        super().close()

    def size(self):
        return self._L.orbx_vocabulary_words(self._h)

    def transform(self, descriptors, levelsup=4):
        """(word id, FeatureVector node id or -1, word weight) per descriptor."""
        d = np.ascontiguousarray(descriptors, np.uint8)
        n = len(d)
        w, nd, wt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        _check(self._L.orbx_bow_transform(self._h, _ptr(d), n, levelsup, _ptr(w), _ptr(nd), _ptr(wt)))
        return w[:n], nd[:n], wt[:n]

    def transform_sorted(self, descriptors, levelsup=4):
        """transform() plus the two orders of its std::map fills: (word, node, weight, by_word, by_node) - by_word[k] / by_node[k] = the feature that is
        k-th by (word id, index) / (node id, index) among the filed features (orbx_bow_transform_sorted)."""
        d = np.ascontiguousarray(descriptors, np.uint8)
        n = len(d)
        w, nd, wt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        bw, bn = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        filed = ctypes.c_int32()
        self._L.orbx_bow_transform_sorted.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
        _check(self._L.orbx_bow_transform_sorted(self._h, _ptr(d), n, levelsup, _ptr(w), _ptr(nd), _ptr(wt), _ptr(bw), _ptr(bn), ctypes.byref(filed)))
        return w[:n], nd[:n], wt[:n], bw[:filed.value], bn[:filed.value]

    def job_transform(self, extractor, levelsup=4):
        """The latency form (orbx_bow_job_begin / _end) on the features `extractor`'s last single-frame call left on the device: same five arrays."""
        L = self._L
        vp = ctypes.c_void_p
        L.orbx_bow_job_create.argtypes = [vp, ctypes.POINTER(vp)]
        L.orbx_bow_job_destroy.argtypes = [vp]
        L.orbx_bow_job_destroy.restype = None
        L.orbx_bow_job_begin.argtypes = [vp, vp, ctypes.c_int]
        L.orbx_bow_job_end.argtypes = [vp] + [ctypes.POINTER(vp)] * 5 + [ctypes.POINTER(ctypes.c_int32)] * 2
        if getattr(self, "_job", None) is None:
            self._job = vp()
            _check(L.orbx_bow_job_create(self._h, ctypes.byref(self._job)))
        _check(L.orbx_bow_job_begin(self._job, extractor._h, levelsup))
        ptrs = [vp() for _ in range(5)]
        filed, n = ctypes.c_int32(), ctypes.c_int32()
        _check(L.orbx_bow_job_end(self._job, *[ctypes.byref(q) for q in ptrs], ctypes.byref(filed), ctypes.byref(n)))
        if n.value == 0:
            return tuple(np.zeros(0, t) for t in (np.int32, np.int32, np.float64, np.int32, np.int32))
        view = lambda q, t, k: np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(t)), (k,)).copy()
        return (view(ptrs[0], ctypes.c_int32, n.value), view(ptrs[1], ctypes.c_int32, n.value), view(ptrs[2], ctypes.c_double, n.value),
                view(ptrs[3], ctypes.c_int32, filed.value), view(ptrs[4], ctypes.c_int32, filed.value))

    def transform_device(self, extractor, levelsup=4):
        _check(self._L.orbx_bow_transform_device(self._h, extractor._h, levelsup))

    def groups_device(self):
        """device pointer of the FeatureVector node ids of the last transform_device (orbx_feature_set.groups)."""
        nd, cap = ctypes.c_void_p(), ctypes.c_int()
        _check(self._L.orbx_bow_results_device(self._h, None, ctypes.byref(nd), None, ctypes.byref(cap)))
        return nd, cap.value

    def download(self, extractor, batch):
        _, cap = self.groups_device()
        w, nd, wt = np.zeros((batch, cap), np.int32), np.zeros((batch, cap), np.int32), np.zeros((batch, cap), np.float64)
        _check(self._L.orbx_bow_download(self._h, extractor._h, batch, _ptr(w), _ptr(nd), _ptr(wt)))
        return w, nd, wt


class VocTextInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("k", "L", "scoring", "weighting", "num_nodes", "num_words", "final_newline", "host_lines", "error_line", "launches", "waits")] + \
               [("bytes", ctypes.c_int64)] + [(n, ctypes.c_float) for n in ("read_ms", "upload_ms", "kernel_ms", "host_ms", "total_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _bind_voc_text(L):
    vp, ci, ip = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(VocTextInfo)
    L.orbx_vocabulary_load_text.argtypes = [ci, ctypes.c_char_p, ctypes.POINTER(vp), ip]
    L.orbx_vocabulary_load_text_buffer.argtypes = [ci, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp), ip]
    L.orbx_vocabulary_tree.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int32)] * 3 + [vp] * 4
    L.orbx_voc_text_parse_host.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ip, ctypes.c_int32, vp, vp, vp, vp]
    L.orbx_voc_text_weight_rule.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)]


def voc_text_parse_host(data):
    """orbx_voc_text_parse_host: the literal host statement of the text parse (no device) -> voc_synth's dict plus the header fields, num_words,
    final_newline and error_line.  A format error raises OrbxError with .text_info."""
    L = load_library()
    _bind_voc_text(L)
    data = bytes(data)
    info = VocTextInfo()
    rc = L.orbx_voc_text_parse_host(data, len(data), ctypes.byref(info), 0, None, None, None, None)
    if rc == ORBX_OK:
        n = info.num_nodes
        par, leaf, desc, wt = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
        rc = L.orbx_voc_text_parse_host(data, len(data), ctypes.byref(info), n, _ptr(par), _ptr(leaf), _ptr(desc), _ptr(wt))
    if rc != ORBX_OK:
        e = OrbxError(rc, L.orbx_last_error().decode("utf-8", "replace"))
        e.text_info = info.as_dict()
        raise e
    return dict(info.as_dict(), parent=par, is_leaf=leaf, desc=desc, weight=wt)


def voc_text_weight_rule(token):
    """the device's accept rule for one weight token, run on the host: the double it proves, or None where it flags the line"""
    L = load_library()
    _bind_voc_text(L)
    t, v = bytes(token), ctypes.c_double()
    return v.value if L.orbx_voc_text_weight_rule(t, len(t), ctypes.byref(v)) else None


VOC_MAX_K, VOC_MAX_L = 32, 10      # ORBX_VOC_MAX_K, ORBX_VOC_MAX_L
VOC_TF_IDF, VOC_TF, VOC_IDF, VOC_BINARY = 0, 1, 2, 3      # DBoW2::WeightingType


class VocTrainParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("weighting", ctypes.c_int), ("max_iterations", ctypes.c_int)]


class VocTrainSummary(ctypes.Structure):
    _fields_ = [("num_nodes", ctypes.c_int), ("num_words", ctypes.c_int), ("unconverged_nodes", ctypes.c_int), ("passes_per_level", ctypes.c_int * VOC_MAX_L)]


class VocabularyTrainer(_Handle):
    """TemplatedVocabulary::create(training_features, k, L, weighting, scoring) on the device (reference
    Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-996): hierarchical k-means++ over 256-bit descriptors and the IDF weights, with the three
    stated differences of include/orbx.h (counter-hash draws, an empty cluster keeps its centre, a cap on the assignment passes)."""
    _destroy = "orbx_voc_trainer_destroy"

    def __init__(self, k, L, max_descriptors, max_images, device=0):
        self._L = load_library()
        L_ = self._L
        vp, ci, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
        L_.orbx_voc_trainer_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
        L_.orbx_voc_trainer_destroy.argtypes = [vp]
        L_.orbx_voc_trainer_destroy.restype = None
        L_.orbx_voc_trainer_add.argtypes = [vp, vp, vp, ci]
        L_.orbx_voc_trainer_add_extracted.argtypes = [vp, vp]
        L_.orbx_voc_trainer_clear.argtypes = [vp]
        L_.orbx_voc_trainer_size.argtypes = [vp, vp, vp]
        L_.orbx_voc_train.argtypes = [vp, ctypes.POINTER(VocTrainParams), ctypes.POINTER(VocTrainSummary)]
        L_.orbx_voc_trainer_result.argtypes = [vp, vp, vp, vp, vp, vp, ci]
        L_.orbx_voc_trainer_vocabulary.argtypes = [vp, ctypes.POINTER(vp)]
        L_.orbx_voc_trainer_set_profiling.argtypes = [vp, ci]
        L_.orbx_voc_trainer_last_timing.argtypes = [vp, vp, vp, vp, vp]
        L_.orbx_voc_seed_segments.argtypes = [vp, vp, ci, vp, vp, ci, u64, vp]
        L_.orbx_voc_lloyd_pass.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp]
        self.k, self.L = int(k), int(L)
        self._h = vp()
        _check(L_.orbx_voc_trainer_create(device, int(k), int(L), int(max_descriptors), int(max_images), ctypes.byref(self._h)))

    def add(self, images):
        """one uint8 array (n_i, 32) per image; an image may be empty"""
        arrs = [np.ascontiguousarray(a, np.uint8).reshape(-1, 32) for a in images]
        counts = np.array([len(a) for a in arrs], np.int32)
        d = np.concatenate(arrs) if arrs else np.zeros((0, 32), np.uint8)
        _check(self._L.orbx_voc_trainer_add(self._h, _ptr(d) if len(d) else None, _ptr(counts), len(counts)))

    def add_extracted(self, extractor):
        """every frame of `extractor`'s last batch as one image, read where the extractor left it on the device"""
        _check(self._L.orbx_voc_trainer_add_extracted(self._h, extractor._h))

    def clear(self):
        _check(self._L.orbx_voc_trainer_clear(self._h))

    def size(self):
        """(descriptors, images)"""
        a, b = ctypes.c_int(), ctypes.c_int()
        _check(self._L.orbx_voc_trainer_size(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def train(self, seed=0, weighting=VOC_TF_IDF, max_iterations=100):
        """-> dict in voc_synth's format (usable as Vocabulary(voc) and by voc_synth.write_text) plus ni per node and the summary
        (num_words, unconverged_nodes, passes_per_level)."""
        p, s = VocTrainParams(int(seed) & (2 ** 64 - 1), int(weighting), int(max_iterations)), VocTrainSummary()
        _check(self._L.orbx_voc_train(self._h, ctypes.byref(p), ctypes.byref(s)))
        n = s.num_nodes
        par, leaf, desc = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
        wt, ni = np.zeros(n, np.float64), np.zeros(n, np.int32)
        _check(self._L.orbx_voc_trainer_result(self._h, _ptr(par), _ptr(leaf), _ptr(desc), _ptr(wt), _ptr(ni), n))
        return dict(k=self.k, L=self.L, parent=par, is_leaf=leaf, desc=desc, weight=wt, num_nodes=n, ni=ni, num_words=s.num_words,
                    unconverged_nodes=s.unconverged_nodes, passes_per_level=list(s.passes_per_level)[:self.L])

    def vocabulary(self):
        """the device Vocabulary of the last training"""
        v = Vocabulary.__new__(Vocabulary)
        v._L = self._L
        Vocabulary._bind(v._L)
        v._h = ctypes.c_void_p()
        _check(self._L.orbx_voc_trainer_vocabulary(self._h, ctypes.byref(v._h)))
        return v

    def set_profiling(self, enable=True):
        _check(self._L.orbx_voc_trainer_set_profiling(self._h, int(bool(enable))))

    def last_timing(self):
        """dict(total_ms, level_ms (L), stage_ms: seeding / assignment / mean / partition / other (device time, profiling only), launches)"""
        t, n = ctypes.c_float(), ctypes.c_int()
        lv, st = (ctypes.c_float * VOC_MAX_L)(), (ctypes.c_float * 5)()
        _check(self._L.orbx_voc_trainer_last_timing(self._h, ctypes.byref(t), lv, st, ctypes.byref(n)))
        return dict(total_ms=t.value, level_ms=list(lv)[:self.L], stage_ms=dict(zip(("seeding", "assignment", "mean", "partition", "other"), list(st))), launches=n.value)

    def seed_segments(self, descriptors, offsets, slots, seed=0):
        """orbx_voc_seed_segments -> chosen (S, k): index inside segment s of its j-th centre, -1 where the seeding ended early"""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        off, sl = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(slots, np.uint64)
        out = np.zeros((len(sl), self.k), np.int32)
        _check(self._L.orbx_voc_seed_segments(self._h, _ptr(d), len(d), _ptr(off), _ptr(sl), len(sl), int(seed) & (2 ** 64 - 1), _ptr(out)))
        return out

    def lloyd_pass(self, descriptors, offsets, centres, num_centres, prev=None):
        """orbx_voc_lloyd_pass -> (centres (S, k, 32), association (n), changed (S))"""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        off, nc = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(num_centres, np.int32)
        c = np.ascontiguousarray(centres, np.uint8).reshape(len(nc), self.k, 32)
        pv = None if prev is None else np.ascontiguousarray(prev, np.int32)
        co, ao, ch = np.zeros_like(c), np.zeros(len(d), np.int32), np.zeros(len(nc), np.uint8)
        _check(self._L.orbx_voc_lloyd_pass(self._h, _ptr(d), len(d), _ptr(off), len(nc), _ptr(c), _ptr(nc), None if pv is None else _ptr(pv), _ptr(co), _ptr(ao), _ptr(ch)))
        return co, ao, ch


class Camera(ctypes.Structure):
    """orbx_camera: mK and mDistCoef (k1 k2 p1 p2 [k3])."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("dist", ctypes.c_float * 5), ("ndist", ctypes.c_int)]


FRAME_GRID_COLS, FRAME_GRID_ROWS = 64, 48


class FrameGrid(ctypes.Structure):
    """orbx_frame_grid: Frame::mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv."""
    _fields_ = [("min_x", ctypes.c_float), ("min_y", ctypes.c_float), ("width_inv", ctypes.c_float), ("height_inv", ctypes.c_float)]

    @classmethod
    def from_bounds(cls, bounds):
        """the grid constants as the Frame constructor derives them from the image bounds (src/Frame.cc:326-327)"""
        b = np.asarray(bounds, np.float32)
        return cls(float(b[0]), float(b[2]), float(np.float32(FRAME_GRID_COLS) / np.float32(b[1] - b[0])),
                   float(np.float32(FRAME_GRID_ROWS) / np.float32(b[3] - b[2])))


DEPTH_F32, DEPTH_U16 = 0, 1


class DepthDesc(ctypes.Structure):
    """orbx_depth_desc: a depth image (latency form, host) or B of them (batch form, device)."""
    _fields_ = [("data", ctypes.c_void_p), ("format", ctypes.c_int), ("cols", ctypes.c_int), ("rows", ctypes.c_int),
                ("stride_bytes", ctypes.c_int), ("factor", ctypes.c_float)]

    @classmethod
    def of(cls, image, factor=1.0):
        """descriptor of a host image (float32 or uint16, rows may be strided); the caller keeps `image` alive"""
        assert image.ndim == 2 and image.strides[1] == image.itemsize and image.dtype in (np.float32, np.uint16)
        return cls(image.ctypes.data, DEPTH_F32 if image.dtype == np.float32 else DEPTH_U16, image.shape[1], image.shape[0], image.strides[0], factor)


class RgbdParams(ctypes.Structure):
    """orbx_rgbd_params: mbf, mThDepth."""
    _fields_ = [("bf", ctypes.c_float), ("th_depth", ctypes.c_float)]


class RgbdFrame(ctypes.Structure):
    """orbx_rgbd_frame: what orbx_frame_rgbd_end hands out."""
    _fields_ = [("depth", ctypes.c_void_p), ("u_right", ctypes.c_void_p), ("order", ctypes.c_void_p), ("xyz_cam", ctypes.c_void_p),
                ("n_valid", ctypes.c_int), ("n_close", ctypes.c_int)]


class FrameOps(_Handle):
    """Frame::UndistortKeyPoints, ComputeImageBounds and AssignFeaturesToGrid on the device
    (reference src/Frame.cc:899-1004, 460-491) for one camera (mK, mDistCoef)."""
    _destroy = "orbx_frame_ops_destroy"

    def __init__(self, fx, fy, cx, cy, dist, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_frame_ops_create.argtypes = [ci, vp, ctypes.POINTER(vp)]
        L.orbx_frame_ops_destroy.argtypes = [vp]
        L.orbx_frame_ops_destroy.restype = None
        L.orbx_frame_image_bounds.argtypes = [vp, ci, ci, vp]
        L.orbx_frame_undistort.argtypes = [vp, vp, ci, vp]
        L.orbx_frame_assign_grid.argtypes = [vp, vp, vp, ci, vp, vp]
        L.orbx_frame_finish_device.argtypes = [vp, vp, vp]
        L.orbx_frame_results_device.argtypes = [vp, vp, vp, vp, vp]
        L.orbx_frame_download.argtypes = [vp, vp, ci, vp, vp, vp]
        L.orbx_upload_depth.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.c_float, vp]
        L.orbx_frame_rgbd_device.argtypes = [vp, vp, vp, vp, vp]
        L.orbx_frame_rgbd_results_device.argtypes = [vp] * 7 + [vp]
        L.orbx_frame_rgbd_download.argtypes = [vp, vp, ci] + [vp] * 6
        L.orbx_frame_rgbd_begin.argtypes = [vp, vp, vp, vp, vp]
        L.orbx_frame_rgbd_end.argtypes = [vp, vp, vp, vp, vp, vp]
        cam = Camera(fx, fy, cx, cy)
        dist = [float(d) for d in dist]
        for i, d in enumerate(dist[:5]):
            cam.dist[i] = d
        cam.ndist = len(dist)
        self._h = vp()
        _check(L.orbx_frame_ops_create(device, ctypes.byref(cam), ctypes.byref(self._h)))

    def ComputeImageBounds(self, cols, rows):
        """mnMinX, mnMaxX, mnMinY, mnMaxY."""
        b = np.zeros(4, np.float32)
        _check(self._L.orbx_frame_image_bounds(self._h, cols, rows, _ptr(b)))
        return b

    def UndistortKeyPoints(self, keypoints):
        kp = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
        un = np.zeros(max(len(kp), 1), KEYPOINT_DTYPE)
        _check(self._L.orbx_frame_undistort(self._h, _ptr(kp), len(kp), _ptr(un)))
        return un[:len(kp)]

    def AssignFeaturesToGrid(self, keypoints_un, grid):
        """mGrid as CSR: offsets[64*48+1] over cell = x*48 + y, indices in push_back order."""
        kp = np.ascontiguousarray(keypoints_un, dtype=KEYPOINT_DTYPE)
        off = np.zeros(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1, np.int32)
        idx = np.zeros(max(len(kp), 1), np.int32)
        _check(self._L.orbx_frame_assign_grid(self._h, ctypes.byref(grid), _ptr(kp), len(kp), _ptr(off), _ptr(idx)))
        return off, idx[:off[-1]]

    def finish_device(self, extractor, grid):
        """both, fused, on the extractor's last batch (device resident)"""
        _check(self._L.orbx_frame_finish_device(self._h, extractor._h, ctypes.byref(grid)))

    def finish_frame(self, extractor, grid=None):
        """Latency form for ONE frame that `extractor`'s last single-frame call extracted (orbx_frame_finish_begin + _end): the kernel reads
        the keypoints on the device and writes into pinned memory.  -> (mvKeysUn or None when the camera is not distorted, offsets, indices, n);
        offsets / indices are None without a grid."""
        L = self._L
        vp = ctypes.c_void_p
        L.orbx_frame_finish_begin.argtypes = [vp, vp, vp]
        L.orbx_frame_finish_end.argtypes = [vp, vp, vp, vp, vp]
        _check(L.orbx_frame_finish_begin(self._h, extractor._h, ctypes.byref(grid) if grid is not None else None))
        un, off, idx, n = vp(), vp(), vp(), ctypes.c_int()
        _check(L.orbx_frame_finish_end(self._h, ctypes.byref(un), ctypes.byref(off), ctypes.byref(idx), ctypes.byref(n)))
        n = n.value
        kun = np.ctypeslib.as_array(ctypes.cast(un, ctypes.POINTER(ctypes.c_uint8)), shape=(max(n, 1) * KEYPOINT_DTYPE.itemsize,)).view(KEYPOINT_DTYPE)[:n].copy() if un.value else None
        o = np.ctypeslib.as_array(ctypes.cast(off, ctypes.POINTER(ctypes.c_int32)), shape=(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1,)).copy() if off.value else None
        i = np.ctypeslib.as_array(ctypes.cast(idx, ctypes.POINTER(ctypes.c_int32)), shape=(max(n, 1),))[:int(o[-1])].copy() if (idx.value and o is not None) else None
        return kun, o, i, n

    # --- the RGB-D constructor: frame finish + Frame::ComputeStereoFromRGBD (src/Frame.cc:1423-1461) in one launch ---
    def upload_depth(self, images, factor=1.0):
        """B host depth images (float32 or uint16, same shape) -> DepthDesc of their device copy (orbx_upload_depth)"""
        B = len(images)
        d0 = DepthDesc.of(images[0], factor)
        arr = (ctypes.c_void_p * B)(*[im.ctypes.data for im in images])
        assert all(im.shape == images[0].shape and im.dtype == images[0].dtype and im.strides == images[0].strides for im in images)
        out = DepthDesc()
        _check(self._L.orbx_upload_depth(self._h, arr, B, d0.format, d0.cols, d0.rows, d0.stride_bytes, factor, ctypes.byref(out)))
        return out

    def rgbd_device(self, extractor, grid, depth_dev, bf, th_depth):
        """finish_device + the RGB-D step on the extractor's last batch (device resident)"""
        prm = RgbdParams(bf, th_depth)
        _check(self._L.orbx_frame_rgbd_device(self._h, extractor._h, ctypes.byref(grid), ctypes.byref(depth_dev), ctypes.byref(prm)))

    def rgbd_download(self, extractor, batch):
        """-> dict(depth, u_right, order [B, cap], n_valid, n_close [B], xyz_cam [B, cap, 3]); entries behind a frame's keypoint count are undefined"""
        cap = ctypes.c_int()
        _check(self._L.orbx_frame_rgbd_results_device(self._h, None, None, None, None, None, None, ctypes.byref(cap)))
        cap = cap.value
        r = dict(depth=np.zeros((batch, cap), np.float32), u_right=np.zeros((batch, cap), np.float32), order=np.zeros((batch, cap), np.int32),
                 n_valid=np.zeros(batch, np.int32), n_close=np.zeros(batch, np.int32), xyz_cam=np.zeros((batch, cap, 3), np.float32))
        _check(self._L.orbx_frame_rgbd_download(self._h, extractor._h, batch, _ptr(r["depth"]), _ptr(r["u_right"]), _ptr(r["order"]), _ptr(r["n_valid"]),
                                                _ptr(r["n_close"]), _ptr(r["xyz_cam"])))
        return r

    def rgbd_frame(self, extractor, grid, depth, bf, th_depth, factor=1.0):
        """Latency form for ONE frame (orbx_frame_rgbd_begin + _end) with the host image `depth` (float32, or uint16 with `factor`).
        -> (mvKeysUn or None, offsets, indices, n, dict(depth, u_right, order, xyz_cam, n_valid, n_close)); copies of the pinned views."""
        L = self._L
        vp = ctypes.c_void_p
        dd, prm = DepthDesc.of(depth, factor), RgbdParams(bf, th_depth)
        _check(L.orbx_frame_rgbd_begin(self._h, extractor._h, ctypes.byref(grid) if grid is not None else None, ctypes.byref(dd), ctypes.byref(prm)))
        un, off, idx, n, rf = vp(), vp(), vp(), ctypes.c_int(), RgbdFrame()
        _check(L.orbx_frame_rgbd_end(self._h, ctypes.byref(un), ctypes.byref(off), ctypes.byref(idx), ctypes.byref(n), ctypes.byref(rf)))
        n = n.value
        kun = np.ctypeslib.as_array(ctypes.cast(un, ctypes.POINTER(ctypes.c_uint8)), shape=(max(n, 1) * KEYPOINT_DTYPE.itemsize,)).view(KEYPOINT_DTYPE)[:n].copy() if un.value else None
        o = np.ctypeslib.as_array(ctypes.cast(off, ctypes.POINTER(ctypes.c_int32)), shape=(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1,)).copy() if off.value else None
        i = np.ctypeslib.as_array(ctypes.cast(idx, ctypes.POINTER(ctypes.c_int32)), shape=(max(n, 1),))[:int(o[-1])].copy() if (idx.value and o is not None) else None

        def view(p, ct, dt, m):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(max(m, 1),))[:m].astype(dt, copy=True)
        r = dict(depth=view(rf.depth, ctypes.c_float, np.float32, n), u_right=view(rf.u_right, ctypes.c_float, np.float32, n),
                 order=view(rf.order, ctypes.c_int32, np.int32, n), xyz_cam=view(rf.xyz_cam, ctypes.c_float, np.float32, 3 * n).reshape(n, 3),
                 n_valid=rf.n_valid, n_close=rf.n_close)
        return kun, o, i, n, r

    def keypoints_un_device(self):
        kp, cap = ctypes.c_void_p(), ctypes.c_int()
        _check(self._L.orbx_frame_results_device(self._h, ctypes.byref(kp), None, None, ctypes.byref(cap)))
        return kp, cap.value

    def download(self, extractor, batch):
        _, cap = self.keypoints_un_device()
        un = np.zeros((batch, cap), KEYPOINT_DTYPE)
        off = np.zeros((batch, FRAME_GRID_COLS * FRAME_GRID_ROWS + 1), np.int32)
        idx = np.zeros((batch, cap), np.int32)
        _check(self._L.orbx_frame_download(self._h, extractor._h, batch, _ptr(un), _ptr(off), _ptr(idx)))
        return un, off, idx


class LbaProblem(ctypes.Structure):
    _fields_ = [("num_keyframes", ctypes.c_int), ("poses", ctypes.c_void_p), ("fixed", ctypes.c_void_p), ("intrinsics", ctypes.c_void_p),
                ("num_points", ctypes.c_int), ("points", ctypes.c_void_p), ("num_edges", ctypes.c_int), ("edge_point", ctypes.c_void_p),
                ("edge_keyframe", ctypes.c_void_p), ("edge_obs", ctypes.c_void_p), ("edge_inv_sigma2", ctypes.c_void_p)]


class LbaResult(ctypes.Structure):
    _fields_ = [("poses", ctypes.c_void_p), ("points", ctypes.c_void_p), ("edge_chi2", ctypes.c_void_p), ("edge_outlier", ctypes.c_void_p),
                ("stats", ctypes.c_double * 8)]


def _load_lba_synth():
    spec = importlib.util.spec_from_file_location("orbx_lba_synth", _PKG / "lba_synth.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lba_synth = _load_lba_synth()


def _load_sibling(name):
    spec = importlib.util.spec_from_file_location("orbx_" + name, _PKG / (name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


distributed = _load_sibling("distributed")
voc_synth = _load_sibling("voc_synth")


class PoseProblem(ctypes.Structure):
    _fields_ = [("num_frames", ctypes.c_int), ("capacity", ctypes.c_int), ("poses", ctypes.c_void_p), ("cameras", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("world_points", ctypes.c_void_p), ("observations", ctypes.c_void_p), ("inv_sigma2", ctypes.c_void_p)]


class PoseOptimizer(_Handle):
    """Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:363-605) for a batch of independent frames."""
    _destroy = "orbx_pose_optimizer_destroy"

    def __init__(self, max_frames=64, max_features=4096, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_pose_optimizer_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_pose_optimizer_destroy.argtypes = [vp]
        L.orbx_pose_optimizer_destroy.restype = None
        L.orbx_pose_optimization.argtypes = [vp, ctypes.POINTER(PoseProblem), vp, vp, vp, vp]
        self._h = vp()
        _check(L.orbx_pose_optimizer_create(device, max_frames, max_features, ctypes.byref(self._h)))

    def PoseOptimization(self, frames):
        """frames: list of dict(pose (4x4), cam (fx,fy,cx,cy,bf), Xw (n,3), obs (n,3; uR<0 mono), inv_sigma2 (n)).
        Returns list of dict(pose, outlier, inliers, stats)."""
        B = len(frames)
        cap = max(1, max(len(f["Xw"]) for f in frames))
        poses = np.zeros((B, 16), np.float32)
        cams = np.zeros((B, 5), np.float32)
        counts = np.zeros(B, np.int32)
        Xw, obs, inv = np.zeros((B, cap, 3), np.float32), np.zeros((B, cap, 3), np.float32), np.zeros((B, cap), np.float32)
        for i, f in enumerate(frames):
            n = len(f["Xw"])
            poses[i] = np.asarray(f["pose"], np.float32).reshape(16)
            cams[i] = np.asarray(f["cam"], np.float32)
            counts[i] = n
            Xw[i, :n], obs[i, :n], inv[i, :n] = f["Xw"], f["obs"], f["inv_sigma2"]
        P = PoseProblem(B, cap, _ptr(poses).value, _ptr(cams).value, _ptr(counts).value, _ptr(Xw).value, _ptr(obs).value, _ptr(inv).value)
        po, outl, inl, st = np.zeros((B, 16), np.float32), np.zeros((B, cap), np.uint8), np.zeros(B, np.int32), np.zeros((B, 8), np.float64)
        _check(self._L.orbx_pose_optimization(self._h, ctypes.byref(P), _ptr(po), _ptr(outl), _ptr(inl), _ptr(st)))
        return [dict(pose=po[i].reshape(4, 4), outlier=outl[i, :counts[i]], inliers=int(inl[i]), stats=st[i]) for i in range(B)]


class Optimizer(_Handle):
    """Mirror of the static ORB_SLAM2::Optimizer::LocalBundleAdjustment (reference include/Optimizer.h:112)
    on a flat window (dict as produced by lba_synth.make_window)."""
    _destroy = "orbx_lba_destroy"
    _keeps_pointer = True

    def __init__(self, max_keyframes=256, max_points=20000, max_edges=400000, device=0):
        self._L = load_library()
        vp, ci = ctypes.c_void_p, ctypes.c_int
        self._L.orbx_lba_create.argtypes = [ci, ci, ci, ci, ctypes.POINTER(vp)]
        self._L.orbx_lba_destroy.argtypes = [vp]
        self._L.orbx_lba_destroy.restype = None
        self._L.orbx_lba_solve.argtypes = [vp, ctypes.POINTER(LbaProblem), vp, ctypes.POINTER(LbaResult)]
        self._L.orbx_lba_last_timing.argtypes = [vp, vp, vp]
        self._h = vp()
        _check(self._L.orbx_lba_create(device, max_keyframes, max_points, max_edges, ctypes.byref(self._h)))

    def LocalBundleAdjustment(self, w, stop_flag=None, iterations=None, robust=True):
        K, P, E = w["K"], w["P"], w["E"]
        arrs = {k: np.ascontiguousarray(w[k]) for k in ("poses", "fixed", "intr", "points", "edge_point", "edge_kf", "edge_obs", "edge_inv_sigma2")}
        prob = LbaProblem(K, arrs["poses"].ctypes.data, arrs["fixed"].ctypes.data, arrs["intr"].ctypes.data, P, arrs["points"].ctypes.data, E,
                          arrs["edge_point"].ctypes.data, arrs["edge_kf"].ctypes.data, arrs["edge_obs"].ctypes.data, arrs["edge_inv_sigma2"].ctypes.data)
        poses = np.zeros((K, 16), np.float32)
        points = np.zeros((P, 3), np.float32)
        chi2 = np.zeros(E, np.float64)
        outl = np.zeros(E, np.uint8)
        res = LbaResult(poses.ctypes.data, points.ctypes.data, chi2.ctypes.data, outl.ctypes.data)
        stop = None if stop_flag is None else stop_flag.ctypes.data_as(ctypes.c_void_p)
        if iterations is None:
            _check(self._L.orbx_lba_solve(self._h, ctypes.byref(prob), stop, ctypes.byref(res)))
        else:
            self._L.orbx_bundle_adjustment.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
            _check(self._L.orbx_bundle_adjustment(self._h, ctypes.byref(prob), int(iterations), 1 if robust else 0, stop, ctypes.byref(res)))
        return dict(poses=poses, points=points, chi2=chi2, outlier=outl, stats=np.array(list(res.stats)))

    def BundleAdjustment(self, w, iterations=5, robust=True, stop_flag=None):
        """Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (reference src/Optimizer.cc:55-360) on the same flat problem layout."""
        return self.LocalBundleAdjustment(w, stop_flag, iterations=iterations, robust=robust)

    def last_timing(self):
        return self._timing("orbx_lba_last_timing", ctypes.c_float, ctypes.c_double)


class BatchOptimizer(_Handle):
    """Optimizer::LocalBundleAdjustment on many independent windows with ONE handle (orbx_lba_solve_batch): every kernel launch
    covers all windows of a call, and every window's result is bit-identical to Optimizer().LocalBundleAdjustment(w).
    Capacities are per window; max_keyframes <= 341."""
    _destroy = "orbx_lba_batch_destroy"
    _keeps_pointer = True

    def __init__(self, max_windows, max_keyframes, max_points, max_edges, device=0):
        self._L = load_library()
        vp, ci = ctypes.c_void_p, ctypes.c_int
        self._L.orbx_lba_batch_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
        self._L.orbx_lba_batch_destroy.argtypes = [vp]
        self._L.orbx_lba_batch_destroy.restype = None
        self._L.orbx_lba_solve_batch.argtypes = [vp, ci, ctypes.POINTER(LbaProblem), vp, ctypes.POINTER(LbaResult)]
        self._L.orbx_lba_batch_last_timing.argtypes = [vp, vp, vp]
        self._h = vp()
        _check(self._L.orbx_lba_batch_create(device, max_windows, max_keyframes, max_points, max_edges, ctypes.byref(self._h)))

    def LocalBundleAdjustment(self, windows, stop_flags=None):
        """windows: list of dicts as produced by lba_synth.make_window; stop_flags: None, or one uint8 array (or None) per window.
        Returns one dict per window, in the form of Optimizer.LocalBundleAdjustment."""
        n = len(windows)
        keep, outs = [], []
        probs = (LbaProblem * max(n, 1))()
        results = (LbaResult * max(n, 1))()
        for i, w in enumerate(windows):
            arrs = {k: np.ascontiguousarray(w[k]) for k in ("poses", "fixed", "intr", "points", "edge_point", "edge_kf", "edge_obs", "edge_inv_sigma2")}
            keep.append(arrs)
            probs[i] = LbaProblem(w["K"], arrs["poses"].ctypes.data, arrs["fixed"].ctypes.data, arrs["intr"].ctypes.data, w["P"], arrs["points"].ctypes.data, w["E"],
                                  arrs["edge_point"].ctypes.data, arrs["edge_kf"].ctypes.data, arrs["edge_obs"].ctypes.data, arrs["edge_inv_sigma2"].ctypes.data)
            o = dict(poses=np.zeros((w["K"], 16), np.float32), points=np.zeros((w["P"], 3), np.float32), chi2=np.zeros(w["E"], np.float64),
                     outlier=np.zeros(w["E"], np.uint8))
            outs.append(o)
            results[i] = LbaResult(o["poses"].ctypes.data, o["points"].ctypes.data, o["chi2"].ctypes.data, o["outlier"].ctypes.data)
        stops = None
        if stop_flags is not None:
            if len(stop_flags) != n:
                raise ValueError("stop_flags: one entry per window")
            stops = (ctypes.c_void_p * max(n, 1))(*[None if f is None else f.ctypes.data for f in stop_flags])
        _check(self._L.orbx_lba_solve_batch(self._h, n, probs, stops, results))
        for i, o in enumerate(outs):
            o["stats"] = np.array(list(results[i].stats))
        return outs

    def last_timing(self):
        return self._timing("orbx_lba_batch_last_timing", ctypes.c_float, ctypes.c_double)


class MapPointBatch(ctypes.Structure):
    _fields_ = [("num_points", ctypes.c_int), ("num_obs", ctypes.c_int), ("obs_offset", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("desc_valid", ctypes.c_void_p),
                ("cam_center", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("ref_center", ctypes.c_void_p), ("ref_scale", ctypes.c_void_p), ("top_scale", ctypes.c_void_p)]


class MapPointResult(ctypes.Structure):
    _fields_ = [("best_obs", ctypes.c_void_p), ("best_median", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("max_dist", ctypes.c_void_p), ("min_dist", ctypes.c_void_p),
                ("updated", ctypes.c_void_p)]


class MapPointOps(_Handle):
    """MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:359-439, 477-521) for a batch of
    points with ragged observation lists (orbx_mappoint_refresh): one launch chain, the observations of a point in the caller's order."""
    _destroy = "orbx_mappoint_ops_destroy"

    def __init__(self, max_points, max_obs_total, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_mappoint_ops_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_mappoint_ops_destroy.argtypes = [vp]
        L.orbx_mappoint_ops_destroy.restype = None
        L.orbx_mappoint_refresh.argtypes = [vp, ctypes.POINTER(MapPointBatch), ctypes.POINTER(MapPointResult)]
        L.orbx_mappoint_last_timing.argtypes = [vp, vp, vp]
        self._h = vp()
        _check(L.orbx_mappoint_ops_create(device, max_points, max_obs_total, ctypes.byref(self._h)))

    def refresh(self, obs_offset, desc, cam_center, pos, ref_center, ref_scale, top_scale, desc_valid=None):
        """obs_offset (M+1) int32; desc (T,32) uint8; cam_center (T,3); pos, ref_center (M,3); ref_scale, top_scale (M); desc_valid (T) uint8 or
        None (all valid).  Returns dict(best_obs, best_median (M) int32; normal (M,3), max_dist, min_dist (M) float32; updated (M) uint8)."""
        off = np.ascontiguousarray(obs_offset, np.int32)
        M = len(off) - 1
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        T = len(d)
        cam = np.ascontiguousarray(cam_center, np.float32).reshape(-1, 3)
        ps, rc = np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(ref_center, np.float32).reshape(-1, 3)
        rs, ts = np.ascontiguousarray(ref_scale, np.float32).reshape(-1), np.ascontiguousarray(top_scale, np.float32).reshape(-1)
        dv = None if desc_valid is None else np.ascontiguousarray(desc_valid, np.uint8).reshape(-1)
        if M < 0 or len(cam) != T or (dv is not None and len(dv) != T) or any(len(a) != M for a in (ps, rc, rs, ts)):
            raise ValueError("MapPointOps.refresh: array sizes do not agree")
        B = MapPointBatch(M, T, off.ctypes.data, d.ctypes.data, None if dv is None else dv.ctypes.data, cam.ctypes.data, ps.ctypes.data, rc.ctypes.data,
                          rs.ctypes.data, ts.ctypes.data)
        o = dict(best_obs=np.zeros(M, np.int32), best_median=np.zeros(M, np.int32), normal=np.zeros((M, 3), np.float32), max_dist=np.zeros(M, np.float32),
                 min_dist=np.zeros(M, np.float32), updated=np.zeros(M, np.uint8))
        R = MapPointResult(*[o[k].ctypes.data for k in ("best_obs", "best_median", "normal", "max_dist", "min_dist", "updated")])
        _check(self._L.orbx_mappoint_refresh(self._h, ctypes.byref(B), ctypes.byref(R)))
        return o

    def last_timing(self):
        """(device ms of the last call's kernels, kernel launches)"""
        return self._timing("orbx_mappoint_last_timing", ctypes.c_float, ctypes.c_int)


class InitMatches(ctypes.Structure):
    _fields_ = [("keys1_xy", ctypes.c_void_p), ("keys2_xy", ctypes.c_void_p), ("n1", ctypes.c_int), ("n2", ctypes.c_int), ("matches12", ctypes.c_void_p)]


class InitProblem(ctypes.Structure):
    _fields_ = [("keys1_xy", ctypes.c_void_p), ("keys2_xy", ctypes.c_void_p), ("n1", ctypes.c_int), ("n2", ctypes.c_int), ("matches12", ctypes.c_void_p),
                ("sets", ctypes.c_void_p), ("iterations", ctypes.c_int), ("sigma", ctypes.c_float), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("min_parallax", ctypes.c_float), ("min_triangulated", ctypes.c_int)]


_INIT_RESULT_FIELDS = ("success", "model", "hyp", "r21", "t21", "p3d", "triangulated", "n_matches", "t1", "t2", "hn", "fpre", "fn", "h21", "h12", "f21", "score_h", "score_f",
                       "best_h", "best_f", "sh", "sf", "rh", "inliers_h", "inliers_f", "hyp_r", "hyp_t", "hyp_valid", "hyp_good", "hyp_cos_parallax", "hyp_parallax_deg",
                       "hyp_status", "hyp_p3d", "hyp_cos")


class InitResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _INIT_RESULT_FIELDS]


INIT_STATUS_NAMES = ("NOT_INLIER", "NONFINITE", "BEHIND1", "BEHIND2", "REPROJ1", "REPROJ2", "GOOD", "GOOD_LOW_PARALLAX")      # ORBX_INIT_*


def initializer_sets(n, iterations, randint):
    """mvSets of Initializer::Initialize (reference src/Initializer.cc:139-168): `iterations` sets of 8 distinct indices into n matches, each drawn
    as randint(0, len(available) - 1) (both bounds inclusive, like DUtils::Random::RandomInt) from the list of indices still available; the drawn
    slot is overwritten with the list's back and the back is popped.  -> (iterations, 8) int32"""
    if n < 8:
        raise ValueError("initializer_sets: %d matches, a set needs 8" % n)
    out = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            r = int(randint(0, len(avail) - 1))
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


class Initializer(_Handle):
    """Initializer (reference include/Initializer.h, src/Initializer.cc) on the device: Initialize as one launch chain (orbx_initialize), and its
    two inner loops on explicit inputs (ScoreModels = CheckHomography / CheckFundamental, CheckRT)."""
    _destroy = "orbx_initializer_destroy"

    def __init__(self, sigma=1.0, iterations=200, max_matches=4096, device=0):
        self._L = load_library()
        L = self._L
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.orbx_initializer_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_initializer_destroy.argtypes = [vp]
        L.orbx_initializer_destroy.restype = None
        L.orbx_initialize.argtypes = [vp, ctypes.POINTER(InitProblem), ctypes.POINTER(InitResult)]
        L.orbx_init_score_models.argtypes = [vp, ctypes.POINTER(InitMatches), vp, ci, ci, cf, vp, vp]
        L.orbx_init_check_rt.argtypes = [vp, ctypes.POINTER(InitMatches), vp, vp, vp, ci, cf, cf, cf, cf, cf, vp, vp, vp, vp, vp]
        L.orbx_initializer_last_timing.argtypes = [vp, vp, vp]
        self.sigma, self.iterations, self.max_matches = float(sigma), int(iterations), int(max_matches)
        self._h = vp()
        _check(L.orbx_initializer_create(device, self.max_matches, self.iterations, ctypes.byref(self._h)))

    @staticmethod
    def _matches(keys1, keys2, matches12):
        k1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        if len(m) != len(k1):
            raise ValueError("Initializer: matches12 holds %d entries for %d keypoints of frame 1" % (len(m), len(k1)))
        return k1, k2, m, InitMatches(k1.ctypes.data, k2.ctypes.data, len(k1), len(k2), m.ctypes.data)

    def Initialize(self, keys1, keys2, matches12, K, sets=None, rng=None, full=False, min_parallax=1.0, min_triangulated=50):
        """keys1 (n1,2), keys2 (n2,2): mvKeysUn[i].pt of the reference / current frame; matches12 (n1): index into frame 2 or -1; K = (fx, fy, cx, cy);
        sets (iterations,8) int32 or None = drawn by initializer_sets from rng (numpy Generator; default seed 0).
        -> dict(success, model (0 = H, 1 = F), hyp, r21 (3,3), t21 (3), p3d (n1,3), triangulated (n1) bool); full=True adds every diagnostic of
        orbx_init_result."""
        k1, k2, m, _ = self._matches(keys1, keys2, matches12)
        n1, N = len(k1), int((m >= 0).sum())
        if sets is None:
            g = np.random.default_rng(0) if rng is None else rng
            sets = initializer_sets(N, self.iterations, lambda lo, hi: g.integers(lo, hi + 1))
        s = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
        it = len(s)
        fx, fy, cx, cy = [float(v) for v in K]
        P = InitProblem(k1.ctypes.data, k2.ctypes.data, n1, len(k2), m.ctypes.data, s.ctypes.data, it, self.sigma, fx, fy, cx, cy, float(min_parallax), int(min_triangulated))
        f4, i4, u1 = np.float32, np.int32, np.uint8
        o = dict(success=np.zeros(1, i4), model=np.zeros(1, i4), hyp=np.zeros(1, i4), r21=np.zeros((3, 3), f4), t21=np.zeros(3, f4), p3d=np.zeros((n1, 3), f4),
                 triangulated=np.zeros(n1, u1))
        if full:
            Nn, itn = max(N, 1), max(it, 1)
            o.update(n_matches=np.zeros(1, i4), t1=np.zeros((3, 3), f4), t2=np.zeros((3, 3), f4), hn=np.zeros((itn, 3, 3), f4), fpre=np.zeros((itn, 3, 3), f4),
                     fn=np.zeros((itn, 3, 3), f4), h21=np.zeros((itn, 3, 3), f4), h12=np.zeros((itn, 3, 3), f4), f21=np.zeros((itn, 3, 3), f4), score_h=np.zeros(itn, f4),
                     score_f=np.zeros(itn, f4), best_h=np.zeros(1, i4), best_f=np.zeros(1, i4), sh=np.zeros(1, f4), sf=np.zeros(1, f4), rh=np.zeros(1, f4),
                     inliers_h=np.zeros(Nn, u1), inliers_f=np.zeros(Nn, u1), hyp_r=np.zeros((12, 3, 3), f4), hyp_t=np.zeros((12, 3), f4), hyp_valid=np.zeros(12, u1),
                     hyp_good=np.zeros(12, i4), hyp_cos_parallax=np.zeros(12, f4), hyp_parallax_deg=np.zeros(12, f4), hyp_status=np.zeros((12, Nn), u1),
                     hyp_p3d=np.zeros((12, Nn, 3), f4), hyp_cos=np.zeros((12, Nn), f4))
        R = InitResult(*[o[k].ctypes.data if k in o else None for k in _INIT_RESULT_FIELDS])
        _check(self._L.orbx_initialize(self._h, ctypes.byref(P), ctypes.byref(R)))
        out = {k: (v.reshape(-1)[0].item() if k in ("success", "model", "hyp", "n_matches", "best_h", "best_f") else v) for k, v in o.items()}
        for k in ("sh", "sf", "rh"):
            if k in out:
                out[k] = out[k][0]
        out["success"] = bool(out["success"])
        out["triangulated"] = out["triangulated"].astype(bool)
        for k in ("inliers_h", "inliers_f"):
            if k in out:
                out[k] = out[k][:N].astype(bool)
        if full:
            out["hyp_status"], out["hyp_p3d"], out["hyp_cos"] = out["hyp_status"][:, :N], out["hyp_p3d"][:, :N], out["hyp_cos"][:, :N]
        out["sets"] = s
        return out

    def ScoreModels(self, keys1, keys2, matches12, models, kind, sigma=None):
        """CheckHomography (kind 0 / "H") or CheckFundamental (kind 1 / "F") of models (M,3,3) -> (scores (M) float32, inliers (M,N) bool)"""
        k1, k2, m, Mt = self._matches(keys1, keys2, matches12)
        mod = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
        kind = {"H": 0, "F": 1}.get(kind, kind)
        N, M = int((m >= 0).sum()), len(mod)
        scores, inl = np.zeros(max(M, 1), np.float32), np.zeros((max(M, 1), max(N, 1)), np.uint8)
        _check(self._L.orbx_init_score_models(self._h, ctypes.byref(Mt), mod.ctypes.data, M, int(kind), self.sigma if sigma is None else float(sigma), scores.ctypes.data,
                                              inl.ctypes.data))
        return scores[:M], inl.reshape(-1)[:M * N].reshape(M, N).astype(bool)

    def CheckRT(self, keys1, keys2, matches12, inliers, R, t, K, th2=None):
        """CheckRT of the motions R (M,3,3), t (M,3), M <= 12, over the matches whose `inliers` (N) entry is set; th2 defaults to 4 sigma^2.
        -> dict(good (M) int32, vb_good (M,n1) bool, p3d (M,n1,3), cos_parallax (M), parallax_deg (M), status (M,N) uint8)"""
        k1, k2, m, Mt = self._matches(keys1, keys2, matches12)
        Rm, tm = np.ascontiguousarray(R, np.float32).reshape(-1, 9), np.ascontiguousarray(t, np.float32).reshape(-1, 3)
        N, M, n1 = int((m >= 0).sum()), len(Rm), len(k1)
        inl = np.ascontiguousarray(np.asarray(inliers).astype(np.uint8)).reshape(-1)
        if len(inl) != N or len(tm) != M:
            raise ValueError("Initializer.CheckRT: array sizes do not agree")
        fx, fy, cx, cy = [float(v) for v in K]
        if th2 is None:
            th2 = np.float32(4.0 * np.float64(np.float32(self.sigma) * np.float32(self.sigma)))
        o = dict(good=np.zeros(max(M, 1), np.int32), vb_good=np.zeros((max(M, 1), n1), np.uint8), p3d=np.zeros((max(M, 1), n1, 3), np.float32),
                 cos_parallax=np.zeros(max(M, 1), np.float32), status=np.zeros(max(M, 1) * max(N, 1), np.uint8))
        _check(self._L.orbx_init_check_rt(self._h, ctypes.byref(Mt), inl.ctypes.data, Rm.ctypes.data, tm.ctypes.data, M, fx, fy, cx, cy, float(th2), o["good"].ctypes.data,
                                          o["vb_good"].ctypes.data, o["p3d"].ctypes.data, o["cos_parallax"].ctypes.data, o["status"].ctypes.data))
        o["status"] = o["status"][:M * N].reshape(M, N)
        o["vb_good"] = o["vb_good"].astype(bool)
        c = o["cos_parallax"]
        o["parallax_deg"] = ((np.arccos(c).astype(np.float32) * np.float32(180)).astype(np.float64) / np.pi).astype(np.float32)
        return o

    def last_timing(self):
        """(device ms of the last Initialize chain, kernel launches)"""
        return self._timing("orbx_initializer_last_timing", ctypes.c_float, ctypes.c_int)


class Sim3Problem(ctypes.Structure):
    _fields_ = [("rcw1", ctypes.c_float * 9), ("tcw1", ctypes.c_float * 3), ("rcw2", ctypes.c_float * 9), ("tcw2", ctypes.c_float * 3),
                ("fx1", ctypes.c_float), ("fy1", ctypes.c_float), ("cx1", ctypes.c_float), ("cy1", ctypes.c_float),
                ("fx2", ctypes.c_float), ("fy2", ctypes.c_float), ("cx2", ctypes.c_float), ("cy2", ctypes.c_float),
                ("n", ctypes.c_int), ("world1", ctypes.c_void_p), ("world2", ctypes.c_void_p), ("sigma2_1", ctypes.c_void_p), ("sigma2_2", ctypes.c_void_p),
                ("sets", ctypes.c_void_p), ("iterations", ctypes.c_int), ("min_inliers", ctypes.c_int), ("fix_scale", ctypes.c_int)]


_SIM3_RESULT_FIELDS = ("count", "r12", "t12", "s12", "is_event", "first_event", "best_iteration", "no_more", "inliers_first", "x3dc1", "x3dc2", "p1im1", "p2im2",
                       "max_err1", "max_err2", "nmat", "quat", "t12m", "t21m")


class Sim3Result(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _SIM3_RESULT_FIELDS]


def sim3_sets(n, iterations, randint):
    """The minimal sets of Sim3Solver::iterate (reference src/Sim3Solver.cc:228-249): `iterations` sets of 3 distinct indices into n kept pairs, each
    drawn as randint(0, len(available) - 1) (both bounds inclusive, like DUtils::Random::RandomInt) from the list of indices still available; the
    drawn slot is overwritten with the list's back and the back is popped.  -> (iterations, 3) int32"""
    if n < 3 and iterations > 0:
        raise ValueError("sim3_sets: %d matches, a set needs 3" % n)
    out = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(3):
            r = int(randint(0, len(avail) - 1))
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def sim3_ransac_iterations(prob, min_inliers, max_iterations, n):
    """mRansacMaxIts of Sim3Solver::SetRansacParameters (:143-196); needs no device"""
    L = load_library()
    L.orbx_sim3_ransac_iterations.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return int(L.orbx_sim3_ransac_iterations(float(prob), int(min_inliers), int(max_iterations), int(n)))


class Sim3Candidate:
    """One solved candidate: the device's per-iteration outputs, and the reference's stateful surface replayed from them on the host.
    iterate(nIterations) -> (T12 (4,4) float32 or None, bNoMore, vbInliers (mN1) bool, nInliers), call after call, also after a success."""

    def __init__(self, solver, index, out, n, n1, indices1, min_inliers):
        self._solver, self._index, self.n, self.mN1, self.indices1, self.min_inliers = solver, index, n, n1, indices1, min_inliers
        self.__dict__.update(out)
        self.iterations = len(self.count)
        self.mnIterations = 0
        self._best, self._best_count = -1, 0

    def inliers(self, iteration):
        """mvbInliersi (n, compacted) of any iteration: one row of the device's masks"""
        return self._solver._inliers(self._index, iteration, self.n)

    def T12(self, iteration):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.float32(self.s12[iteration]) * self.r12[iteration]
        T[:3, 3] = self.t12[iteration]
        return T

    def iterate(self, nIterations):
        vb = np.zeros(self.mN1, bool)
        if self.n < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.mnIterations < self.iterations and cur < nIterations:
            it = self.mnIterations
            cur += 1
            self.mnIterations += 1
            if self.count[it] < self._best_count:
                continue
            self._best, self._best_count = it, int(self.count[it])
            if self.count[it] > self.min_inliers:
                inl = self.inliers_first if it == self.first_event else self.inliers(it)
                vb[self.indices1[inl]] = True
                return self.T12(it), False, vb, int(self.count[it])
        return None, self.mnIterations >= self.iterations, vb, 0

    def find(self):
        T, _, vb, k = self.iterate(self.iterations)
        return T, vb, k

    def GetEstimatedRotation(self):
        return self.r12[self._best].copy()

    def GetEstimatedTranslation(self):
        return self.t12[self._best].copy()

    def GetEstimatedScale(self):
        return np.float32(self.s12[self._best])


class Sim3Solver(_Handle):
    """Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc) on the device: every RANSAC iteration of every loop candidate in one launch
    chain (orbx_sim3_solve), and CheckInliers on explicit transformations (CheckModels)."""
    _destroy = "orbx_sim3_solver_destroy"

    def __init__(self, max_candidates=8, max_matches=2048, max_iterations=300, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_sim3_solver_create.argtypes = [ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_sim3_solver_destroy.argtypes = [vp]
        L.orbx_sim3_solver_destroy.restype = None
        L.orbx_sim3_solve.argtypes = [vp, ctypes.POINTER(Sim3Problem), ci, ctypes.POINTER(Sim3Result)]
        L.orbx_sim3_inliers.argtypes = [vp, ci, ci, vp]
        L.orbx_sim3_check_models.argtypes = [vp, ctypes.POINTER(Sim3Problem), vp, vp, ci, vp, vp]
        L.orbx_sim3_last_timing.argtypes = [vp, vp, vp]
        self.max_candidates, self.max_matches, self.max_iterations = int(max_candidates), int(max_matches), int(max_iterations)
        self._h = vp()
        _check(L.orbx_sim3_solver_create(device, self.max_candidates, self.max_matches, self.max_iterations, ctypes.byref(self._h)))

    @staticmethod
    def _problem(c, keep):
        """c: dict(Rcw1 (3,3), tcw1 (3), Rcw2, tcw2, K1 (fx, fy, cx, cy), K2, world1 (n,3), world2 (n,3), sigma2_1 (n), sigma2_2 (n))"""
        f4 = np.float32
        w1, w2 = np.ascontiguousarray(c["world1"], f4).reshape(-1, 3), np.ascontiguousarray(c["world2"], f4).reshape(-1, 3)
        s1, s2 = np.ascontiguousarray(c["sigma2_1"], f4).reshape(-1), np.ascontiguousarray(c["sigma2_2"], f4).reshape(-1)
        n = len(w1)
        if not (len(w2) == len(s1) == len(s2) == n):
            raise ValueError("Sim3Solver: the per-pair arrays of a candidate disagree in length")
        keep.extend([w1, w2, s1, s2])
        P = Sim3Problem()
        for name, key, k in (("rcw1", "Rcw1", 9), ("tcw1", "tcw1", 3), ("rcw2", "Rcw2", 9), ("tcw2", "tcw2", 3)):
            setattr(P, name, (ctypes.c_float * k)(*np.asarray(c[key], f4).reshape(-1)))
        P.fx1, P.fy1, P.cx1, P.cy1 = [float(v) for v in c["K1"]]
        P.fx2, P.fy2, P.cx2, P.cy2 = [float(v) for v in c["K2"]]
        P.n, P.world1, P.world2, P.sigma2_1, P.sigma2_2 = n, w1.ctypes.data, w2.ctypes.data, s1.ctypes.data, s2.ctypes.data
        return P, n

    def Solve(self, candidates, sets=None, rng=None, prob=0.99, min_inliers=20, max_iterations=300, fix_scale=False, full=False):
        """candidates: list of dicts (see _problem; optional "indices1" (n) = mvnIndices1 and "mN1" = len(vpMatched12), default the identity).
        sets: list of (iterations,3) int32 per candidate or None = mRansacMaxIts sets per candidate drawn by sim3_sets from rng (numpy Generator,
        default seed 0), candidate after candidate.  -> [Sim3Candidate]; full=True adds every diagnostic of orbx_sim3_result."""
        C = len(candidates)
        keep, probs, ns = [], (Sim3Problem * max(C, 1))(), []
        g = np.random.default_rng(0) if rng is None else rng
        used = []
        for c, cd in enumerate(candidates):
            P, n = self._problem(cd, keep)
            if sets is None:
                its = sim3_ransac_iterations(prob, min_inliers, max_iterations, n) if n >= min_inliers else 0
                s = sim3_sets(n, its, lambda lo, hi: g.integers(lo, hi + 1))
            else:
                s = np.ascontiguousarray(sets[c], np.int32).reshape(-1, 3)
            used.append(s)
            P.sets, P.iterations, P.min_inliers, P.fix_scale = s.ctypes.data, len(s), int(min_inliers), 1 if fix_scale else 0
            probs[c] = P
            ns.append(n)
        f4, i4, u1 = np.float32, np.int32, np.uint8
        res, outs = (Sim3Result * max(C, 1))(), []
        for c in range(C):
            n, it = ns[c], (len(used[c]) if ns[c] >= min_inliers else 0)
            o = dict(count=np.zeros(it, i4), r12=np.zeros((it, 3, 3), f4), t12=np.zeros((it, 3), f4), s12=np.zeros(it, f4), is_event=np.zeros(it, u1),
                     first_event=np.zeros(1, i4), best_iteration=np.zeros(1, i4), no_more=np.zeros(1, i4), inliers_first=np.zeros(n, u1))
            if full:
                o.update(x3dc1=np.zeros((n, 3), f4), x3dc2=np.zeros((n, 3), f4), p1im1=np.zeros((n, 2), f4), p2im2=np.zeros((n, 2), f4), max_err1=np.zeros(n, f4),
                         max_err2=np.zeros(n, f4), nmat=np.zeros((it, 4, 4), f4), quat=np.zeros((it, 4), f4), t12m=np.zeros((it, 4, 4), f4), t21m=np.zeros((it, 4, 4), f4))
            res[c] = Sim3Result(*[o[k].ctypes.data if k in o and o[k].size else None for k in _SIM3_RESULT_FIELDS])
            outs.append(o)
        _check(self._L.orbx_sim3_solve(self._h, probs, C, res))
        result = []
        for c, o in enumerate(outs):
            for k in ("first_event", "best_iteration"):
                o[k] = int(o[k][0])
            o["no_more"] = bool(o["no_more"][0])
            o["is_event"], o["inliers_first"] = o["is_event"].astype(bool), o["inliers_first"].astype(bool)
            o["sets"] = used[c][:len(o["count"])]
            cd = candidates[c]
            idx = np.asarray(cd["indices1"], np.int64) if "indices1" in cd else np.arange(ns[c])
            result.append(Sim3Candidate(self, c, o, ns[c], int(cd.get("mN1", ns[c])), idx, int(min_inliers)))
        return result

    def _inliers(self, candidate, iteration, n):
        out = np.zeros(max(n, 1), np.uint8)
        _check(self._L.orbx_sim3_inliers(self._h, int(candidate), int(iteration), out.ctypes.data))
        return out[:n].astype(bool)

    def CheckModels(self, candidate, t12, t21):
        """CheckInliers of the explicit transformations t12, t21 (M,4,4) over a candidate's pairs -> (count (M) int32, inliers (M,n) bool)"""
        keep = []
        P, n = self._problem(candidate, keep)
        a, b = np.ascontiguousarray(t12, np.float32).reshape(-1, 16), np.ascontiguousarray(t21, np.float32).reshape(-1, 16)
        M = len(a)
        if len(b) != M:
            raise ValueError("Sim3Solver.CheckModels: %d T12 for %d T21" % (M, len(b)))
        count, inl = np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1) * max(n, 1), np.uint8)
        _check(self._L.orbx_sim3_check_models(self._h, ctypes.byref(P), a.ctypes.data, b.ctypes.data, M, count.ctypes.data, inl.ctypes.data))
        return count[:M], inl[:M * n].reshape(M, n).astype(bool)

    def last_timing(self):
        """(device ms of the last Solve chain, kernel launches)"""
        return self._timing("orbx_sim3_last_timing", ctypes.c_float, ctypes.c_int)


class Sim3OptProblem(ctypes.Structure):
    _fields_ = [("rcw1", ctypes.c_float * 9), ("tcw1", ctypes.c_float * 3), ("rcw2", ctypes.c_float * 9), ("tcw2", ctypes.c_float * 3),
                ("fx1", ctypes.c_float), ("fy1", ctypes.c_float), ("cx1", ctypes.c_float), ("cy1", ctypes.c_float),
                ("fx2", ctypes.c_float), ("fy2", ctypes.c_float), ("cx2", ctypes.c_float), ("cy2", ctypes.c_float),
                ("n", ctypes.c_int), ("world1", ctypes.c_void_p), ("world2", ctypes.c_void_p), ("obs1", ctypes.c_void_p), ("obs2", ctypes.c_void_p),
                ("inv_sigma2_1", ctypes.c_void_p), ("inv_sigma2_2", ctypes.c_void_p),
                ("r12", ctypes.c_double * 9), ("t12", ctypes.c_double * 3), ("s12", ctypes.c_double), ("th2", ctypes.c_float), ("fix_scale", ctypes.c_int)]


_SIM3_OPT_RESULT_FIELDS = ("n_inliers", "quat", "t", "s", "r12", "removed_first", "removed_final", "n_bad", "chi2_round1", "chi2_round2", "stats", "x3dc1", "x3dc2")


class Sim3OptResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _SIM3_OPT_RESULT_FIELDS]


class Sim3Refined:
    """One optimised problem: n_inliers (the reference's return value), quat (x, y, z, w) / t / s (g2oS12 afterwards, float64), r12 (3,3) float32,
    removed_first / removed_final (n) bool (the pairs the caller nulls in vpMatches1), n_bad; with full=True also chi2_round1 / chi2_round2 (n,2),
    stats (2,2) = (Levenberg iterations, final robust chi2) per round, x3dc1 / x3dc2 (n,3)."""

    def __init__(self, out):
        self.__dict__.update(out)

    @property
    def removed(self):
        return self.removed_first | self.removed_final

    def T12(self):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.float32(self.s) * self.r12
        T[:3, 3] = self.t.astype(np.float32)
        return T


def sim3_opt_problem(candidate, solved, matches, iteration=None):
    """A Sim3Optimizer problem from a Sim3Solver event: `candidate` is the dict Sim3Solver.Solve took (poses and intrinsics are read), `solved` the
    Sim3Candidate it returned, `iteration` the event (default: the first), `matches` SearchBySim3's pairs as a dict(world1 (n,3), world2 (n,3),
    obs1 (n,2), obs2 (n,2), inv_sigma2_1 (n), inv_sigma2_2 (n)).  The float R, t, s of the event are widened, as LoopClosing::ComputeSim3 builds gScm."""
    it = solved.first_event if iteration is None else int(iteration)
    if it < 0:
        raise ValueError("sim3_opt_problem: the candidate has no event")
    p = {k: candidate[k] for k in ("Rcw1", "tcw1", "Rcw2", "tcw2", "K1", "K2")}
    p.update({k: matches[k] for k in ("world1", "world2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")})
    p.update(R12=solved.r12[it].astype(np.float64), t12=solved.t12[it].astype(np.float64), s12=float(solved.s12[it]))
    return p


class Sim3Optimizer(_Handle):
    """Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1364-1590) on the device: every problem of a call in one launch (orbx_optimize_sim3)."""
    _destroy = "orbx_sim3_optimizer_destroy"

    def __init__(self, max_problems=8, max_pairs=1024, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_sim3_optimizer_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_sim3_optimizer_destroy.argtypes = [vp]
        L.orbx_sim3_optimizer_destroy.restype = None
        L.orbx_optimize_sim3.argtypes = [vp, ctypes.POINTER(Sim3OptProblem), ci, ctypes.POINTER(Sim3OptResult)]
        L.orbx_optimize_sim3_linearize.argtypes = [vp, ctypes.POINTER(Sim3OptProblem), vp, vp, ctypes.c_double, vp, vp, vp, vp, vp, vp]
        L.orbx_sim3_optimizer_last_timing.argtypes = [vp, vp, vp]
        self.max_problems, self.max_pairs = int(max_problems), int(max_pairs)
        self._h = vp()
        _check(L.orbx_sim3_optimizer_create(device, self.max_problems, self.max_pairs, ctypes.byref(self._h)))

    @staticmethod
    def _problem(c, keep, th2, fix_scale):
        """c: dict(Rcw1 (3,3), tcw1 (3), Rcw2, tcw2, K1 (fx, fy, cx, cy), K2, world1 (n,3), world2 (n,3), obs1 (n,2), obs2 (n,2), inv_sigma2_1 (n),
        inv_sigma2_2 (n), R12 (3,3) float64, t12 (3), s12)"""
        f4 = np.float32
        w1, w2 = np.ascontiguousarray(c["world1"], f4).reshape(-1, 3), np.ascontiguousarray(c["world2"], f4).reshape(-1, 3)
        o1, o2 = np.ascontiguousarray(c["obs1"], f4).reshape(-1, 2), np.ascontiguousarray(c["obs2"], f4).reshape(-1, 2)
        s1, s2 = np.ascontiguousarray(c["inv_sigma2_1"], f4).reshape(-1), np.ascontiguousarray(c["inv_sigma2_2"], f4).reshape(-1)
        n = len(w1)
        if not (len(w2) == len(o1) == len(o2) == len(s1) == len(s2) == n):
            raise ValueError("Sim3Optimizer: the per-pair arrays of a problem disagree in length")
        keep.extend([w1, w2, o1, o2, s1, s2])
        P = Sim3OptProblem()
        for name, key, k in (("rcw1", "Rcw1", 9), ("tcw1", "tcw1", 3), ("rcw2", "Rcw2", 9), ("tcw2", "tcw2", 3)):
            setattr(P, name, (ctypes.c_float * k)(*np.asarray(c[key], f4).reshape(-1)))
        P.fx1, P.fy1, P.cx1, P.cy1 = [float(v) for v in c["K1"]]
        P.fx2, P.fy2, P.cx2, P.cy2 = [float(v) for v in c["K2"]]
        P.n = n
        P.world1, P.world2, P.obs1, P.obs2, P.inv_sigma2_1, P.inv_sigma2_2 = [a.ctypes.data for a in (w1, w2, o1, o2, s1, s2)]
        P.r12 = (ctypes.c_double * 9)(*np.asarray(c["R12"], np.float64).reshape(-1))
        P.t12 = (ctypes.c_double * 3)(*np.asarray(c["t12"], np.float64).reshape(-1))
        P.s12, P.th2, P.fix_scale = float(c["s12"]), float(th2), 1 if fix_scale else 0
        return P, n

    def OptimizeSim3(self, problems, th2=10, fix_scale=False, full=False):
        """problems: list of dicts (see _problem, sim3_opt_problem) -> [Sim3Refined]; full=True adds the diagnostics of orbx_sim3_opt_result."""
        C = len(problems)
        keep, probs, ns = [], (Sim3OptProblem * max(C, 1))(), []
        for c, cd in enumerate(problems):
            probs[c], n = self._problem(cd, keep, th2, fix_scale)
            ns.append(n)
        f8, f4, i4, u1 = np.float64, np.float32, np.int32, np.uint8
        res, outs = (Sim3OptResult * max(C, 1))(), []
        for c in range(C):
            n = ns[c]
            o = dict(n_inliers=np.zeros(1, i4), quat=np.zeros(4, f8), t=np.zeros(3, f8), s=np.zeros(1, f8), r12=np.zeros((3, 3), f4), removed_first=np.zeros(n, u1),
                     removed_final=np.zeros(n, u1), n_bad=np.zeros(1, i4))
            if full:
                o.update(chi2_round1=np.zeros((n, 2), f8), chi2_round2=np.zeros((n, 2), f8), stats=np.zeros((2, 2), f8), x3dc1=np.zeros((n, 3), f4), x3dc2=np.zeros((n, 3), f4))
            res[c] = Sim3OptResult(*[o[k].ctypes.data if k in o and o[k].size else None for k in _SIM3_OPT_RESULT_FIELDS])
            outs.append(o)
        _check(self._L.orbx_optimize_sim3(self._h, probs, C, res))
        result = []
        for o in outs:
            o["n_inliers"], o["n_bad"], o["s"] = int(o["n_inliers"][0]), int(o["n_bad"][0]), float(o["s"][0])
            o["removed_first"], o["removed_final"] = o["removed_first"].astype(bool), o["removed_final"].astype(bool)
            result.append(Sim3Refined(o))
        return result

    def linearize(self, problem, quat, t, s, active=None, th2=10, fix_scale=False):
        """One linearisation of a problem's edges at the estimate (quat (x, y, z, w), t, s) with the chain's device functions ->
        dict(errors (2n,2), chi2 (2n), jac (2n,2,7), H (7,7), b (7)); edge 2 i = e12, 2 i + 1 = e21 of pair i; active (n) bool or None = every pair."""
        keep = []
        P, n = self._problem(problem, keep, th2, fix_scale)
        f8 = np.float64
        q, tt = np.ascontiguousarray(quat, f8).reshape(4), np.ascontiguousarray(t, f8).reshape(3)
        act = None if active is None else np.ascontiguousarray(active, np.uint8).reshape(-1)
        if act is not None and len(act) != n:
            raise ValueError("Sim3Optimizer.linearize: %d active flags for %d pairs" % (len(act), n))
        m = max(n, 1)
        o = dict(errors=np.zeros((2 * m, 2), f8), chi2=np.zeros(2 * m, f8), jac=np.zeros((2 * m, 2, 7), f8), H=np.zeros((7, 7), f8), b=np.zeros(7, f8))
        _check(self._L.orbx_optimize_sim3_linearize(self._h, ctypes.byref(P), q.ctypes.data, tt.ctypes.data, float(s), None if act is None or n == 0 else act.ctypes.data,
                                                    o["errors"].ctypes.data, o["chi2"].ctypes.data, o["jac"].ctypes.data, o["H"].ctypes.data, o["b"].ctypes.data))
        for k in ("errors", "chi2", "jac"):
            o[k] = o[k][:2 * n]
        return o

    def last_timing(self):
        """(device ms of the last OptimizeSim3 launch chain, kernel launches)"""
        return self._timing("orbx_sim3_optimizer_last_timing", ctypes.c_float, ctypes.c_int)


class PnPProblem(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("n", ctypes.c_int),
                ("p2d", ctypes.c_void_p), ("sigma2", ctypes.c_void_p), ("p3dw", ctypes.c_void_p), ("probability", ctypes.c_double),
                ("min_inliers", ctypes.c_int), ("max_iterations", ctypes.c_int), ("min_set", ctypes.c_int), ("epsilon", ctypes.c_float), ("th2", ctypes.c_float),
                ("sets", ctypes.c_void_p), ("iterations", ctypes.c_int)]


_PNP_RESULT_FIELDS = ("count", "r", "t", "err", "record_of", "is_event", "nrecords", "record_iteration", "refined_count", "refined_r", "refined_t", "refined_tcw",
                      "best_tcw", "first_event", "best_iteration", "no_more", "min_inliers", "inliers_first", "inliers_best", "max_error")
# orbx_pnp_epnp(full): name -> (offset, shape) inside the ORBX_PNP_FULL_DOUBLES doubles of a set (ORBX_PNP_F_* of include/orbx.h)
PNP_FULL_DOUBLES = 472
PNP_FULL_LAYOUT = dict(cws=(0, (4, 3)), pca=(12, (3, 3)), dc=(21, (3,)), uct=(24, (3, 3)), ci=(33, (3, 3)), mtm=(42, (12, 12)), d=(186, (12,)), ut=(198, (12, 12)),
                       L=(342, (6, 10)), rho=(402, (6,)), b0=(408, (3, 4)), b1=(420, (3, 4)), Rs=(432, (3, 3, 3)), ts=(459, (3, 3)), errs=(468, (3,)), choice=(471, ()))


class PnPResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _PNP_RESULT_FIELDS]


def pnp_sets(n, iterations, randint):
    """The minimal sets of PnPsolver::iterate (reference src/PnPsolver.cc:274-290): `iterations` sets of mRansacMinSet = 4 distinct indices into n kept
    matches, each drawn as randint(0, len(available) - 1) (both bounds inclusive, like DUtils::Random::RandomInt) from the list of indices still
    available; the drawn slot is overwritten with the list's back and the back is popped.  -> (iterations, 4) int32"""
    if n < 4 and iterations > 0:
        raise ValueError("pnp_sets: %d matches, a set needs 4" % n)
    out = np.zeros((iterations, 4), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(4):
            r = int(randint(0, len(avail) - 1))
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def pnp_ransac_parameters(n, prob=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
    """PnPsolver::SetRansacParameters (:181-223) -> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon); needs no device"""
    L = load_library()
    L.orbx_pnp_ransac_parameters.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    mi, its, eps = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    _check(L.orbx_pnp_ransac_parameters(float(prob), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), float(th2), int(n),
                                        ctypes.byref(mi), ctypes.byref(its), ctypes.byref(eps)))
    return mi.value, its.value, np.float32(eps.value)


class PnPCandidate:
    """One solved candidate: the device's per-iteration and per-record outputs, and the reference's stateful surface replayed from them on the host.
    iterate(nIterations) -> (Tcw (4,4) float32 or None, bNoMore, vbInliers (mN) bool, nInliers), call after call, also after a success; the loop
    condition is the reference's (:266) `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`.  Iterations beyond the sets already solved
    are solved by a further device call on further sets (drawn from the same generator)."""

    def __init__(self, solver, cand, params, out, rng):
        self._solver, self._cand, self._params, self._rng = solver, cand, params, rng
        self.n = len(out["inliers_best"])
        idx = cand.get("indices")
        self.indices = np.arange(self.n) if idx is None else np.asarray(idx, np.int64)
        self.mN = int(cand.get("mN", self.n))
        self.mnIterations = 0
        self._take(out)
        self.mRansacMaxIts = params["max_its"]

    def _take(self, out):
        self.__dict__.update(out)
        self.iterations = len(self.count)

    @staticmethod
    def _tcw(rows):
        T = np.eye(4, dtype=np.float32)
        T[:3, :] = np.asarray(rows, np.float32).reshape(3, 4)
        return T

    def Tcw(self, iteration):
        """mRi, mti of an iteration narrowed to float (:310-316)"""
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = self.r[iteration].astype(np.float32)
        T[:3, 3] = self.t[iteration].astype(np.float32)
        return T

    def _extend(self, more):
        extra = pnp_sets(self.n, int(more), lambda lo, hi: self._rng.integers(lo, hi + 1))
        sets = np.concatenate([self.sets, extra]).astype(np.int32)
        self._take(self._solver._solve([self._cand], [sets], self._params, False)[0])

    def iterate(self, nIterations):
        vb = np.zeros(self.mN, bool)
        if self.n < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:
            cur += 1
            it = self.mnIterations
            self.mnIterations += 1
            if it >= self.iterations:
                self._extend(max(1, nIterations - cur + 1, self.mRansacMaxIts - it))
            if self.count[it] >= self.min_inliers:
                rec = int(self.record_of[it])
                if self.refined_count[rec] > self.min_inliers:
                    vb[self.indices[self.refined_masks[rec]]] = True
                    return self._tcw(self.refined_tcw[rec]), False, vb, int(self.refined_count[rec])
        if self.mnIterations >= self.mRansacMaxIts:
            rec = int(self.record_of[self.mnIterations - 1])
            if rec >= 0:
                b = int(self.record_iteration[rec])
                vb[self.indices[self.record_masks[rec]]] = True
                return self.Tcw(b), True, vb, int(self.count[b])
            return None, True, vb, 0
        return None, False, vb, 0

    def find(self):
        T, _, vb, k = self.iterate(self.mRansacMaxIts)
        return T, vb, k


class PnPsolver(_Handle):
    """PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc) on the device: every RANSAC iteration and every Refine of every relocalisation
    candidate in one launch chain (orbx_pnp_solve); CheckInliers on explicit poses (CheckModels) and compute_pose on explicit sets (EPnP)."""
    _destroy = "orbx_pnp_solver_destroy"

    def __init__(self, max_candidates=8, max_matches=2048, max_iterations=300, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_pnp_solver_create.argtypes = [ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_pnp_solver_destroy.argtypes = [vp]
        L.orbx_pnp_solver_destroy.restype = None
        L.orbx_pnp_solve.argtypes = [vp, ctypes.POINTER(PnPProblem), ci, ctypes.POINTER(PnPResult)]
        L.orbx_pnp_inliers.argtypes = [vp, ci, ci, ci, vp]
        L.orbx_pnp_check_models.argtypes = [vp, ctypes.POINTER(PnPProblem), vp, vp, ci, vp, vp]
        L.orbx_pnp_epnp.argtypes = [vp, ctypes.POINTER(PnPProblem), vp, ci, ci, vp, vp, vp, vp, vp]
        L.orbx_pnp_last_timing.argtypes = [vp, vp, vp]
        self.max_candidates, self.max_matches, self.max_iterations = int(max_candidates), int(max_matches), int(max_iterations)
        self._h = vp()
        _check(L.orbx_pnp_solver_create(device, self.max_candidates, self.max_matches, self.max_iterations, ctypes.byref(self._h)))

    @staticmethod
    def _problem(c, keep, params):
        """c: dict(K (fx, fy, cx, cy), p2d (n,2) mvP2D, sigma2 (n) mvLevelSigma2[octave], p3d (n,3) mvP3Dw)"""
        f4 = np.float32
        p2, p3 = np.ascontiguousarray(c["p2d"], f4).reshape(-1, 2), np.ascontiguousarray(c["p3d"], f4).reshape(-1, 3)
        s2 = np.ascontiguousarray(c["sigma2"], f4).reshape(-1)
        n = len(p2)
        if not (len(p3) == len(s2) == n):
            raise ValueError("PnPsolver: the per-match arrays of a candidate disagree in length")
        keep.extend([p2, p3, s2])
        P = PnPProblem()
        P.fx, P.fy, P.cx, P.cy = [float(v) for v in c["K"]]
        P.n, P.p2d, P.sigma2, P.p3dw = n, p2.ctypes.data, s2.ctypes.data, p3.ctypes.data
        P.probability, P.min_inliers, P.max_iterations, P.min_set = float(params["prob"]), int(params["min_inliers"]), int(params["max_iterations"]), int(params["min_set"])
        P.epsilon, P.th2 = float(params["epsilon"]), float(params["th2"])
        return P, n

    def Solve(self, candidates, sets=None, rng=None, prob=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991, full=False):
        """candidates: list of dicts (see _problem; optional "indices" (n) = mvKeyPointIndices and "mN" = len(vpMapPointMatches), default the identity).
        sets: list of (iterations,4) int32 per candidate or None = mRansacMaxIts sets per candidate drawn by pnp_sets from rng (numpy Generator,
        default seed 0), candidate after candidate.  -> [PnPCandidate]; full=True adds the mask of every iteration (masks) and max_error."""
        params = dict(prob=prob, min_inliers=min_inliers, max_iterations=max_iterations, min_set=min_set, epsilon=epsilon, th2=th2)
        g = np.random.default_rng(0) if rng is None else rng
        used = []
        for c, cd in enumerate(candidates):
            n = len(np.asarray(cd["p2d"]).reshape(-1, 2))
            mi, its, _ = pnp_ransac_parameters(n, prob, min_inliers, max_iterations, min_set, epsilon, th2)
            if sets is None:
                s = pnp_sets(n, its if n >= mi else 0, lambda lo, hi: g.integers(lo, hi + 1))
            else:
                s = np.ascontiguousarray(sets[c], np.int32).reshape(-1, 4)
            used.append(s)
        outs = self._solve(candidates, used, params, full)
        result = []
        for c, o in enumerate(outs):
            n = len(o["inliers_best"])
            _, its, _ = pnp_ransac_parameters(n, prob, min_inliers, max_iterations, min_set, epsilon, th2)
            result.append(PnPCandidate(self, candidates[c], dict(params, max_its=its), o, g))
        return result

    def _solve(self, candidates, used, params, full):
        C = len(candidates)
        keep, probs, ns = [], (PnPProblem * max(C, 1))(), []
        for c, cd in enumerate(candidates):
            P, n = self._problem(cd, keep, params)
            s = np.ascontiguousarray(used[c], np.int32).reshape(-1, 4)
            keep.append(s)
            P.sets, P.iterations = s.ctypes.data, len(s)
            probs[c] = P
            ns.append(n)
        f4, f8, i4, u1 = np.float32, np.float64, np.int32, np.uint8
        res, outs = (PnPResult * max(C, 1))(), []
        for c in range(C):
            n, it = ns[c], len(used[c])
            o = dict(count=np.zeros(it, i4), r=np.zeros((it, 3, 3), f8), t=np.zeros((it, 3), f8), err=np.zeros(it, f8), record_of=np.full(it, -1, i4), is_event=np.zeros(it, u1),
                     nrecords=np.zeros(1, i4), record_iteration=np.full(it, -1, i4), refined_count=np.zeros(it, i4), refined_r=np.zeros((it, 3, 3), f8),
                     refined_t=np.zeros((it, 3), f8), refined_tcw=np.zeros((it, 12), f4), best_tcw=np.zeros(12, f4), first_event=np.full(1, -1, i4),
                     best_iteration=np.full(1, -1, i4), no_more=np.zeros(1, i4), min_inliers=np.zeros(1, i4), inliers_first=np.zeros(n, u1), inliers_best=np.zeros(n, u1))
            if full:
                o["max_error"] = np.zeros(n, f4)
            res[c] = PnPResult(*[o[k].ctypes.data if k in o and o[k].size else None for k in _PNP_RESULT_FIELDS])
            outs.append(o)
        _check(self._L.orbx_pnp_solve(self._h, probs, C, res))
        for c, o in enumerate(outs):
            for k in ("first_event", "best_iteration", "nrecords", "min_inliers"):
                o[k] = int(o[k][0])
            o["no_more"] = bool(o["no_more"][0])
            ran = 0 if o["no_more"] else len(used[c])      # n < min_inliers: nothing was run
            for k in ("count", "r", "t", "err", "record_of", "is_event", "record_iteration", "refined_count", "refined_r", "refined_t", "refined_tcw"):
                o[k] = o[k][:ran]
            o["is_event"], o["inliers_first"], o["inliers_best"] = o["is_event"].astype(bool), o["inliers_first"].astype(bool), o["inliers_best"].astype(bool)
            o["sets"] = np.asarray(used[c], np.int32).reshape(-1, 4)[:ran]
            # the rows iterate can return: the refined mask of every record and the mask of every record's iteration (host copies, made before
            # another call overwrites the device's)
            o["refined_masks"] = [self._inliers(c, r, 1, ns[c]) for r in range(o["nrecords"])]
            o["record_masks"] = [self._inliers(c, int(o["record_iteration"][r]), 0, ns[c]) for r in range(o["nrecords"])]
            if full:
                o["masks"] = np.array([self._inliers(c, i, 0, ns[c]) for i in range(ran)], bool).reshape(ran, ns[c])
        return outs

    def _inliers(self, candidate, index, refined, n):
        out = np.zeros(max(n, 1), np.uint8)
        _check(self._L.orbx_pnp_inliers(self._h, int(candidate), int(index), int(refined), out.ctypes.data))
        return out[:n].astype(bool)

    _DEFAULTS = dict(prob=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)

    def CheckModels(self, candidate, R, t, th2=5.991):
        """CheckInliers of the explicit poses R (M,3,3), t (M,3) (float64) over a candidate's matches -> (count (M) int32, inliers (M,n) bool)"""
        keep = []
        P, n = self._problem(candidate, keep, dict(self._DEFAULTS, th2=th2))
        a, b = np.ascontiguousarray(R, np.float64).reshape(-1, 9), np.ascontiguousarray(t, np.float64).reshape(-1, 3)
        M = len(a)
        if len(b) != M:
            raise ValueError("PnPsolver.CheckModels: %d R for %d t" % (M, len(b)))
        count, inl = np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1) * max(n, 1), np.uint8)
        _check(self._L.orbx_pnp_check_models(self._h, ctypes.byref(P), a.ctypes.data, b.ctypes.data, M, count.ctypes.data, inl.ctypes.data))
        return count[:M], inl[:M * n].reshape(M, n).astype(bool)

    def EPnP(self, candidate, sets, full=False):
        """compute_pose (:684-759) on explicit index sets (M, set_size >= 4) -> dict(R (M,3,3), t (M,3), err (M)); full=True adds every stage output of
        PNP_FULL_LAYOUT, each with a leading M, and alphas (M, set_size, 4)"""
        keep = []
        P, n = self._problem(candidate, keep, self._DEFAULTS)
        s = np.ascontiguousarray(sets, np.int32)
        if s.ndim != 2:
            raise ValueError("PnPsolver.EPnP: sets must be (M, set_size)")
        M, k = s.shape
        R, t, err = np.zeros((max(M, 1), 3, 3)), np.zeros((max(M, 1), 3)), np.zeros(max(M, 1))
        blk = np.zeros((max(M, 1), PNP_FULL_DOUBLES)) if full else None
        al = np.zeros((max(M, 1), max(k, 1), 4)) if full else None
        _check(self._L.orbx_pnp_epnp(self._h, ctypes.byref(P), s.ctypes.data, M, k, R.ctypes.data, t.ctypes.data, err.ctypes.data,
                                     blk.ctypes.data if full else None, al.ctypes.data if full else None))
        o = dict(R=R[:M], t=t[:M], err=err[:M])
        if full:
            for name, (off, shape) in PNP_FULL_LAYOUT.items():
                size = int(np.prod(shape)) if shape else 1
                o[name] = blk[:M, off:off + size].reshape((M,) + shape).copy()
            o["choice"] = o["choice"].astype(np.int32)
            o["alphas"] = al[:M]
        return o

    def last_timing(self):
        """(device ms of the last Solve chain, kernel launches)"""
        return self._timing("orbx_pnp_last_timing", ctypes.c_float, ctypes.c_int)


class EssentialGraphProblem(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("est", ctypes.c_void_p), ("meas", ctypes.c_void_p), ("fixed", ctypes.c_int), ("fix_scale", ctypes.c_int),
                ("n_edges", ctypes.c_int), ("edges", ctypes.c_void_p), ("n_points", ctypes.c_int), ("points", ctypes.c_void_p), ("point_ref", ctypes.c_void_p),
                ("iterations", ctypes.c_int), ("lambda_init", ctypes.c_double)]


_EG_RESULT_FIELDS = ("est", "tiw", "inv", "points", "chi2", "iterations", "ended", "iter_trials", "iter_chi2", "iter_lambda", "iter_rho", "order", "fill_blocks")
EG_ENDED = ("iterations", "trials", "rho0", "three")


class EssentialGraphCResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _EG_RESULT_FIELDS]


class EssentialGraphResult:
    """One optimised essential graph: est (N,8) float64 rows [qx, qy, qz, qw, tx, ty, tz, s] (the final estimates), Tiw (N,3,4) float32 = [R | t / s] (what
    SetPose takes), inv (N,8) (vCorrectedSwc), points (M,3) float32, chi2 (initial, final), iterations, ended ("iterations", "trials", "rho0", "three"),
    order (N - 1) the elimination order as vertex indices, fill_blocks; with full=True also trials / iter_chi2 / iter_lambda / iter_rho per iteration."""

    def __init__(self, out):
        self.__dict__.update(out)


def _quat_from_R(R):
    """Eigen::Quaterniond(Matrix3d) -> [x, y, z, w]"""
    import math
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    q = [0.0] * 4
    t = (R[0] + R[4]) + R[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
        return q
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def essential_graph_edges(keyframes, loop_kf, cur_kf, corrected, non_corrected, loop_connections, min_feat=100):
    """The vertex and edge selection of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1059-1262) on plain data.
    keyframes: the map's keyframes in any order (they are walked in ascending id, as shim/EssentialGraph_hip.cc does), each a dict(id, parent (id or None), children (ids), loop_edges (ids), covisibles (ids by
    descending weight: GetCovisiblesByWeight keeps those with weight >= min_feat, in this order), weights (id -> weight), bad, Rcw (3,3), tcw (3));
    loop_kf / cur_kf: ids; corrected / non_corrected: id -> Sim3 [qx, qy, qz, qw, tx, ty, tz, s]; loop_connections: id -> ids.
    -> dict(ids (ascending, the bad keyframes left out), est (N,8) = vScw, meas (N,8), fixed, edges (E,3) int32 = (i, j, kind)): vertex 0 of an edge is i;
    kind 0 = a LoopConnections edge (measured from est), kind 1 = spanning tree, loop or covisibility (measured from meas).  The rules: a
    LoopConnections edge below min_feat is skipped unless it is the (current, loop) pair; sInsertedEdges holds the LoopConnections pairs and
    dedupes covisibility edges only; loop and covisibility edges go towards the smaller id; covisibility edges skip the parent, the children,
    the loop edges and bad keyframes."""
    good = [kf for kf in keyframes if not kf.get("bad", False)]
    ids = sorted(kf["id"] for kf in good)
    index = {k: n for n, k in enumerate(ids)}
    by_id = {kf["id"]: kf for kf in keyframes}
    est, meas = np.zeros((len(ids), 8)), np.zeros((len(ids), 8))
    for kf in good:
        k = kf["id"]
        if k in corrected:
            est[index[k]] = np.asarray(corrected[k], np.float64).reshape(8)
        else:
            est[index[k]] = _quat_from_R(kf["Rcw"]) + [float(v) for v in np.asarray(kf["tcw"], np.float64).reshape(3)] + [1.0]
        meas[index[k]] = np.asarray(non_corrected[k], np.float64).reshape(8) if k in non_corrected else est[index[k]]
    edges, inserted = [], set()
    for ki, conns in loop_connections.items():
        for kj in (sorted(conns) if isinstance(conns, (set, frozenset)) else conns):
            if (ki != cur_kf or kj != loop_kf) and by_id[ki]["weights"].get(kj, 0) < min_feat:
                continue
            if ki in index and kj in index:
                edges.append((index[ki], index[kj], 0))
            inserted.add((min(ki, kj), max(ki, kj)))
    for kf in sorted(good, key=lambda k: k["id"]):      # ascending id, as the shim walks them: the edge order is the summation order
        ki = kf["id"]
        par = kf.get("parent")
        if par is not None and par in index:
            edges.append((index[ki], index[par], 1))
        loops = set(kf.get("loop_edges", ()))
        for kl in sorted(loops):
            if kl < ki and kl in index:
                edges.append((index[ki], index[kl], 1))
        children = set(kf.get("children", ()))
        for kn in kf.get("covisibles", ()):
            if kf["weights"].get(kn, 0) < min_feat:
                continue
            if kn == par or kn in children or kn in loops:
                continue
            if by_id[kn].get("bad", False) or not kn < ki:
                continue
            if (min(ki, kn), max(ki, kn)) in inserted:
                continue
            edges.append((index[ki], index[kn], 1))
    return dict(ids=np.array(ids, np.int64), est=est, meas=meas, fixed=index[loop_kf], edges=np.array(edges, np.int32).reshape(-1, 3))


class EssentialGraphOptimizer(_Handle):
    """Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1017-1339) on the device (orbx_optimize_essential_graph)."""
    _destroy = "orbx_essential_graph_destroy"

    def __init__(self, max_keyframes, max_edges, max_points=0, max_fill_blocks=None, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_essential_graph_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_essential_graph_destroy.argtypes = [vp]
        L.orbx_essential_graph_destroy.restype = None
        L.orbx_optimize_essential_graph.argtypes = [vp, ctypes.POINTER(EssentialGraphProblem), ctypes.POINTER(EssentialGraphCResult)]
        L.orbx_essential_graph_linearize.argtypes = [vp, ctypes.POINTER(EssentialGraphProblem)] + [vp] * 8
        L.orbx_essential_graph_solve.argtypes = [vp, ctypes.c_double, vp, vp]
        L.orbx_essential_graph_last_timing.argtypes = [vp, vp, vp, vp]
        self.max_keyframes, self.max_edges, self.max_points = int(max_keyframes), int(max_edges), int(max_points)
        nk = self.max_keyframes
        self.max_fill_blocks = int(max_fill_blocks) if max_fill_blocks is not None else max(1, min(nk * (nk + 1) // 2, 64 * nk))
        self._n = 0
        self._h = vp()
        _check(L.orbx_essential_graph_create(device, self.max_keyframes, self.max_edges, self.max_points, self.max_fill_blocks, ctypes.byref(self._h)))

    @staticmethod
    def _problem(g, keep, fix_scale, iterations, lambda_init):
        """g: dict(est (N,8), meas (N,8) or None, fixed, edges (E,3), points (M,3) and ref (M), both optional), or an object with these attributes"""
        get = (lambda k: g.get(k)) if isinstance(g, dict) else (lambda k: getattr(g, k, None))
        est = np.ascontiguousarray(get("est"), np.float64).reshape(-1, 8)
        meas = None if get("meas") is None else np.ascontiguousarray(get("meas"), np.float64).reshape(-1, 8)
        edges = np.ascontiguousarray(get("edges") if get("edges") is not None else np.zeros((0, 3)), np.int32).reshape(-1, 3)
        pts = np.ascontiguousarray(get("points") if get("points") is not None else np.zeros((0, 3)), np.float32).reshape(-1, 3)
        ref = np.ascontiguousarray(get("ref") if get("ref") is not None else np.zeros(0), np.int32).reshape(-1)
        if meas is not None and len(meas) != len(est):
            raise ValueError("EssentialGraphOptimizer: %d measured poses for %d keyframes" % (len(meas), len(est)))
        if len(ref) != len(pts):
            raise ValueError("EssentialGraphOptimizer: %d references for %d points" % (len(ref), len(pts)))
        keep.extend([est, meas, edges, pts, ref])
        P = EssentialGraphProblem()
        P.n, P.est, P.meas = len(est), est.ctypes.data, None if meas is None else meas.ctypes.data
        P.fixed, P.fix_scale = int(get("fixed")), 1 if fix_scale else 0
        P.n_edges, P.edges = len(edges), edges.ctypes.data if len(edges) else None
        P.n_points, P.points, P.point_ref = len(pts), pts.ctypes.data if len(pts) else None, ref.ctypes.data if len(pts) else None
        P.iterations, P.lambda_init = int(iterations), float(lambda_init)
        return P

    def OptimizeEssentialGraph(self, graph, fix_scale=False, full=False, iterations=20, lambda_init=1e-16):
        """graph: see _problem (essential_graph_edges returns one) -> EssentialGraphResult"""
        keep = []
        P = self._problem(graph, keep, fix_scale, iterations, lambda_init)
        n, m, it = max(P.n, 1), max(P.n_points, 1), max(int(iterations) if iterations > 0 else 20, 1)
        f8, f4, i4 = np.float64, np.float32, np.int32
        o = dict(est=np.zeros((n, 8), f8), tiw=np.zeros((n, 3, 4), f4), inv=np.zeros((n, 8), f8), points=np.zeros((m, 3), f4), chi2=np.zeros(2, f8),
                 iterations=np.zeros(1, i4), ended=np.zeros(1, i4), order=np.zeros(n, i4), fill_blocks=np.zeros(1, i4))
        if full:
            o.update(iter_trials=np.zeros(it, i4), iter_chi2=np.zeros(it, f8), iter_lambda=np.zeros(it, f8), iter_rho=np.zeros(it, f8))
        R = EssentialGraphCResult(*[o[k].ctypes.data if k in o else None for k in _EG_RESULT_FIELDS])
        _check(self._L.orbx_optimize_essential_graph(self._h, ctypes.byref(P), ctypes.byref(R)))
        done = int(o["iterations"][0])
        out = dict(est=o["est"][:P.n], Tiw=o["tiw"][:P.n], inv=o["inv"][:P.n], points=o["points"][:P.n_points], chi2=(float(o["chi2"][0]), float(o["chi2"][1])),
                   iterations=done, ended=EG_ENDED[int(o["ended"][0])], order=o["order"][:max(P.n - 1, 0)].copy(), fill_blocks=int(o["fill_blocks"][0]))
        if full:
            out.update(trials=o["iter_trials"][:done], iter_chi2=o["iter_chi2"][:done], iter_lambda=o["iter_lambda"][:done], iter_rho=o["iter_rho"][:done])
        return EssentialGraphResult(out)

    def linearize(self, graph, at=None, fix_scale=False):
        """One linearisation at the estimates `at` (N,8; default: the graph's est) with the chain's kernels -> dict(meas (E,8), errors (E,7), chi2,
        jac (E,2,7,7), h_diag (N,7,7), h_off (E,7,7), b (N,7)); solve() then runs on it."""
        keep = []
        P = self._problem(graph, keep, fix_scale, 20, 1e-16)
        a = None if at is None else np.ascontiguousarray(at, np.float64).reshape(-1, 8)
        if a is not None and len(a) != P.n:
            raise ValueError("EssentialGraphOptimizer.linearize: %d estimates for %d keyframes" % (len(a), P.n))
        n, e = max(P.n, 1), max(P.n_edges, 1)
        f8 = np.float64
        o = dict(meas=np.zeros((e, 8), f8), errors=np.zeros((e, 7), f8), chi2=np.zeros(1, f8), jac=np.zeros((e, 2, 7, 7), f8), h_diag=np.zeros((n, 7, 7), f8),
                 h_off=np.zeros((e, 7, 7), f8), b=np.zeros((n, 7), f8))
        _check(self._L.orbx_essential_graph_linearize(self._h, ctypes.byref(P), None if a is None else a.ctypes.data,
                                                      *[o[k].ctypes.data for k in ("meas", "errors", "chi2", "jac", "h_diag", "h_off", "b")]))
        self._n = P.n
        for k in ("meas", "errors", "jac", "h_off"):
            o[k] = o[k][:P.n_edges]
        for k in ("h_diag", "b"):
            o[k] = o[k][:P.n]
        o["chi2"] = float(o["chi2"][0])
        return o

    def solve(self, lam):
        """(H + lam I) x = b on the last linearize() -> (ok, x (N,7) by vertex, zeros for the fixed one)"""
        x, ok = np.zeros((max(self._n, 1), 7), np.float64), np.zeros(1, np.int32)
        _check(self._L.orbx_essential_graph_solve(self._h, float(lam), x.ctypes.data, ok.ctypes.data))
        return bool(ok[0]), x[:self._n]

    def last_timing(self):
        """(device ms of the last OptimizeEssentialGraph chain, kernel launches, ms inside the solve kernel)"""
        return self._timing("orbx_essential_graph_last_timing", ctypes.c_float, ctypes.c_int, ctypes.c_float)


KFDB_LOOP, KFDB_RELOC = 0, 1


class KfdbQuery(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("words", ctypes.c_void_p), ("values", ctypes.c_void_p), ("n", ctypes.c_int), ("connected", ctypes.c_void_p),
                ("connected_counts", ctypes.c_void_p), ("n_connected", ctypes.c_int), ("min_score_in", ctypes.c_float), ("capacity", ctypes.c_int)]


_KFDB_RESULT_FIELDS = ("n_sharing", "max_common_words", "min_common_words", "min_score", "connected_score", "scored_id", "scored_words", "scored_score", "n_scored",
                       "kept", "acc_score", "best_id", "n_kept", "best_acc_score", "candidates", "n_candidates")


class KfdbCResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _KFDB_RESULT_FIELDS]


def _kfdb_bow(bow):
    """(words, values) or {word: value} -> (int32 words ascending as given, float64 values)"""
    if isinstance(bow, dict):
        if "words" in bow and "values" in bow:
            bow = (bow["words"], bow["values"])
        else:
            ks = sorted(bow)
            bow = (ks, [bow[k] for k in ks])
    w = np.ascontiguousarray(bow[0], np.int32).reshape(-1)
    v = np.ascontiguousarray(bow[1], np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("KeyFrameDatabase: %d words for %d values" % (len(w), len(v)))
    return w, v


class KeyFrameDatabase(_Handle):
    """KeyFrameDatabase (reference src/KeyFrameDatabase.cc) on the device: add / erase / clear as there, set_covisibles pushes GetBestCovisibilityKeyFrames(10)
    of a keyframe (a query reads the covisibles as last pushed), DetectLoopCandidates / DetectRelocalizationCandidates return the candidate ids in the
    reference's order (full=True: every field of orbx_kfdb_result as a dict), query() runs several queries in one call.  A bow is (words, values) with ascending
    words, or a dict word -> value."""
    _destroy = "orbx_kfdb_destroy"

    def __init__(self, n_words, max_keyframes, max_entries, max_queries=8, max_query_words=4096, device=0):
        self._L = load_library()
        L = self._L
        vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        L.orbx_kfdb_create.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.orbx_kfdb_destroy.argtypes = [vp]
        L.orbx_kfdb_destroy.restype = None
        L.orbx_kfdb_add.argtypes = [vp, i64, vp, vp, ci]
        L.orbx_kfdb_erase.argtypes = [vp, i64]
        L.orbx_kfdb_clear.argtypes = [vp]
        L.orbx_kfdb_set_covisibles.argtypes = [vp, i64, vp, ci]
        L.orbx_kfdb_size.argtypes = [vp, vp, vp, vp]
        L.orbx_kfdb_reloc_score.argtypes = [vp, i64, vp]
        L.orbx_kfdb_query.argtypes = [vp, ctypes.POINTER(KfdbQuery), ci, ctypes.POINTER(KfdbCResult)]
        L.orbx_kfdb_last_timing.argtypes = [vp, vp, vp]
        self.n_words, self.max_keyframes, self.max_entries = int(n_words), int(max_keyframes), int(max_entries)
        self._h = vp()
        _check(L.orbx_kfdb_create(device, self.n_words, self.max_keyframes, self.max_entries, int(max_queries), int(max_query_words), ctypes.byref(self._h)))

    def add(self, kf_id, bow):
        w, v = _kfdb_bow(bow)
        _check(self._L.orbx_kfdb_add(self._h, int(kf_id), w.ctypes.data, v.ctypes.data, len(w)))

    def erase(self, kf_id):
        _check(self._L.orbx_kfdb_erase(self._h, int(kf_id)))

    def clear(self):
        _check(self._L.orbx_kfdb_clear(self._h))

    def set_covisibles(self, kf_id, ids):
        a = np.ascontiguousarray(ids, np.int64).reshape(-1)
        _check(self._L.orbx_kfdb_set_covisibles(self._h, int(kf_id), a.ctypes.data, len(a)))

    def size(self):
        """(alive keyframes, pool entries in use, dead entries)"""
        k, e, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self._L.orbx_kfdb_size(self._h, ctypes.byref(k), ctypes.byref(e), ctypes.byref(d)))
        return k.value, e.value, d.value

    def __len__(self):
        return self.size()[0]

    def reloc_score(self, kf_id):
        s = ctypes.c_float()
        _check(self._L.orbx_kfdb_reloc_score(self._h, int(kf_id), ctypes.byref(s)))
        return np.float32(s.value)

    def stage_timing(self, enable=True, read=False):
        """read=True: device ms of the last query's (staging, intersect, score, commit, select), which must have run with the events enabled; then switch them"""
        ms = (ctypes.c_float * 5)()
        self._L.orbx_kfdb_stage_timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        _check(self._L.orbx_kfdb_stage_timing(self._h, 1 if enable else 0, ms if read else None))
        return tuple(ms) if read else None

    def query(self, queries, marshal_only=False):
        """queries: dicts with mode (KFDB_LOOP / KFDB_RELOC), bow (or words and values), and for loop mode connected (ids), counts (default: all 1),
        min_score_in (default 1.0); capacity (default: the keyframes in the database) -> one dict per query with every field of orbx_kfdb_result"""
        nq = len(queries)
        keep, outs = [], []
        Q, R = (KfdbQuery * max(nq, 1))(), (KfdbCResult * max(nq, 1))()
        alive = len(self)
        for i, q in enumerate(queries):
            w, v = _kfdb_bow(q["bow"] if "bow" in q else (q["words"], q["values"]))
            con = np.ascontiguousarray(q.get("connected", ()), np.int64).reshape(-1)
            cnt = np.ascontiguousarray(q["counts"] if q.get("counts") is not None else np.ones(len(con)), np.int32).reshape(-1)
            if len(cnt) != len(con):
                raise ValueError("KeyFrameDatabase.query: %d counts for %d connected keyframes" % (len(cnt), len(con)))
            cap = int(q.get("capacity", alive))
            keep.extend([w, v, con, cnt])
            Q[i].mode, Q[i].words, Q[i].values, Q[i].n = int(q["mode"]), w.ctypes.data, v.ctypes.data, len(w)
            Q[i].connected, Q[i].connected_counts, Q[i].n_connected = con.ctypes.data, cnt.ctypes.data, len(con)
            Q[i].min_score_in, Q[i].capacity = float(q.get("min_score_in", 1.0)), cap
            c, i4, i8, f4 = max(cap, 1), np.int32, np.int64, np.float32
            o = dict(n_sharing=np.zeros(1, i4), max_common_words=np.zeros(1, i4), min_common_words=np.zeros(1, i4), min_score=np.zeros(1, f4),
                     connected_score=np.zeros(max(len(con), 1), f4), scored_id=np.zeros(c, i8), scored_words=np.zeros(c, i4), scored_score=np.zeros(c, f4),
                     n_scored=np.zeros(1, i4), kept=np.zeros(c, i4), acc_score=np.zeros(c, f4), best_id=np.zeros(c, i8), n_kept=np.zeros(1, i4),
                     best_acc_score=np.zeros(1, f4), candidates=np.zeros(c, i8), n_candidates=np.zeros(1, i4))
            outs.append((o, len(con) if int(q["mode"]) == KFDB_LOOP else 0))
            R[i] = KfdbCResult(*[o[k].ctypes.data for k in _KFDB_RESULT_FIELDS])
        if marshal_only:
            return Q, R, nq, keep, outs
        _check(self._L.orbx_kfdb_query(self._h, Q, nq, R))
        res = []
        for o, ncon in outs:
            ns, nk, ncand = int(o["n_scored"][0]), int(o["n_kept"][0]), int(o["n_candidates"][0])
            res.append(dict(n_sharing=int(o["n_sharing"][0]), max_common_words=int(o["max_common_words"][0]), min_common_words=int(o["min_common_words"][0]),
                            min_score=o["min_score"][0], connected_score=o["connected_score"][:ncon], scored_id=o["scored_id"][:ns], scored_words=o["scored_words"][:ns],
                            scored_score=o["scored_score"][:ns], kept=o["kept"][:nk], acc_score=o["acc_score"][:nk], best_id=o["best_id"][:nk],
                            best_acc_score=o["best_acc_score"][0], candidates=o["candidates"][:ncand]))
        return res

    def DetectLoopCandidates(self, bow, connected, min_score_in=1.0, full=False):
        """connected: GetConnectedKeyFrames as ids, (id, count) pairs or a dict id -> count (count 0 = isBad())"""
        if isinstance(connected, dict):
            connected = list(connected.items())
        connected = list(connected)
        if connected and np.ndim(connected[0]) == 1:
            ids, counts = [c[0] for c in connected], [c[1] for c in connected]
        else:
            ids, counts = connected, None
        r = self.query([dict(mode=KFDB_LOOP, bow=bow, connected=ids, counts=counts, min_score_in=min_score_in)])[0]
        return r if full else [int(i) for i in r["candidates"]]

    def DetectRelocalizationCandidates(self, bow, full=False):
        r = self.query([dict(mode=KFDB_RELOC, bow=bow)])[0]
        return r if full else [int(i) for i in r["candidates"]]

    def last_timing(self):
        """(device ms of the last query chain, kernel launches)"""
        return self._timing("orbx_kfdb_last_timing", ctypes.c_float, ctypes.c_int)


class CovisSlice(ctypes.Structure):
    _fields_ = [("num_keyframes", ctypes.c_int), ("kf_rank", ctypes.c_void_p), ("kf_flags", ctypes.c_void_p), ("num_points", ctypes.c_int), ("num_obs", ctypes.c_int),
                ("obs_offset", ctypes.c_void_p), ("obs_kf", ctypes.c_void_p), ("obs_octave", ctypes.c_void_p), ("obs_stereo", ctypes.c_void_p), ("point_bad", ctypes.c_void_p),
                ("num_lists", ctypes.c_int), ("num_entries", ctypes.c_int), ("list_offset", ctypes.c_void_p), ("list_kf", ctypes.c_void_p), ("list_point", ctypes.c_void_p),
                ("list_octave", ctypes.c_void_p), ("list_close", ctypes.c_void_p)]


class CovisConnections(ctypes.Structure):
    _fields_ = [("counter_offset", ctypes.c_void_p), ("counter_kf", ctypes.c_void_p), ("counter_weight", ctypes.c_void_p), ("counter_capacity", ctypes.c_int),
                ("n_max", ctypes.c_void_p), ("kf_max", ctypes.c_void_p), ("conn_offset", ctypes.c_void_p), ("conn_kf", ctypes.c_void_p), ("conn_weight", ctypes.c_void_p),
                ("conn_capacity", ctypes.c_int)]


class CovisCulling(ctypes.Structure):
    _fields_ = [("n_mps", ctypes.c_void_p), ("n_redundant", ctypes.c_void_p), ("culled", ctypes.c_void_p), ("point_bad", ctypes.c_void_p), ("point_obs", ctypes.c_void_p)]


COVIS_MNID0, COVIS_NOT_ERASE, COVIS_BAD = 1, 2, 4      # kf_flags
COVIS_LDS_KEYFRAMES = 4096      # ORBX_COVIS_LDS_KEYFRAMES

_COVIS_ARRAYS = (("kf_rank", np.int32), ("kf_flags", np.uint8), ("obs_offset", np.int32), ("obs_kf", np.int32), ("obs_octave", np.uint8), ("obs_stereo", np.uint8),
                 ("point_bad", np.uint8), ("list_offset", np.int32), ("list_kf", np.int32), ("list_point", np.int32), ("list_octave", np.uint8), ("list_close", np.uint8))


def covis_slice(keyframes, lists=None, n_points=None, point_bad=None, ranks=None, flags=None):
    """The arrays of orbx_covis_slice from per-keyframe observation tuples.  keyframes[slot] = the keyframe's non-NULL mvpMapPoints in feature order as
    (point, octave, stereo) or (point, octave, stereo, close) tuples (close defaults to 1); a point that a keyframe lists twice is observed by it once (the
    first tuple: mObservations is a map) and stays twice in its list.  lists = the lists of the call: a slot (that keyframe's list) or (-1, tuples) for a
    Frame; default: every keyframe in slot order.  ranks default to the slot numbers, flags and point_bad to 0."""
    NK = len(keyframes)
    M = int(n_points) if n_points is not None else 1 + max([int(t[0]) for kf in keyframes for t in kf] + [int(t[0]) for l in (lists or ()) if not np.isscalar(l) for t in l[1]] + [-1])
    per_point = [[] for _ in range(M)]
    for k, kf in enumerate(keyframes):
        seen = set()
        for t in kf:
            if int(t[0]) not in seen:
                seen.add(int(t[0]))
                per_point[int(t[0])].append((k, int(t[1]), 1 if t[2] else 0))
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in per_point])
    flat = [o for p in per_point for o in p]
    ent, loff, lkf = [], [0], []
    for l in (range(NK) if lists is None else lists):
        owner, tuples = (int(l), keyframes[int(l)]) if np.isscalar(l) else (int(l[0]), l[1])
        ent.extend((int(t[0]), int(t[1]), int(t[3]) if len(t) > 3 else 1) for t in tuples)
        loff.append(len(ent))
        lkf.append(owner)
    col = lambda rows, i, dt: np.array([r[i] for r in rows], dt).reshape(-1)      # noqa: E731
    return dict(kf_rank=np.arange(NK, dtype=np.int32) if ranks is None else np.ascontiguousarray(ranks, np.int32),
                kf_flags=np.zeros(NK, np.uint8) if flags is None else np.ascontiguousarray(flags, np.uint8),
                obs_offset=off, obs_kf=col(flat, 0, np.int32), obs_octave=col(flat, 1, np.uint8), obs_stereo=col(flat, 2, np.uint8),
                point_bad=np.zeros(M, np.uint8) if point_bad is None else np.ascontiguousarray(point_bad, np.uint8),
                list_offset=np.array(loff, np.int32), list_kf=np.array(lkf, np.int32).reshape(-1), list_point=col(ent, 0, np.int32), list_octave=col(ent, 1, np.uint8),
                list_close=col(ent, 2, np.uint8))


def covis_marshal(map_slice, keep):
    """orbx_covis_slice of a dict of arrays (covis_slice's keys); the converted arrays are appended to `keep`, which must outlive the call"""
    a = {k: np.ascontiguousarray(map_slice[k], dt).reshape(-1) for k, dt in _COVIS_ARRAYS}
    keep.append(a)
    NK, M, T, Q, S = len(a["kf_rank"]), len(a["point_bad"]), len(a["obs_kf"]), len(a["list_kf"]), len(a["list_point"])
    if len(a["kf_flags"]) != NK or len(a["obs_offset"]) != M + 1 or len(a["obs_octave"]) != T or len(a["obs_stereo"]) != T or len(a["list_offset"]) != Q + 1 or \
            len(a["list_octave"]) != S or len(a["list_close"]) != S:
        raise ValueError("covisibility slice: array sizes do not agree")
    p = {k: v.ctypes.data for k, v in a.items()}
    return CovisSlice(NK, p["kf_rank"], p["kf_flags"], M, T, p["obs_offset"], p["obs_kf"], p["obs_octave"], p["obs_stereo"], p["point_bad"], Q, S, p["list_offset"], p["list_kf"],
                      p["list_point"], p["list_octave"], p["list_close"]), a


class Covisibility(_Handle):
    """The counting of KeyFrame::UpdateConnections (reference src/KeyFrame.cc:386-507), Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1895-1955) and
    LocalMapping::KeyFrameCulling (src/LocalMapping.cc:873-956) on the device, over a slice of the map (covis_slice); keyframes are slot numbers, their
    std::map order is the slice's kf_rank.  Exact integers; AddConnection, the spanning tree and SetBadFlag stay with the caller."""
    _destroy = "orbx_covis_destroy"

    def __init__(self, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_covis_create.argtypes = [ci, ctypes.POINTER(vp)]
        L.orbx_covis_destroy.argtypes = [vp]
        L.orbx_covis_destroy.restype = None
        L.orbx_covis_update_connections.argtypes = [vp, ctypes.POINTER(CovisSlice), ci, ctypes.POINTER(CovisConnections)]
        L.orbx_covis_keyframe_culling.argtypes = [vp, ctypes.POINTER(CovisSlice), ctypes.POINTER(CovisCulling)]
        L.orbx_covis_last_timing.argtypes = [vp, vp, vp]
        self._h = vp()
        _check(L.orbx_covis_create(device, ctypes.byref(self._h)))

    def UpdateConnections(self, map_slice, th=15, counter_capacity=None, conn_capacity=None):
        """All lists of the slice in one call -> dict(counter_offset, conn_offset (Q+1); counter_kf, counter_weight: KFcounter in ascending rank;
        n_max, kf_max (Q); conn_kf, conn_weight: mvpOrderedConnectedKeyFrames / mvOrderedWeights).  The capacities default to the worst case."""
        keep = []
        S, a = covis_marshal(map_slice, keep)
        Q = S.num_lists
        worst = Q + min(Q * S.num_keyframes, int(np.diff(a["obs_offset"])[a["list_point"]].sum()) if S.num_entries and (a["list_point"] < S.num_points).all() and
                        (a["list_point"] >= 0).all() else 0)
        cc, nc = int(worst if counter_capacity is None else counter_capacity), int(worst if conn_capacity is None else conn_capacity)
        i4 = np.int32
        o = dict(counter_offset=np.zeros(Q + 1, i4), counter_kf=np.zeros(max(cc, 1), i4), counter_weight=np.zeros(max(cc, 1), i4), n_max=np.zeros(max(Q, 1), i4),
                 kf_max=np.zeros(max(Q, 1), i4), conn_offset=np.zeros(Q + 1, i4), conn_kf=np.zeros(max(nc, 1), i4), conn_weight=np.zeros(max(nc, 1), i4))
        R = CovisConnections(o["counter_offset"].ctypes.data, o["counter_kf"].ctypes.data, o["counter_weight"].ctypes.data, cc, o["n_max"].ctypes.data, o["kf_max"].ctypes.data,
                             o["conn_offset"].ctypes.data, o["conn_kf"].ctypes.data, o["conn_weight"].ctypes.data, nc)
        _check(self._L.orbx_covis_update_connections(self._h, ctypes.byref(S), int(th), ctypes.byref(R)))
        n, m = int(o["counter_offset"][Q]), int(o["conn_offset"][Q])
        for k in ("counter_kf", "counter_weight"):
            o[k] = o[k][:n]
        for k in ("conn_kf", "conn_weight"):
            o[k] = o[k][:m]
        o["n_max"], o["kf_max"] = o["n_max"][:Q], o["kf_max"][:Q]
        return o

    def UpdateLocalKeyFrames(self, map_slice):
        """The vote of Tracking::UpdateLocalKeyFrames: every list taken as a Frame's (list_kf = -1: no self-exclusion, bad keyframes are no candidates
        for kf_max) -> dict(counter_offset, counter_kf, counter_weight, n_max, kf_max)"""
        s = dict(map_slice)
        s["list_kf"] = np.full(len(np.ascontiguousarray(map_slice["list_kf"]).reshape(-1)), -1, np.int32)
        o = self.UpdateConnections(s)
        return {k: o[k] for k in ("counter_offset", "counter_kf", "counter_weight", "n_max", "kf_max")}

    def KeyFrameCulling(self, map_slice):
        """The lists are vpLocalKeyFrames in order -> dict(n_mps, n_redundant (Q) int32, culled (Q) uint8; point_bad (M) uint8 and point_obs (M) int32
        after the loop's erases)"""
        keep = []
        S, _ = covis_marshal(map_slice, keep)
        Q, M = S.num_lists, S.num_points
        o = dict(n_mps=np.zeros(max(Q, 1), np.int32), n_redundant=np.zeros(max(Q, 1), np.int32), culled=np.zeros(max(Q, 1), np.uint8), point_bad=np.zeros(max(M, 1), np.uint8),
                 point_obs=np.zeros(max(M, 1), np.int32))
        R = CovisCulling(*[o[k].ctypes.data for k in ("n_mps", "n_redundant", "culled", "point_bad", "point_obs")])
        _check(self._L.orbx_covis_keyframe_culling(self._h, ctypes.byref(S), ctypes.byref(R)))
        return dict(n_mps=o["n_mps"][:Q], n_redundant=o["n_redundant"][:Q], culled=o["culled"][:Q], point_bad=o["point_bad"][:M], point_obs=o["point_obs"][:M])

    def last_timing(self):
        """(device ms of the last call's chain, kernel launches)"""
        return self._timing("orbx_covis_last_timing", ctypes.c_float, ctypes.c_int)


class LoopSim3Problem(ctypes.Structure):
    _fields_ = [("num_keyframes", ctypes.c_int), ("tcw", ctypes.c_void_p), ("ow", ctypes.c_void_p), ("num_group", ctypes.c_int), ("current", ctypes.c_int),
                ("group_kf", ctypes.c_void_p), ("scw", ctypes.c_void_p), ("num_entries", ctypes.c_int), ("list_offset", ctypes.c_void_p), ("list_point", ctypes.c_void_p),
                ("num_points", ctypes.c_int), ("num_obs", ctypes.c_int), ("pos", ctypes.c_void_p), ("point_bad", ctypes.c_void_p), ("point_done", ctypes.c_void_p),
                ("point_ref", ctypes.c_void_p), ("ref_scale", ctypes.c_void_p), ("top_scale", ctypes.c_void_p), ("obs_offset", ctypes.c_void_p), ("obs_kf", ctypes.c_void_p)]


class LoopSim3Result(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("noncorrected", "corrected", "tiw", "ow_new", "scw_mat", "pos", "corrected_by", "normal", "max_dist", "min_dist", "updated")]


class LoopGbaProblem(ctypes.Structure):
    _fields_ = [("num_keyframes", ctypes.c_int), ("parent", ctypes.c_void_p), ("tcw", ctypes.c_void_p), ("tcw_gba", ctypes.c_void_p), ("in_gba", ctypes.c_void_p),
                ("num_points", ctypes.c_int), ("pos", ctypes.c_void_p), ("pos_gba", ctypes.c_void_p), ("point_in_gba", ctypes.c_void_p), ("point_bad", ctypes.c_void_p),
                ("point_ref", ctypes.c_void_p)]


class LoopGbaResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("tcw_gba", "reached", "pos", "moved")]


_LOOP_SIM3_ARRAYS = (("tcw", np.float32), ("ow", np.float32), ("group_kf", np.int32), ("scw", np.float64), ("list_offset", np.int32), ("list_point", np.int32),
                     ("pos", np.float32), ("point_bad", np.uint8), ("point_done", np.uint8), ("point_ref", np.int32), ("ref_scale", np.float32), ("top_scale", np.float32),
                     ("obs_offset", np.int32), ("obs_kf", np.int32))
_LOOP_GBA_ARRAYS = (("parent", np.int32), ("tcw", np.float32), ("tcw_gba", np.float32), ("in_gba", np.uint8), ("pos", np.float32), ("pos_gba", np.float32),
                    ("point_in_gba", np.uint8), ("point_bad", np.uint8), ("point_ref", np.int32))
LOOP_SIM3_FIELDS = (("noncorrected", np.float64, "G", 8), ("corrected", np.float64, "G", 8), ("tiw", np.float32, "G", 12), ("ow_new", np.float32, "G", 3),
                    ("scw_mat", np.float32, "G", 12), ("pos", np.float32, "M", 3), ("corrected_by", np.int32, "M", 1), ("normal", np.float32, "M", 3),
                    ("max_dist", np.float32, "M", 1), ("min_dist", np.float32, "M", 1), ("updated", np.uint8, "M", 1))
LOOP_GBA_FIELDS = (("tcw_gba", np.float32, "n", 12), ("reached", np.uint8, "n", 1), ("pos", np.float32, "M", 3), ("moved", np.uint8, "M", 1))


def loop_marshal(problem, keep):
    """orbx_loop_sim3_problem (a dict with "scw": the keys of _LOOP_SIM3_ARRAYS and "current") or orbx_loop_gba_problem (the keys of _LOOP_GBA_ARRAYS) of a
    dict of arrays -> (struct, arrays); the converted arrays are appended to `keep`, which must outlive the call"""
    sim3 = "scw" in problem
    a = {k: np.ascontiguousarray(problem[k], dt).reshape(-1) for k, dt in (_LOOP_SIM3_ARRAYS if sim3 else _LOOP_GBA_ARRAYS)}
    keep.append(a)
    p = {k: v.ctypes.data for k, v in a.items()}
    if sim3:
        NK, G, S, M, T = len(a["tcw"]) // 12, len(a["group_kf"]), len(a["list_point"]), len(a["point_bad"]), len(a["obs_kf"])
        if len(a["tcw"]) != 12 * NK or len(a["ow"]) != 3 * NK or len(a["scw"]) != 8 or len(a["list_offset"]) != G + 1 or len(a["pos"]) != 3 * M or len(a["obs_offset"]) != M + 1 or \
                any(len(a[k]) != M for k in ("point_done", "point_ref", "ref_scale", "top_scale")):
            raise ValueError("loop correction problem: array sizes do not agree")
        return LoopSim3Problem(NK, p["tcw"], p["ow"], G, int(problem["current"]), p["group_kf"], p["scw"], S, p["list_offset"], p["list_point"], M, T, p["pos"], p["point_bad"],
                               p["point_done"], p["point_ref"], p["ref_scale"], p["top_scale"], p["obs_offset"], p["obs_kf"]), a
    n, M = len(a["parent"]), len(a["point_bad"])
    if len(a["tcw"]) != 12 * n or len(a["tcw_gba"]) != 12 * n or len(a["in_gba"]) != n or len(a["pos"]) != 3 * M or len(a["pos_gba"]) != 3 * M or \
            len(a["point_in_gba"]) != M or len(a["point_ref"]) != M:
        raise ValueError("loop correction problem: array sizes do not agree")
    return LoopGbaProblem(n, p["parent"], p["tcw"], p["tcw_gba"], p["in_gba"], M, p["pos"], p["pos_gba"], p["point_in_gba"], p["point_bad"], p["point_ref"]), a


def _loop_outputs(fields, sizes):
    o = {k: np.zeros((max(sizes[s], 1), w) if w > 1 else max(sizes[s], 1), dt) for k, dt, s, w in fields}
    return o, (lambda: {k: o[k][:sizes[s]] for k, dt, s, w in fields})


class LoopCorrection(_Handle):
    """The two passes of the loop closer that move the map, on the device: CorrectLoop = the Sim3 propagation of LoopClosing::CorrectLoop (reference
    src/LoopClosing.cc:617-716: CorrectedSim3 / NonCorrectedSim3, every point of the group moved once by the first keyframe that reaches it, its
    UpdateNormalAndDepth, the SE3 poses), PropagateGBA = the map update after global BA (:930-1003: poses through the spanning tree, then every point).
    Keyframes are slot numbers; floats are bit for bit the reference's on the project's OpenCV stand-in.  Replace, AddObservation, UpdateConnections
    and the mutexes stay with the caller."""
    _destroy = "orbx_loop_destroy"

    def __init__(self, device=0):
        self._L = load_library()
        L = self._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.orbx_loop_create.argtypes = [ci, ctypes.POINTER(vp)]
        L.orbx_loop_destroy.argtypes = [vp]
        L.orbx_loop_destroy.restype = None
        L.orbx_loop_correct_sim3.argtypes = [vp, ctypes.POINTER(LoopSim3Problem), ctypes.POINTER(LoopSim3Result)]
        L.orbx_loop_propagate_gba.argtypes = [vp, ctypes.POINTER(LoopGbaProblem), ctypes.POINTER(LoopGbaResult)]
        L.orbx_loop_last_timing.argtypes = [vp, vp, vp]
        self._h = vp()
        _check(L.orbx_loop_create(device, ctypes.byref(self._h)))

    def CorrectLoop(self, problem):
        """problem: dict(tcw (NK,12), ow (NK,3), group_kf (G), current, scw (8), list_offset (G+1), list_point, pos (M,3), point_bad, point_done, point_ref,
        ref_scale, top_scale (M), obs_offset (M+1), obs_kf) -> dict(noncorrected, corrected (G,8) float64; tiw (G,12), ow_new (G,3), scw_mat (G,12); pos
        (M,3), corrected_by (M) int32 = the group position that moved the point or -1, normal (M,3), max_dist, min_dist, updated (M))"""
        keep = []
        P, _ = loop_marshal(problem, keep)
        if not isinstance(P, LoopSim3Problem):
            raise ValueError("CorrectLoop takes a Sim3 problem (with scw)")
        o, cut = _loop_outputs(LOOP_SIM3_FIELDS, dict(G=P.num_group, M=P.num_points))
        R = LoopSim3Result(*[o[k].ctypes.data for k, _, _, _ in LOOP_SIM3_FIELDS])
        _check(self._L.orbx_loop_correct_sim3(self._h, ctypes.byref(P), ctypes.byref(R)))
        return cut()

    def PropagateGBA(self, problem):
        """problem: dict(parent (n) slot / -1 origin / -2 outside the tree, tcw, tcw_gba (n,12), in_gba (n), pos, pos_gba (M,3), point_in_gba, point_bad (M),
        point_ref (M) slot or -1) -> dict(tcw_gba (n,12) completed, reached (n), pos (M,3), moved (M): 0 untouched, 1 mPosGBA, 2 re-projected)"""
        keep = []
        P, _ = loop_marshal(problem, keep)
        if not isinstance(P, LoopGbaProblem):
            raise ValueError("PropagateGBA takes a global BA problem (without scw)")
        o, cut = _loop_outputs(LOOP_GBA_FIELDS, dict(n=P.num_keyframes, M=P.num_points))
        R = LoopGbaResult(*[o[k].ctypes.data for k, _, _, _ in LOOP_GBA_FIELDS])
        _check(self._L.orbx_loop_propagate_gba(self._h, ctypes.byref(P), ctypes.byref(R)))
        return cut()

    def last_timing(self):
        """(device ms of the last call's launch chain, kernel launches)"""
        return self._timing("orbx_loop_last_timing", ctypes.c_float, ctypes.c_int)


# ------------------------------------------------------------------------------------------------
# Image front end: colour to grey and stereo rectification (csrc/orbx_image.hip)
# ------------------------------------------------------------------------------------------------
class ImagePrepConfig(ctypes.Structure):
    """orbx_image_prep_config (include/orbx.h)."""
    _fields_ = [("device", ctypes.c_int), ("max_width", ctypes.c_int), ("max_height", ctypes.c_int), ("max_batch", ctypes.c_int),
                ("gray_coef", ctypes.c_uint16 * 3), ("gray_shift", ctypes.c_uint16)]


GRAY_COEF_CV4 = ((9798, 19235, 3735), 15)      # R, G, B and the shift of OpenCV 4.x's 8-bit cvtColor (the default)
GRAY_COEF_CV3 = ((4899, 9617, 1868), 14)       # ... of OpenCV 3.x


def _bind_image_prep(L):
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.orbx_image_prep_create.argtypes = [ctypes.POINTER(ImagePrepConfig), ctypes.POINTER(vp)]
    L.orbx_image_prep_destroy.argtypes = [vp]
    L.orbx_image_prep_destroy.restype = None
    L.orbx_rectify_maps.argtypes = [vp, vp, ci, vp, vp, ci, ci, vp, vp]
    L.orbx_image_prep_set_maps.argtypes = [vp, ci, vp, vp, ci, ci, ci]
    L.orbx_image_prep_batch_device.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, sz, ci]
    L.orbx_image_prep_results_device.argtypes = [vp, vp, vp, vp]
    L.orbx_image_prep_sync.argtypes = [vp]
    L.orbx_image_prep_upload.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]
    L.orbx_image_prep_download.argtypes = [vp, ci, ci, ci, vp, ci]
    L.orbx_image_prep_run.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci]
    L.orbx_image_prep_last_timing.argtypes = [vp, vp, vp]
    return L


def rectify_maps(K, D, R, P, w, h):
    """cv::initUndistortRectifyMap(K, D, R, P[:3, :3], (w, h), CV_32FC1) -> (map_x, map_y), float32 (h, w): host code in double, no device
    (orbx_rectify_maps).  D = k1 k2 p1 p2 [k3]; P may be the 3 x 4 projection matrix of the calibration file."""
    L = _bind_image_prep(load_library())
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
    P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, -1)[:, :3])
    D = np.ascontiguousarray(np.asarray(D, np.float64).reshape(-1))
    mx, my = np.empty((max(h, 0), max(w, 0)), np.float32), np.empty((max(h, 0), max(w, 0)), np.float32)
    _check(L.orbx_rectify_maps(_ptr(K), _ptr(D), len(D), _ptr(R), _ptr(P), w, h, _ptr(mx), _ptr(my)))
    return mx, my


class ImagePrep(_Handle):
    """What the reference does to a camera image in front of ORBextractor::operator(), on the device: cvtColor to grey (Tracking::GrabImage*,
    src/Tracking.cc:250-278, 311-326, 369-384) and cv::remap through the maps of cv::initUndistortRectifyMap (Examples/Stereo/stereo_euroc.cc:124-134,
    181-188).  The grey, rectified frames land in a device buffer in the padded layout ORBextractor.run_device prefers.  Colour frames that are also
    rectified are converted to grey first, then remapped (one launch).  Parity with OpenCV is unpinned; tests/imgprep_ref.py restates the arithmetic."""
    _destroy = "orbx_image_prep_destroy"
    _keeps_pointer = True

    def __init__(self, max_width, max_height, max_batch, gray_coef=None, gray_shift=0, device=0):
        self._L = _bind_image_prep(load_library())
        cfg = ImagePrepConfig(device, max_width, max_height, max_batch)
        if gray_coef is not None:
            for i in range(3):
                cfg.gray_coef[i] = int(gray_coef[i])
        cfg.gray_shift = int(gray_shift)
        self._h = ctypes.c_void_p()
        _check(self._L.orbx_image_prep_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        self.max_batch = max_batch

    def set_maps(self, side, mx, my):
        """The two CV_32FC1 maps of `side` (0 left, 1 right), converted once to fixed point on the device."""
        mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
        if mx.ndim != 2 or mx.shape != my.shape:
            raise ValueError("set_maps: two float maps of one 2-d shape")
        _check(self._L.orbx_image_prep_set_maps(self._h, side, _ptr(mx), _ptr(my), mx.shape[1], mx.shape[1], mx.shape[0]))

    @staticmethod
    def _frames(images):
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        shp = imgs[0].shape
        if len(shp) not in (2, 3) or any(im.shape != shp for im in imgs):
            raise ValueError("frames of one shape (H, W) or (H, W, C)")
        return imgs, shp[1], shp[0], (1 if len(shp) == 2 else shp[2])

    def upload(self, images, dev_stride=0, dev_offset=0):
        """Host frames (H, W) or (H, W, C) into the handle's device source buffer -> (pointer, stride, pitch, (B, W, H, C))"""
        imgs, W, H, C = self._frames(images)
        arr = (ctypes.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        dev, st, fp = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_size_t()
        _check(self._L.orbx_image_prep_upload(self._h, arr, len(imgs), W, H, C, W * C, dev_stride, dev_offset, ctypes.byref(dev), ctypes.byref(st), ctypes.byref(fp)))
        return dev, st.value, fp.value, (len(imgs), W, H, C)

    def run_device(self, ext, src, stride, pitch, shape, rgb=True, rectify=None):
        """Enqueue one batch on `ext`'s stream (None: the handle's own); nothing is waited for.  Follow it with
        ext.run_device(*prep.results_device(), (B, W, H)): the extraction is ordered behind it."""
        B, W, H, C = shape
        _check(self._L.orbx_image_prep_batch_device(self._h, ext._h if ext is not None else None, src, B, W, H, C, 1 if rgb else 0, stride, pitch,
                                                    -1 if rectify is None else int(rectify)))

    def results_device(self):
        """(device pointer, stride, frame pitch) of the last batch's grey frames"""
        dev, st, fp = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_size_t()
        _check(self._L.orbx_image_prep_results_device(self._h, ctypes.byref(dev), ctypes.byref(st), ctypes.byref(fp)))
        return dev, st.value, fp.value

    def sync(self):
        _check(self._L.orbx_image_prep_sync(self._h))

    def download(self, batch, width, height):
        """Wait for the last batch and return its grey frames (batch, height, width) without their padding"""
        out = np.empty((batch, height, width), np.uint8)
        _check(self._L.orbx_image_prep_download(self._h, batch, width, height, _ptr(out), width))
        return out

    def run(self, images, rgb=True, rectify=None):
        """The synchronous form: frames (H, W) or (H, W, 3 / 4) uint8 -> grey (B, H, W) uint8"""
        imgs, W, H, C = self._frames(images)
        arr = (ctypes.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        out = np.empty((len(imgs), H, W), np.uint8)
        _check(self._L.orbx_image_prep_run(self._h, arr, len(imgs), W, H, C, 1 if rgb else 0, W * C, -1 if rectify is None else int(rectify), _ptr(out), W))
        return out

    def last_timing(self):
        """(device ms of the last call's kernel, kernel launches)"""
        return self._timing("orbx_image_prep_last_timing", ctypes.c_float, ctypes.c_int)
