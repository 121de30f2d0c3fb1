"""The image front end (csrc/orbx_image.hip): colour to grey and stereo rectification in front of the extractor.

CPU: the numpy restatement (tests/imgprep_ref.py) checks itself, orbx_rectify_maps equals it bit for bit, the ABI refuses bad arguments
without a device, the shim compiles against the reference headers.  GPU: every comparison is exact (== on bytes)."""
import ctypes
import functools
import os
import subprocess
import tempfile
import threading
from pathlib import Path

import numpy as np
import pytest

import imgprep_ref as ref

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
ERR_ARG, ERR_NODEVICE, ERR_STATE = -1, -4, -5
COEFS = {"cv4": ref.GRAY_CV4, "cv3": ref.GRAY_CV3}


def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def _euroc():
    z = np.load(ROOT / "tests" / "golden" / "imgprep" / "euroc_rectify.npz")
    return {k: z[k] for k in z.files}


def _euroc_side(side):
    e = _euroc()
    return e[side + "_K"], e[side + "_D"], e[side + "_R"], e[side + "_P"], int(e["width"]), int(e["height"])


@functools.lru_cache(maxsize=None)
def _euroc_maps(side):
    """the restatement's EuRoC maps, computed once and shared (read-only)"""
    mx, my = ref.rectify_maps(*_euroc_side(side))
    mx.setflags(write=False); my.setflags(write=False)
    return mx, my


# ---------------------------------------------------------------------------------------------------------------------
# the restatement checks itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COEFS))
def test_gray_formula_is_within_one_level_of_the_float_weights(name):
    """all 2^24 triples against round(0.299 R + 0.587 G + 0.114 B) in float64"""
    coef, shift = COEFS[name]
    assert sum(coef) == 1 << shift
    i = np.arange(1 << 24, dtype=np.uint32)
    r, g, b = i >> 16, (i >> 8) & 255, i & 255
    got = ref.gray_rgb(r, g, b, coef, shift).astype(np.int32)
    want = np.rint(0.299 * r.astype(np.float64) + 0.587 * g + 0.114 * b).astype(np.int32)
    assert np.abs(got - want).max() <= 1
    assert (ref.gray_rgb(i & 255, i & 255, i & 255, coef, shift)[:256] == np.arange(256)).all()      # grey stays grey


def test_remap_table_form_equals_the_short_form_for_all_phases():
    """OpenCV's literal form - 16-bit weights saturate_short(w * 32768), (sum + 16384) >> 15 - with and without the sum fix-up on any of the
    four entries, against ((32 - fx)(32 - fy) p00 + ... + 512) >> 10: all 1024 phases, the 16 extreme tap sets and random taps"""
    rng = np.random.default_rng(7)
    ext = np.array([[(k >> j & 1) * 255 for j in range(4)] for k in range(16)], np.int64)
    taps = np.concatenate([ext, rng.integers(0, 256, (240, 4))]).astype(np.int64)      # (256, 4)
    fy, fx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    fy, fx = fy.reshape(-1, 1), fx.reshape(-1, 1)                                        # (1024, 1) against (256,) taps
    p = [taps[:, k][None, :] for k in range(4)]
    short = ref.blend_short(*p, fx, fy)
    assert short.min() == 0 and short.max() == 255
    for fixup in (None, 0, 1, 2, 3):
        tab = ref.remap_table(fixup)
        assert tab.shape == (32, 32, 4) and (fixup is None or (tab.sum(-1) == 32768).all())
        assert (ref.blend_table(*p, fx, fy, tab) == short).all(), fixup


def test_remap_identity_and_integer_shift():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (19, 37), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(19, dtype=np.float32), np.arange(37, dtype=np.float32), indexing="ij")
    assert (ref.remap(src, xx, yy) == src).all()
    for dx, dy in ((3, 2), (-4, 1), (0, -5), (40, 0)):
        want = np.zeros_like(src)
        ys, xs = np.arange(19) + dy, np.arange(37) + dx
        oky, okx = (ys >= 0) & (ys < 19), (xs >= 0) & (xs < 37)
        want[np.ix_(oky, okx)] = src[np.ix_(ys[oky], xs[okx])]
        assert (ref.remap(src, xx + dx, yy + dy) == want).all(), (dx, dy)


def test_maps_fixed_rounds_half_to_even_and_saturates():
    m = np.array([0.0, 1 / 64, 1 / 32 + 1 / 64, -1 / 64, -2.5, -1 / 32, 40000.25, -40000.25, 3e38, -3e38], np.float32)
    ix, _, fx, _ = ref.maps_fixed(m, m)
    assert list(ix) == [0, 0, 0, 0, -3, -1, 32767, -32768, 32767, -32768]
    assert list(fx) == [0, 0, 2, 0, 16, 31, 8, 24, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# orbx_rectify_maps: host code in double, bit-equal to the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize("side", ["left", "right"])
def test_rectify_maps_euroc_bit_equal(orbx, side):
    K, D, R, P, w, h = _euroc_side(side)
    mx, my = orbx.rectify_maps(K, D, R, P, w, h)
    wx, wy = _euroc_maps(side)
    assert mx.shape == (h, w) and _same_bits(mx, wx) and _same_bits(my, wy)
    mx4, my4 = orbx.rectify_maps(K, D[:4], R, P, w, h)      # k3 = 0 in the file: four coefficients give the same maps
    assert _same_bits(mx4, wx) and _same_bits(my4, wy)


def test_rectify_maps_distorted_and_tiny_bit_equal(orbx):
    K = [300.0, 0, 161.3, 0, 310.0, 118.9, 0, 0, 1]
    D = [-0.45, 0.31, 0.004, -0.003, -0.12]
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, np.cos(0.03), -np.sin(0.03)], [0, np.sin(0.03), np.cos(0.03)]])
    P = [280.0, 0, 158.0, 0, 285.0, 121.0, 0, 0, 1]
    for w, h, d in ((320, 240, D), (5, 3, D), (5, 3, D[:4]), (1, 1, D), (1, 7, D)):
        got, want = orbx.rectify_maps(K, d, R, P, w, h), ref.rectify_maps(K, d, R, P, w, h)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), (w, h)
    assert np.abs(ref.rectify_maps(K, D, R, P, 320, 240)[0] - ref.rectify_maps(K, [0] * 4, R, P, 320, 240)[0]).max() > 5      # the distortion matters


@pytest.mark.parametrize("side", ["left", "right"])
def test_rectify_maps_sanity(orbx, side):
    """D = 0, R = I, Pnew = K: the pixel grid within 1e-4; the EuRoC maps: the forward distortion model in float64 on the back-projected grid within 1e-3 px"""
    K, D, R, P, w, h = _euroc_side(side)
    mx, my = orbx.rectify_maps(K, [0] * 5, np.eye(3), K, w, h)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.abs(mx - xx).max() <= 1e-4 and np.abs(my - yy).max() <= 1e-4
    mx, my = orbx.rectify_maps(K, D, R, P, w, h)
    fx, fy = ref.distort_forward(K, D, R, P, w, h)
    assert np.abs(mx - fx).max() <= 1e-3 and np.abs(my - fy).max() <= 1e-3
    assert np.abs(mx - xx).max() > 3      # (these maps move pixels)


def test_rectify_maps_refuses_bad_arguments(orbx):
    K, D, R, P, w, h = _euroc_side("left")
    for bad in (lambda: orbx.rectify_maps(K, D[:3], R, P, w, h), lambda: orbx.rectify_maps(K, D, R, P, 0, h), lambda: orbx.rectify_maps(K, D, R, P, w, -1),
                lambda: orbx.rectify_maps(K, D, np.zeros((3, 3)), P, w, h)):
        with pytest.raises(orbx.OrbxError) as e:
            bad()
        assert e.value.code == ERR_ARG
    L = orbx.load_library()
    L.orbx_rectify_maps.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2
    assert L.orbx_rectify_maps(None, None, 5, None, None, 4, 4, None, None) == ERR_ARG and b"NULL" in L.orbx_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_the_front_end_is_built_into_the_library(orbx):
    assert "orbx_image.hip" in orbx.build_mod.HIP_SOURCES
    L = orbx.load_library()
    assert all(hasattr(L, n) for n in ("orbx_image_prep_create", "orbx_image_prep_batch_device", "orbx_image_prep_run", "orbx_rectify_maps"))


def test_abi_refuses_bad_arguments_without_a_device(orbx):
    L = orbx.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    none = vp(None)
    h = vp()
    # bad configurations are refused before a device is looked for
    for cfg in (orbx.ImagePrepConfig(0, 640, 480, 1, (1, 2, 3), 15), orbx.ImagePrepConfig(0, 640, 480, 1, (9798, 19235, 3735), 14),
                orbx.ImagePrepConfig(0, 640, 480, 1, (64, 64, 0), 7), orbx.ImagePrepConfig(0, 640, 480, 1, (0, 0, 0), 15), orbx.ImagePrepConfig(0, 0, 480, 1),
                orbx.ImagePrepConfig(0, 640, 20000, 1), orbx.ImagePrepConfig(0, 640, 480, 0)):
        L.orbx_image_prep_create.argtypes = [vp, vp]
        assert L.orbx_image_prep_create(ctypes.byref(cfg), ctypes.byref(h)) == ERR_ARG and len(L.orbx_last_error()) > 0 and not h.value
    assert L.orbx_image_prep_create(None, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_image_prep_create(ctypes.byref(orbx.ImagePrepConfig(0, 640, 480, 1)), None) == ERR_ARG
    if not _has_gpu():
        for coef, shift in ((None, 0),) + tuple(COEFS.values()):
            with pytest.raises(orbx.OrbxError) as e:
                orbx.ImagePrep(640, 480, 2, coef, shift)
            assert e.value.code == ERR_NODEVICE
    img = np.zeros((4, 4), np.uint8)
    one = (vp * 1)(img.ctypes.data)
    calls = [
        (L.orbx_image_prep_set_maps, [none, 0, none, none, 4, 4, 4]),
        (L.orbx_image_prep_batch_device, [none, none, none, 1, 4, 4, 1, 1, 4, ctypes.c_size_t(16), -1]),
        (L.orbx_image_prep_results_device, [none, none, none, none]),
        (L.orbx_image_prep_sync, [none]),
        (L.orbx_image_prep_upload, [none, one, 1, 4, 4, 1, 4, 0, 0, none, none, none]),
        (L.orbx_image_prep_download, [none, 1, 4, 4, none, 4]),
        (L.orbx_image_prep_run, [none, one, 1, 4, 4, 1, 1, 4, -1, none, 4]),
        (L.orbx_image_prep_last_timing, [none, none, none]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        fn.argtypes = None
        assert fn(*args) == ERR_ARG, fn.__name__
        assert len(L.orbx_last_error()) > 0
    # set_maps checks the maps before it looks at the handle: NaN / infinity are refused here too
    L.orbx_image_prep_set_maps.argtypes = [vp, ci, vp, vp, ci, ci, ci]
    good = np.zeros((4, 6), np.float32)
    for bad in (np.nan, np.inf):
        m = good.copy()
        m[2, 3] = bad
        for a, b in ((m, good), (good, m)):
            assert L.orbx_image_prep_set_maps(None, 0, a.ctypes.data, b.ctypes.data, 6, 6, 4) == ERR_ARG and b"(3, 2) is not finite" in L.orbx_last_error()
    assert L.orbx_image_prep_set_maps(None, 0, good.ctypes.data, good.ctypes.data, 6, 6, 4) == ERR_ARG and b"NULL handle" in L.orbx_last_error()
    assert L.orbx_image_prep_set_maps(None, 0, good.ctypes.data, good.ctypes.data, 5, 6, 4) == ERR_ARG and b"bad size" in L.orbx_last_error()
    L.orbx_image_prep_destroy.argtypes = [vp]
    L.orbx_image_prep_destroy.restype = None
    L.orbx_image_prep_destroy(None)


@pytest.mark.gpu
def test_handle_refuses_bad_arguments(orbx):
    p = _prep("cv4")
    yy, xx = np.meshgrid(np.arange(8, dtype=np.float32), np.arange(12, dtype=np.float32), indexing="ij")
    for bad in (np.nan, np.inf, -np.inf):
        m = xx.copy()
        m[5, 7] = bad
        for a, b in ((m, yy), (xx, m)):
            with pytest.raises(orbx.OrbxError) as e:
                p.set_maps(0, a, b)
            assert e.value.code == ERR_ARG and "(7, 5)" in str(e.value)
    with pytest.raises(orbx.OrbxError) as e:
        p.set_maps(2, xx, yy)
    assert e.value.code == ERR_ARG
    with pytest.raises(orbx.OrbxError) as e:
        p.set_maps(0, np.zeros((8, 2000), np.float32), np.zeros((8, 2000), np.float32))
    assert e.value.code == ERR_ARG
    fresh = orbx.ImagePrep(64, 64, 2)
    with pytest.raises(orbx.OrbxError) as e:
        fresh.results_device()
    assert e.value.code == ERR_STATE
    img = np.zeros((8, 12, 3), np.uint8)
    with pytest.raises(orbx.OrbxError) as e:
        fresh.run([img], rectify=1)      # no maps for that side
    assert e.value.code == ERR_STATE
    fresh.set_maps(1, xx, yy)
    with pytest.raises(orbx.OrbxError) as e:
        fresh.run([np.zeros((8, 16, 3), np.uint8)], rectify=1)      # maps of another size
    assert e.value.code == ERR_ARG
    for frames in ([img] * 3, [np.zeros((8, 12, 2), np.uint8)], [np.zeros((8, 80), np.uint8)]):
        with pytest.raises(orbx.OrbxError) as e:
            fresh.run(frames)
        assert e.value.code == ERR_ARG
    assert (fresh.run([img + 7], rectify=1) == 7).all()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# the shim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.access(REF / "include" / "Tracking.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-include", str(REF / "include" / "Tracking.h"), "-I" + str(ROOT / "include"), "-fsyntax-only", str(shim / "GrabImage_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_makes_the_calls_it_claims_and_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "GrabImage_hip.cc").read_text()
    for piece in ("orbx_image_prep_create(", "orbx_image_prep_run(", "orbx_image_prep_set_maps(", "orbx_rectify_maps(", "orbx_image_prep_destroy(", "shim_error.h", "orbx_shim::Fail("):
        assert piece in text, piece
    head = (shim / "GrabImage_hip.h").read_text()
    for piece in ("cv::Mat ToGray(const cv::Mat &im, bool bRGB)", "class StereoRectifier", "operator()(const cv::Mat &imLeft, const cv::Mat &imRight, cv::Mat &imLeftRect, cv::Mat &imRightRect)"):
        assert piece in head, piece
    assert "GrabImage_hip" not in (ROOT / "oracle" / "Makefile").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    for piece in ("GrabImage_hip", "ToGray(", "StereoRectifier", "stereo_euroc.cc", "orbx_image_prep_batch_device"):
        assert piece in integ, piece


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prep(name):
    coef, shift = COEFS[name]
    return _orbx().ImagePrep(1024, 1024, 16, coef, shift)


def _device(p, frames, rgb=True, rectify=None, dev_stride=0, dev_offset=0, full_rows=False):
    """upload + device form + download; full_rows: the rows with their padding (stride bytes)"""
    src, ss, sp, shape = p.upload(frames, dev_stride, dev_offset)
    p.run_device(None, src, ss, sp, shape, rgb, rectify)
    _, st, fp = p.results_device()
    B, W, H, _ = shape
    assert st % 4 == 0 and st >= (W + 3) // 4 * 4 + 12 and fp == st * H
    out = p.download(B, st, H)
    assert (out[:, :, W:] == 0).all(), "pad bytes must be 0"
    return out if full_rows else out[:, :, :W]


@functools.lru_cache(maxsize=None)
def _all_triples():
    """every (R, G, B) once: 16 frames of 1024 x 1024 - (r, g, b) planes, read-only"""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(16, 1024, 1024)
    planes = tuple(a.astype(np.uint8) for a in (i >> 16, (i >> 8) & 255, i & 255))
    for a in planes:
        a.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def _all_triples_gray(name):
    g = ref.gray_rgb(*_all_triples(), *COEFS[name])
    g.setflags(write=False)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COEFS))
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("rgb", [True, False])
def test_gray_exhaustive(orbx, name, channels, rgb):
    r, g, b = _all_triples()
    planes = [r, g, b] if rgb else [b, g, r]
    if channels == 4:
        planes.append(np.random.default_rng(11).integers(0, 256, r.shape, dtype=np.uint8))      # alpha is ignored
    frames = np.stack(planes, -1)
    got = _device(_prep(name), list(frames), rgb)
    assert (got == _all_triples_gray(name)).all()
    ms, launches = _prep(name).last_timing()
    assert launches == 1 and ms > 0


def _colour(rng, h, w, c):
    return rng.integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("shape", [(37, 19), (4, 1), (1, 1), (641, 5), (64, 17), (260, 33)])
def test_gray_small_shapes_strides_and_offsets(orbx, channels, shape):
    """odd sizes, one pixel, more than one block in x and y; per shape: the aligned path, a tight source stride (641 * 3 is no multiple of 4: the byte
    path), a source stride larger than the row, a source pointer off by 1 and by 3 bytes; batches of 1 and 3; RGB and BGR"""
    w, h = shape
    rng = np.random.default_rng(w * 100 + h + channels)
    p = _prep("cv4")
    frames = [_colour(rng, h, w, channels) for _ in range(3)]
    for rgb in (True, False):
        want = np.stack([ref.gray(f, rgb) for f in frames])
        for kw in (dict(), dict(dev_stride=w * channels), dict(dev_stride=w * channels + 4), dict(dev_stride=w * channels + 7), dict(dev_offset=1), dict(dev_offset=3),
                   dict(dev_stride=w * channels + 8, dev_offset=2)):
            assert (_device(p, frames, rgb, **kw) == want).all(), (rgb, kw)
        assert (_device(p, frames[:1], rgb) == want[:1]).all()
    assert (p.run(frames, rgb=False) == want).all()


def _hand_maps(w, h):
    """maps of the image's own size whose rows walk through what the fixed-point form can get wrong"""
    rng = np.random.default_rng(5)
    mx = rng.uniform(-3, w + 2, (h, w)).astype(np.float32)      # everything not set below: random, some of it outside
    my = rng.uniform(-3, h + 2, (h, w)).astype(np.float32)
    c, r = np.arange(32, dtype=np.float32), np.arange(32, dtype=np.float32)[:, None]
    mx[:32, :32] = 10 + c + c / 32                               # a 32 x 32 grid: every (fx, fy) phase once
    my[:32, :32] = 5 + r + r / 32
    j = np.arange(32, dtype=np.float32)
    mx[32, :32] = 7 + j / 32 + 1 / 64                             # exactly on a rounding tie: 32 k + j + 0.5, j even and odd
    my[32, :32] = 3 + j[::-1] / 32 + 1 / 64
    mx[33, :32] = -(j / 32 + 1 / 64)                              # ... and the negative ties
    my[33, :32] = 2.5
    n = min(w, 161)
    neg = (-2.5 + np.arange(n, dtype=np.float32) / 64)[:n]        # -2.5 .. 0 in steps of 1 / 64: arithmetic shift and mask on negatives
    mx[34, :n] = neg
    my[34, :n] = 1.25
    mx[35, :n] = 4.75
    my[35, :n] = neg
    # taps one pixel outside at the four edges and the four corners, with fractions
    edge_x = np.array([-1, -0.5, -1 / 32, w - 1, w - 1 + 0.25, w - 1 + 31 / 32, 10.5, 10.5, 10.5, 10.5], np.float32)
    edge_y = np.array([8.25, 8.25, 8.25, 8.25, 8.25, 8.25, -1, -0.75, h - 1, h - 1 + 0.5], np.float32)
    mx[36, :10], my[36, :10] = edge_x, edge_y
    cx = np.array([-0.5, w - 0.5, -0.5, w - 0.5, -1, w - 1, -1, w - 1], np.float32)
    cy = np.array([-0.5, -0.5, h - 0.5, h - 0.5, -1, -1, h - 1, h - 1], np.float32)
    mx[36, 10:18], my[36, 10:18] = cx, cy
    # fully outside (expected 0) and beyond +-32768 (saturation)
    mx[37, :8] = [-5, w + 3, 5, 5, -40000.25, 40000.25, 1e9, -3e38]
    my[37, :8] = [5, 5, -5, h + 3, 5, 5, 5, 5]
    mx[38, :8] = [5, 5, 5, 5, 40000.5, -40000.5, -1e9, 3e38]
    my[38, :8] = [-40000.25, 40000.25, 1e9, -3e38, 40000.5, -40000.5, -1e9, 3e38]
    mx[39, :], my[39, :] = -2, -2                                 # a whole row outside
    return mx, my


def _checker_frames(w, h):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    chk = (((xx + yy) & 1) * 255).astype(np.uint8)
    rng = np.random.default_rng(9)
    return [chk, rng.integers(0, 256, (h, w), dtype=np.uint8), 255 - chk, np.full((h, w), 255, np.uint8)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(96, 64), (93, 64), (65, 41)])
def test_remap_hand_made_maps(orbx, size):
    """every phase, rounding ties, negative coordinates, taps outside at every edge and corner, fully outside, saturation, a width that is no multiple
    of 4; 0 / 255 checkerboards (the largest sum) and random bytes"""
    w, h = size
    mx, my = _hand_maps(w, h)
    frames = _checker_frames(w, h)
    p = _prep("cv4")
    p.set_maps(0, mx, my)
    want = np.stack([ref.remap(f, mx, my) for f in frames])
    assert (want[:, 37, :8] == 0).all() and (want[:, 38, :8] == 0).all() and (want[:, 39] == 0).all() and want[3].max() == 255 and (want[1] > 0).mean() > 0.5
    assert (_device(p, frames, rectify=0) == want).all()
    assert (_device(p, frames, rectify=0, dev_stride=w + 3, dev_offset=1) == want).all()
    assert (p.run(frames[:1], rectify=0) == want[:1]).all()
    # colour + rectify in one call = the restatement's grey conversion, then its remap
    rng = np.random.default_rng(w)
    for c in (3, 4):
        col = [_colour(rng, h, w, c) for _ in range(2)]
        for rgb in (True, False):
            wantc = np.stack([ref.prep(f, rgb, maps=(mx, my)) for f in col])
            assert (_device(p, col, rgb, rectify=0) == wantc).all(), (c, rgb)
            assert (_device(p, col, rgb, rectify=0, dev_stride=w * c + 5, dev_offset=3) == wantc).all(), (c, rgb)
    colcv3 = np.stack([ref.prep(f, True, *COEFS["cv3"], maps=(mx, my)) for f in col])
    _prep("cv3").set_maps(1, mx, my)
    assert (_device(_prep("cv3"), col, True, rectify=1) == colcv3).all()


@functools.lru_cache(maxsize=None)
def _euroc_frames():
    orbx = _orbx()
    fr = tuple(orbx.synth_frame(20 + i, 752, 480, orbx.SYNTH_STEREO_RIGHT if i & 1 else 0) for i in range(4))
    for f in fr:
        f.setflags(write=False)
    return fr


@pytest.mark.gpu
def test_remap_euroc_maps_left_then_right(orbx):
    """the maps of orbx_rectify_maps on synthetic 752 x 480 frames: a batch of 4 through the left maps, then a batch of 4 through the right maps, one handle"""
    p = _prep("cv4")
    frames = list(_euroc_frames())
    for s, side in enumerate(("left", "right")):
        mx, my = orbx.rectify_maps(*_euroc_side(side))
        assert _same_bits(mx, _euroc_maps(side)[0])
        p.set_maps(s, mx, my)
    for s, side in enumerate(("left", "right")):
        want = np.stack([ref.remap(f, *_euroc_maps(side)) for f in frames])
        got = _device(p, frames, rectify=s)
        assert (got == want).all(), side
        assert (got != np.stack(frames)).mean() > 0.3      # (the maps move the image)


def _rgb_frames(orbx, seed, n, w, h):
    """colour frames whose channels differ: three synthetic views of one scene as R, G, B"""
    return [np.stack([orbx.synth_frame(seed + i, w, h, 0, v, 5 * v, 3 * v) for v in range(3)], -1) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["640x480", "752x480_rectified"])
def test_end_to_end_prep_then_extract_without_a_wait(orbx, case):
    """ImagePrep.run_device(ext, rgb frames) followed by ext.run_device(prep output): keypoints, descriptors and counts bit-equal to extracting the
    restatement's grey image through orbx_upload_frames - the layout contract, the pad bytes and the stream ordering in one"""
    w, h, nf, rect = (640, 480, 1000, None) if case == "640x480" else (752, 480, 1200, 0)
    B = 3
    frames = _rgb_frames(orbx, 40, B, w, h)
    maps = _euroc_maps("left") if rect is not None else None
    gray = [ref.prep(f, True, maps=maps) for f in frames]
    for f, g in zip(frames, ref.gray(np.stack(frames))):      # vacuity guard: the grey image is none of the channels
        assert all((g != f[..., c]).mean() > 0.5 for c in range(3))
    ext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    ext.run_device(*ext.upload(gray))
    want = ext.download(B)
    assert want[2].min() > 100
    p = _prep("cv4")
    if rect is not None:
        p.set_maps(0, *maps)
    src, ss, sp, shape = p.upload(frames)
    p.run_device(ext, src, ss, sp, shape, True, rect)
    dev, st, fp = p.results_device()
    ext.run_device(dev, st, fp, (B, w, h))
    got = ext.download(B)
    assert (got[2] == want[2]).all()
    for f in range(B):
        n = int(want[2][f])
        assert got[0][f, :n].tobytes() == want[0][f, :n].tobytes() and (got[1][f, :n] == want[1][f, :n]).all()
    assert (p.download(B, w, h) == np.stack(gray)).all()


@pytest.mark.gpu
def test_host_form_equals_device_form_and_two_handles_on_two_threads(orbx):
    rng = np.random.default_rng(21)
    frames = [_colour(rng, 120, 203, 3) for _ in range(3)]
    mx, my = _hand_maps(203, 120)
    want = np.stack([ref.prep(f, False, maps=(mx, my)) for f in frames])
    p = _prep("cv4")
    p.set_maps(0, mx, my)
    assert (_device(p, frames, False, 0) == want).all() and (p.run(frames, rgb=False, rectify=0) == want).all()
    out = [None, None]

    def work(i):
        q = orbx.ImagePrep(256, 128, 3)
        q.set_maps(i, mx, my)
        res = [q.run(frames, rgb=False, rectify=i) for _ in range(4)]
        out[i] = res
        q.close()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert all(o is not None and all((r == want).all() for r in o) for o in out)
