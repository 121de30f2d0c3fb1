"""The RGB-D frame path: orbx_frame_rgbd_device / _begin / _end == Frame::ComputeStereoFromRGBD (reference src/Frame.cc:1423-1461) + the
depth order, Frame::UnprojectStereo's camera-frame points (:1478-1491) and the close-point count the tracker derives from mvDepth.

Expected values: mvKeys / mvKeysUn of the COMPILED reference (oracle_lib.ref_mono_frame: the RGB-D constructor extracts and undistorts like
the monocular one) + tests/rgbd_ref.py's one-operation-per-call numpy restatement of the few lines behind no export; recorded for one frame in
tests/golden/slam/rgbd_tum_640x480_1000.npz (tools/gen_golden_rgbd.py).  Device results must equal them bit for bit."""
import ctypes
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import rgbd_ref

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "slam" / "rgbd_tum_640x480_1000.npz"
needs_ref = pytest.mark.skipif(oracle_lib.slam_lib() is None, reason="oracle/_ref/liborbslam.so not built (needs the reference sources)")

# camera, W, H, nfeatures: a distorted and an undistorted camera at each size
CASES = [("tum1", 640, 480, 1000), ("tum3", 640, 480, 1000), ("euroc", 752, 480, 1200), ("euroc_rect", 752, 480, 1200)]
SEEDS = list(range(61, 69))      # B = 8 different frames


def load_golden():
    """the fixture as tools/gen_golden_rgbd.py recorded it -> (z, {"u16": want, "f32": want})"""
    z = np.load(GOLDEN)
    u = dict(depth=z["u16_depth"], u_right=z["u16_u_right"], order=z["u16_order"].astype(np.int32), n_valid=int(z["u16_n_valid"]), n_close=int(z["u16_n_close"]))
    u["xyz_cam"] = np.stack([z["u16_xyz_cam"][0], z["u16_xyz_cam"][1], np.where(u["depth"] > 0, u["depth"], np.float32(0))], 1).astype(np.float32)
    f = dict(depth=u["depth"].copy(), u_right=u["u_right"].copy(), xyz_cam=u["xyz_cam"].copy(), order=z["f32_order"].astype(np.int32),
             n_valid=int(z["f32_n_valid"]), n_close=int(z["f32_n_close"]))
    d = z["f32_diff"]
    f["depth"][d], f["u_right"][d], f["xyz_cam"][d] = z["f32_depth"], z["f32_u_right"], z["f32_xyz_cam"]
    return z, {"u16": u, "f32": f}


def golden_images(z):
    W, H, seed = int(z["W"]), int(z["H"]), int(z["seed"])
    raw = rgbd_ref.depth_raw(seed, W, H)
    img, special = rgbd_ref.depth_f32(raw, z["kps"])
    assert np.array_equal(np.asarray(special, np.int32), z["special"])
    return rgbd_ref.gray_frame(seed, W, H), raw, img, special


def images_of(fmt, seed, W, H, kps):
    """(depth image, factor, planted pixels or None)"""
    raw = rgbd_ref.depth_raw(seed, W, H)
    if fmt == "u16":
        return raw, rgbd_ref.U16_FACTOR, None
    img, special = rgbd_ref.depth_f32(raw, kps)
    return img, np.float32(1.0), special


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_smaller_than_the_mono_golden():
    assert GOLDEN.stat().st_size < (GOLDEN.parent / "mono_tum1_640x480_1000.npz").stat().st_size


@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_restatement_matches_fixture(fmt):
    z, want = load_golden()
    _, raw, img, special = golden_images(z)
    image, factor = (raw, z["u16_factor"]) if fmt == "u16" else (img, None)
    d = rgbd_ref.lookup(image, z["kps"], factor)
    got = rgbd_ref.restate(d, z["kpsUn"], z["cam"], z["bf"], z["th_depth"])
    rgbd_ref.assert_same(got, want[fmt])
    rgbd_ref.check_inputs(z["kps"], d, want[fmt], special if fmt == "f32" else None, image)
    assert rgbd_ref.same_bits(np.float32(z["th_depth"]), rgbd_ref.th_depth(z["cam"][0]))
    # truncation, not rounding: rounding the coordinates reads other pixels and gives other depths
    rounded = rgbd_ref.lookup(image, np.round(z["kps"]), factor)
    assert np.count_nonzero(rounded.view(np.uint32) != d.view(np.uint32)) >= 20


@needs_ref
def test_fixture_keypoints_are_the_compiled_reference(orbx):
    z, _ = load_golden()
    gray = golden_images(z)[0]
    ref = oracle_lib.ref_mono_frame(gray, int(z["nfeatures"]), *[float(v) for v in z["cam"]], z["dist"])
    assert rgbd_ref.same_bits(ref["kps"][:, :2].copy(), z["kps"]) and rgbd_ref.same_bits(ref["kpsUn"][:, :2].copy(), z["kpsUn"])


def _reference_case(cam, W, H, nf, fmt, seeds):
    """per frame: (gray, depth image, factor, reference mvKeys xy, expected results), the input conditions checked on the reference's values"""
    K, dist = rgbd_ref.CAMS[cam]
    thd = rgbd_ref.th_depth(K[0])
    out = []
    for s in seeds:
        gray = rgbd_ref.gray_frame(s, W, H)
        ref = oracle_lib.ref_mono_frame(gray, nf, K[0], K[1], K[2], K[3], dist)
        kps, un = ref["kps"][:, :2].copy(), ref["kpsUn"][:, :2].copy()
        image, factor, special = images_of(fmt, s, W, H, kps)
        d = rgbd_ref.lookup(image, kps, factor)
        want = rgbd_ref.restate(d, un, np.asarray(K, np.float32), rgbd_ref.BF, thd)
        rgbd_ref.check_inputs(kps, d, want, special, image)
        assert (float(dist[0]) != 0.0) == (np.abs(un - kps).max() > 0.5)      # the distorted camera does move the points
        out.append((gray, image, factor, kps, want))
    return out


@needs_ref
@pytest.mark.parametrize("cam,W,H,nf", CASES)
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_inputs_meet_the_conditions(cam, W, H, nf, fmt):
    """every frame the GPU tests run: 10-30 % of the reference keypoints without depth, fractional coordinates, depth ties, 0 < n_close < n_valid,
    and (float32) NaN / negative / +0.0 pixels under keypoints"""
    _reference_case(cam, W, H, nf, fmt, SEEDS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ops(orbx, cam, W, H):
    K, dist = rgbd_ref.CAMS[cam]
    ops = orbx.FrameOps(K[0], K[1], K[2], K[3], dist)
    return ops, orbx.FrameGrid.from_bounds(ops.ComputeImageBounds(W, H)), float(rgbd_ref.th_depth(K[0]))


def _xy(kps):
    return np.stack([kps["x"], kps["y"]], 1).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_hip_matches_fixture(orbx, fmt):
    """batch form (one frame) and latency form against the recorded fixture"""
    z, want = load_golden()
    gray, raw, img, _ = golden_images(z)
    W, H, nf = int(z["W"]), int(z["H"]), int(z["nfeatures"])
    image, factor = (raw, float(z["u16_factor"])) if fmt == "u16" else (img, 1.0)
    n = len(z["kps"])
    ops = orbx.FrameOps(*[float(v) for v in z["cam"]], z["dist"])
    grid = orbx.FrameGrid.from_bounds(ops.ComputeImageBounds(W, H))
    ext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H)
    kps = ext.extract_with_pyramid(gray)[0]
    assert rgbd_ref.same_bits(_xy(kps), z["kps"])
    un, off, idx, cnt, r = ops.rgbd_frame(ext, grid, image, float(z["bf"]), float(z["th_depth"]), factor)
    assert cnt == n and rgbd_ref.same_bits(_xy(un), z["kpsUn"])
    rgbd_ref.assert_same(r, want[fmt])
    un2, off2, idx2, _ = ops.finish_frame(ext, grid)      # the frame-finish results of the fused launch are those of the plain one
    assert (un2.view(np.uint8) == un.view(np.uint8)).all() and (off2 == off).all() and (idx2 == idx).all()
    dev = ext.upload([gray])
    ext.run_device(*dev)
    ops.rgbd_device(ext, grid, ops.upload_depth([image], factor), float(z["bf"]), float(z["th_depth"]))
    b = ops.rgbd_download(ext, 1)
    rgbd_ref.assert_same({k: v[0] for k, v in b.items()}, want[fmt], n)
    ops.close(); ext.close()


@needs_ref
@pytest.mark.gpu
@pytest.mark.parametrize("cam,W,H,nf", CASES)
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_hip_batch_and_latency_forms(orbx, cam, W, H, nf, fmt):
    """B = 8 different frames in one batch and the same frames one by one through the latency form: both equal the restatement on the
    compiled reference's keypoints, hence each other, to the bit"""
    case = _reference_case(cam, W, H, nf, fmt, SEEDS)
    B = len(case)
    ops, grid, thd = _ops(orbx, cam, W, H)
    ext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    ext.run_device(*ext.upload([c[0] for c in case]))
    ops.rgbd_device(ext, grid, ops.upload_depth([c[1] for c in case], float(case[0][2])), rgbd_ref.BF, thd)
    kps, _, counts = ext.download(B)
    got = ops.rgbd_download(ext, B)
    un_b = ops.download(ext, B)[0]
    one = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H)
    for f, (gray, image, factor, ref_xy, want) in enumerate(case):
        n = int(counts[f])
        assert n == len(ref_xy) and rgbd_ref.same_bits(_xy(kps[f, :n]), ref_xy)
        rgbd_ref.assert_same({k: v[f] for k, v in got.items()}, want, n)
        k1 = one.extract_with_pyramid(gray)[0]
        assert rgbd_ref.same_bits(_xy(k1), ref_xy)
        un, off, idx, cnt, r = ops.rgbd_frame(one, grid, image, rgbd_ref.BF, thd, float(factor))
        assert cnt == n
        rgbd_ref.assert_same(r, want)
        for k in ("depth", "u_right", "order", "xyz_cam"):
            assert rgbd_ref.same_bits(r[k], got[k][f][:n]), k
        if un is not None:
            assert (un.view(np.uint8) == un_b[f, :n].view(np.uint8)).all()
    ops.close(); ext.close(); one.close()


@needs_ref
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_hip_strided_depth_and_staged_image(orbx, fmt, monkeypatch):
    """rows of the depth image further apart than cols * pixel size: latency form (host look-up and ORBX_RGBD_STAGE_IMAGE=1) and upload"""
    cam, W, H, nf = CASES[0]
    gray, image, factor, ref_xy, want = _reference_case(cam, W, H, nf, fmt, SEEDS[:1])[0]
    wide = np.full((H, W + 24), 7 if fmt == "u16" else np.float32(3.0), image.dtype)      # (what a wrong stride would read has a depth)
    wide[:, :W] = image
    view = wide[:, :W]
    assert view.strides[0] == (W + 24) * image.itemsize
    ops, grid, thd = _ops(orbx, cam, W, H)
    ext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H)
    for stage in ("0", "1"):
        monkeypatch.setenv("ORBX_RGBD_STAGE_IMAGE", stage)
        ext.extract_with_pyramid(gray)
        r = ops.rgbd_frame(ext, grid, view, rgbd_ref.BF, thd, float(factor))[4]
        rgbd_ref.assert_same(r, want)
    ext.run_device(*ext.upload([gray]))
    ops.rgbd_device(ext, grid, ops.upload_depth([view], float(factor)), rgbd_ref.BF, thd)
    rgbd_ref.assert_same({k: v[0] for k, v in ops.rgbd_download(ext, 1).items()}, want, len(ref_xy))
    ops.close(); ext.close()


@pytest.mark.gpu
def test_error_returns(orbx):
    L = orbx.load_library()
    W, H = 640, 480
    ops, grid, thd = _ops(orbx, "tum1", W, H)
    ext = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H)
    depth = np.ones((H, W), np.float32)
    prm = orbx.RgbdParams(40.0, thd)
    g, p = ctypes.byref(grid), ctypes.byref(prm)

    def fails(rc, code):
        assert rc == code, (rc, code)
        assert len(L.orbx_last_error()) > 0

    def dd(image=depth, **kw):
        d = orbx.DepthDesc.of(image)
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)
    rf = orbx.RgbdFrame()
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, dd(), p), -5)                       # nothing extracted yet
    fails(L.orbx_frame_rgbd_device(ops._h, ext._h, g, dd(), p), -5)
    fails(L.orbx_frame_rgbd_end(ops._h, None, None, None, None, ctypes.byref(rf)), -5)    # _end without _begin
    fails(L.orbx_frame_rgbd_results_device(ops._h, None, None, None, None, None, None, None), -5)
    ext.extract_with_pyramid(rgbd_ref.gray_frame(61, W, H))
    fails(L.orbx_frame_rgbd_begin(None, ext._h, g, dd(), p), -1)
    fails(L.orbx_frame_rgbd_begin(ops._h, None, g, dd(), p), -1)
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, None, p), -1)
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, dd(), None), -1)
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, dd(np.ones((H, W - 8), np.float32)), p), -1)      # not the extractor's frame size
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, dd(format=7), p), -1)                # unknown format
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, dd(stride_bytes=W * 4 - 4), p), -1)
    fails(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, dd(data=None), p), -1)
    fails(L.orbx_frame_rgbd_end(None, None, None, None, None, ctypes.byref(rf)), -1)
    fails(L.orbx_frame_rgbd_end(ops._h, None, None, None, None, ctypes.byref(rf)), -5)    # the failed _begins began nothing
    fails(L.orbx_frame_rgbd_device(None, ext._h, g, dd(), p), -1)
    fails(L.orbx_frame_rgbd_device(ops._h, ext._h, g, dd(format=-1), p), -1)
    fails(L.orbx_frame_rgbd_device(ops._h, ext._h, g, dd(np.ones((H + 1, W), np.float32)), p), -1)
    out = orbx.DepthDesc()
    arr = (ctypes.c_void_p * 1)(depth.ctypes.data)
    fails(L.orbx_upload_depth(None, arr, 1, 0, W, H, W * 4, 1.0, ctypes.byref(out)), -1)
    fails(L.orbx_upload_depth(ops._h, arr, 1, 5, W, H, W * 4, 1.0, ctypes.byref(out)), -1)
    fails(L.orbx_frame_rgbd_download(ops._h, ext._h, 1, None, None, None, None, None, None), -5)      # no RGB-D batch yet
    # a plain frame begun is not an RGB-D frame; after a batch extraction the extractor holds no single-frame result
    orbx._check(L.orbx_frame_finish_begin(ops._h, ext._h, g))
    fails(L.orbx_frame_rgbd_end(ops._h, None, None, None, None, ctypes.byref(rf)), -5)
    bext = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=2)
    bext.run_device(*bext.upload([rgbd_ref.gray_frame(61, W, H), rgbd_ref.gray_frame(62, W, H)]))
    fails(L.orbx_frame_rgbd_begin(ops._h, bext._h, g, dd(), p), -5)
    # and the handle still works
    r = ops.rgbd_frame(ext, grid, depth, 40.0, thd)[4]
    assert r["n_valid"] == len(r["depth"]) and (r["depth"] == 1.0).all() and (r["order"] == np.arange(len(r["depth"]))).all()
    ops.close(); ext.close(); bext.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# shim/FrameRGBD_hip.cc compiles against the reference's Frame.h with the flags oracle/Makefile's HIP_FLAGS spell (nothing linked or run)
# ---------------------------------------------------------------------------------------------------------------------------------------
REF = Path("/root/reference")


@pytest.mark.skipif(not os.access(REF / "include" / "Frame.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "FrameRGBD_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    src = (shim / "FrameRGBD_hip.cc").read_text()
    assert "void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)" in src
    assert "ComputeStereoFromRGBD" not in (shim / "Frame_hip.cc").read_text()      # one definition: the drop-in link stays as it is
