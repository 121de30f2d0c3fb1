"""Expected values of the RGB-D frame path, independent of the code under test.

The RGB-D constructor (reference src/Frame.cc:238-348) extracts and undistorts exactly like the monocular one, so mvKeys / mvKeysUn come from
the compiled reference (oracle_lib.ref_mono_frame).  What is not compiled behind an export is restated here in numpy float32, ONE operation per
numpy call so that nothing is fused or promoted:
    Frame::ComputeStereoFromRGBD   src/Frame.cc:1428-1459
    Frame::UnprojectStereo         src/Frame.cc:1478-1491 (camera frame: before mRwc * x + mOw)
    the tracker's depth order (sorted vector<pair<float,int>>) and close-point count (0 < z < mThDepth), src/Tracking.cc
and the uint16 -> float conversion of Tracking::GrabImageRGBD (src/Tracking.cc:212-216, 334-338), d = (float)raw * (float)factor: the
published behaviour of cv::Mat::convertTo(CV_32F, scale) for 16U input (OpenCV is not vendored by the reference: parity unpinned there).

Also the seeded synthetic inputs: a gray frame (texture_frames) and a depth image - a smooth surface between 0.4 and 8 m, rectangular holes of
value 0 - as raw uint16 at 5000 units per metre (the TUM convention) and as float32 with NaN, negative and +0.0 pixels planted under keypoints."""
import numpy as np

import texture_frames

F32 = np.float32
U16_FACTOR = F32(1.0) / F32(5000.0)      # mDepthMapFactor = 1.0f / DepthMapFactor, src/Tracking.cc:212-216

# fx fy cx cy, distortion; the sizes the tests run
CAMS = {
    "tum1": ([517.306408, 516.469215, 318.643040, 255.313989], [0.262383, -0.953104, -0.005358, 0.002628, 1.163314]),
    "tum3": ([535.4, 539.2, 320.1, 247.6], [0.0, 0.0, 0.0, 0.0]),
    "euroc": ([458.654, 457.296, 367.215, 248.375], [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]),
    "euroc_rect": ([458.654, 457.296, 367.215, 248.375], [0.0, 0.0, 0.0, 0.0]),
}
BF = 40.0                                # Camera.bf of Examples/RGB-D/TUM1.yaml
TH_DEPTH_FACTOR = 40.0                   # ThDepth of the same file


def th_depth(fx):
    """mThDepth = mbf * ThDepth / fx in float arithmetic (src/Tracking.cc:205)"""
    return F32(F32(F32(BF) * F32(TH_DEPTH_FACTOR)) / F32(fx))


def gray_frame(seed, W, H):
    return texture_frames.texture_frame("pink", seed, W, H)


def depth_raw(seed, W, H):
    """uint16 depth: smooth surface 2000 .. 40000 (0.4 .. 8 m at 5000 / m), quantised to 4 units like a sensor, ten rectangular holes of 0."""
    rng = np.random.Generator(np.random.PCG64(seed * 104729 + 17))
    surf = 21000 + texture_frames._value_noise(rng, W, H, 96, 19000)
    raw = (np.clip(surf, 2000, 40000) >> 2) << 2
    for _ in range(10):
        w, h = int(rng.integers(W // 10, W // 5)), int(rng.integers(H // 10, H // 5))
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        raw[y:y + h, x:x + w] = 0
    return raw.astype(np.uint16)


def pixel_of(kps_xy):
    """imDepth.at<float>(v, u) with float arguments: converted to int by truncation (src/Frame.cc:1440-1444)"""
    xy = np.asarray(kps_xy, F32)
    return xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32)


def depth_f32(raw, kps_xy):
    """the float32 image of the same surface, plus the pixels a real depth image can hold and `d > 0` must reject: NaN, a negative value and
    +0.0, each planted under (at least) one reference keypoint that had a depth; returns (image, planted pixel list)"""
    img = np.multiply(raw.astype(F32), U16_FACTOR)
    iu, iv = pixel_of(kps_xy)
    have = np.flatnonzero(raw[iv, iu] > 0)
    picks, seen = [], set()
    for i in have[::max(1, len(have) // 7)]:      # spread over the list (= over the pyramid levels)
        if (iv[i], iu[i]) not in seen:
            seen.add((iv[i], iu[i]))
            picks.append(int(i))
        if len(picks) == 3:
            break
    assert len(picks) == 3
    for i, val in zip(picks, (F32(np.nan), F32(-1.5), F32(0.0))):
        img[iv[i], iu[i]] = val
    return img, [(int(iv[i]), int(iu[i])) for i in picks]


def lookup(image, kps_xy, factor=None):
    """d of every keypoint as a float32 array: the pixel under the truncated mvKeys position, converted if the image is uint16"""
    iu, iv = pixel_of(kps_xy)
    d = image[iv, iu]
    if image.dtype == np.uint16:
        d = np.multiply(d.astype(F32), F32(factor))
    assert d.dtype == F32
    return d


def restate(d, un_xy, K, bf, thd):
    """d: looked-up depth per feature (float32), un_xy: mvKeysUn.pt -> dict(depth, u_right, order, n_valid, n_close, xyz_cam)"""
    d = np.asarray(d, F32)
    un = np.asarray(un_xy, F32)
    n = len(d)
    fx, fy, cx, cy = (F32(v) for v in K)
    bf, thd = F32(bf), F32(thd)
    invfx, invfy = np.divide(F32(1.0), fx), np.divide(F32(1.0), fy)      # Frame::invfx = 1.0f / fx, src/Frame.cc:327-334
    with np.errstate(all="ignore"):
        valid = np.greater(d, F32(0.0))                                   # false for NaN
        q = np.divide(bf, d)
        ur = np.subtract(un[:, 0], q)                                     # kpU.pt.x - mbf / d
        x = np.multiply(np.multiply(np.subtract(un[:, 0], cx), d), invfx) # (u - cx) * z * invfx
        y = np.multiply(np.multiply(np.subtract(un[:, 1], cy), d), invfy)
    for a in (q, ur, x, y):
        assert a.dtype == F32
    depth = np.where(valid, d, F32(-1.0)).astype(F32)
    u_right = np.where(valid, ur, F32(-1.0)).astype(F32)
    xyz = np.zeros((n, 3), F32)
    xyz[valid, 0], xyz[valid, 1], xyz[valid, 2] = x[valid], y[valid], d[valid]
    pairs = sorted((float(d[i]), int(i)) for i in np.flatnonzero(valid))  # vector<pair<float,int>>: by depth, ties by index
    order = np.full(n, -1, np.int32)
    order[:len(pairs)] = [i for _, i in pairs]
    n_close = int(np.count_nonzero(valid & np.less(d, thd)))
    return dict(depth=depth, u_right=u_right, order=order, n_valid=len(pairs), n_close=n_close, xyz_cam=xyz)


def check_inputs(kps_xy, d, want, special_pixels=None, image=None):
    """Conditions on the inputs, on the reference's values: the test exercises what it means to exercise."""
    xy = np.asarray(kps_xy, F32)
    n = len(xy)
    none = n - want["n_valid"]
    assert 0.10 * n <= none <= 0.30 * n and none >= 50 and want["n_valid"] >= 50, (n, none)
    frac = (np.trunc(xy[:, :2]) != np.round(xy[:, :2])).any(axis=1)        # truncation and rounding pick different pixels
    assert np.count_nonzero(frac) >= 50, np.count_nonzero(frac)
    z = np.sort(want["depth"][want["depth"] > 0])
    assert np.count_nonzero(z[1:] == z[:-1]) >= 2, "no two features share a depth: the (z, i) tie rule is not exercised"
    assert 0 < want["n_close"] < want["n_valid"], (want["n_close"], want["n_valid"])
    if special_pixels is not None:
        vals = [image[p] for p in special_pixels]
        assert np.isnan(vals[0]) and vals[1] < 0 and vals[2] == 0 and not np.signbit(vals[2])
        iu, iv = pixel_of(xy)
        for p in special_pixels:
            hit = np.flatnonzero((iv == p[0]) & (iu == p[1]))
            assert len(hit) >= 1 and (want["depth"][hit] == -1).all() and (want["u_right"][hit] == -1).all()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and np.array_equal(a, b)


def assert_same(got, want, n=None):
    for k in ("depth", "u_right", "order", "xyz_cam"):
        g, w = (got[k], want[k]) if n is None else (got[k][:n], want[k][:n])
        assert same_bits(np.asarray(g, w.dtype) if w.dtype != np.float32 else g, w), k
    assert int(got["n_valid"]) == int(want["n_valid"]) and int(got["n_close"]) == int(want["n_close"]), (got["n_valid"], got["n_close"], want["n_valid"], want["n_close"])
