"""The image front end restated in numpy (include/orbx.h, "Image front end"): colour to grey, the fixed-point maps, remap, and
initUndistortRectifyMap in double.  This is what csrc/orbx_image.hip is held to, byte for byte (bit for bit for the maps).

PARITY WITH OpenCV IS UNPINNED, as oracle/prims.h says of resize: the grey weights and the SIMD path depend on the OpenCV version, the
reference inverts Pnew * R by LU (here: cofactors), and cv::remap corrects the sum of its four 16-bit weights on one entry -
remap_table() below is OpenCV's literal form with that correction as an option, and tests/test_image_prep.py shows that it equals the
short form for all 1024 phases, so the correction changes no output."""
import numpy as np

GRAY_CV4 = ((9798, 19235, 3735), 15)      # R, G, B, shift: OpenCV 4.x, 8-bit path
GRAY_CV3 = ((4899, 9617, 1868), 14)       # OpenCV 3.x


def gray_rgb(r, g, b, coef=GRAY_CV4[0], shift=GRAY_CV4[1]):
    """(c[R] r + c[G] g + c[B] b + (1 << (shift - 1))) >> shift in 32-bit unsigned"""
    r, g, b = (np.asarray(a).astype(np.uint32) for a in (r, g, b))
    return ((np.uint32(coef[0]) * r + np.uint32(coef[1]) * g + np.uint32(coef[2]) * b + np.uint32(1 << (shift - 1))) >> np.uint32(shift)).astype(np.uint8)


def gray(img, rgb=True, coef=GRAY_CV4[0], shift=GRAY_CV4[1]):
    """(H, W) is returned as it is; (H, W, 3 / 4): the first byte is R (rgb) or B, a fourth byte is ignored"""
    img = np.asarray(img)
    if img.ndim == 2:
        return img.copy()
    c0, c2 = img[..., 0], img[..., 2]
    return gray_rgb(c0 if rgb else c2, img[..., 1], c2 if rgb else c0, coef, shift)


def maps_fixed(mx, my):
    """sx = rint(map * 32) half to even (|s| clamped to 2^30: changes nothing, ix saturates from 2^20 on and every float from 2^29 on is a
    multiple of 32); ix = saturate_int16(sx >> 5) with an arithmetic shift, fx = sx & 31 -> ix, iy, fx, fy (int64)"""
    out = []
    for m in (mx, my):
        m = np.asarray(m, np.float32)
        assert np.isfinite(m).all()
        with np.errstate(over="ignore"):
            s = np.rint(m * np.float32(32.0))      # exact product (or infinite), float32 rint = half to even
        s = np.clip(s, np.float32(-2.0 ** 30), np.float32(2.0 ** 30)).astype(np.int64)
        out.append((np.clip(s >> 5, -32768, 32767), s & 31))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _taps(src, ix, iy):
    H, W = src.shape

    def tap(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(np.int64)      # BORDER_CONSTANT, value 0
    return tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)


def blend_short(p00, p01, p10, p11, fx, fy):
    return ((32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p01 + (32 - fx) * fy * p10 + fx * fy * p11 + 512) >> 10


def remap_table(fixup=None):
    """OpenCV's literal table: 16-bit weights saturate_short(w * 32768) of the four taps for every (fy, fx), w the float bilinear weight; the
    entry of tap 0 at fx = fy = 0 saturates to 32767.  fixup = k adds what the sum lacks of 32768 to tap k (OpenCV picks the largest weight,
    which a short cannot take: every other tap is tried instead, and tap 0 as the unsaturated 32768)."""
    f = np.arange(32, dtype=np.float32) / np.float32(32.0)
    wy, wx = np.meshgrid(f, f, indexing="ij")
    w = np.stack([(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy], -1)      # exact in float32: products of k / 32
    tab = np.clip(np.rint(w * np.float32(32768.0)), -32768, 32767).astype(np.int64)
    assert tab[0, 0, 0] == 32767 and (tab.sum(-1).reshape(-1)[1:] == 32768).all()
    if fixup is not None:
        tab[..., fixup] += 32768 - tab.sum(-1)
    return tab


def blend_table(p00, p01, p10, p11, fx, fy, tab):
    w = tab[fy, fx]
    return (w[..., 0] * p00 + w[..., 1] * p01 + w[..., 2] * p10 + w[..., 3] * p11 + 16384) >> 15


def remap(src, mx, my):
    """cv::remap(src, maps, INTER_LINEAR, BORDER_CONSTANT 0) in the pinned arithmetic; src (H, W) uint8, output of the maps' shape"""
    ix, iy, fx, fy = maps_fixed(mx, my)
    return blend_short(*_taps(np.asarray(src), ix, iy), fx, fy).astype(np.uint8)


def prep(img, rgb=True, coef=GRAY_CV4[0], shift=GRAY_CV4[1], maps=None):
    """the front end on one frame: grey first, then the remap of the grey image"""
    g = gray(img, rgb, coef, shift)
    return g if maps is None else remap(g, maps[0], maps[1])


def rectify_maps(K, D, R, P, w, h):
    """cv::initUndistortRectifyMap(K, D, R, P[:3, :3], (w, h), CV_32FC1) as orbx_rectify_maps states it: every operation an IEEE double
    operation in the same order (numpy's elementwise loops do not contract, np.add.accumulate adds in sequence)."""
    K = [float(v) for v in np.asarray(K, np.float64).reshape(-1)]
    R = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
    P = [float(v) for v in np.asarray(P, np.float64).reshape(3, -1)[:, :3].reshape(-1)]
    D = [float(v) for v in np.asarray(D, np.float64).reshape(-1)]
    assert len(D) in (4, 5)
    A = [(P[3 * i] * R[j] + P[3 * i + 1] * R[3 + j]) + P[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
    C = [A[3 * ((i + 1) % 3) + (j + 1) % 3] * A[3 * ((i + 2) % 3) + (j + 2) % 3] - A[3 * ((i + 1) % 3) + (j + 2) % 3] * A[3 * ((i + 2) % 3) + (j + 1) % 3]
         for i in range(3) for j in range(3)]
    det = (A[0] * C[0] + A[1] * C[1]) + A[2] * C[2]
    idet = 1.0 / det
    iR = [C[3 * j + i] * idet for i in range(3) for j in range(3)]
    fx, fy, u0, v0 = K[0], K[4], K[2], K[5]
    k1, k2, p1, p2 = D[:4]
    k3 = D[4] if len(D) == 5 else 0.0
    i = np.arange(h, dtype=np.float64)[:, None]

    def run(a, b, step):      # row start i * a + b, then += step per column, in sequence
        first = i * a + b
        return np.add.accumulate(np.concatenate([first, np.full((h, w - 1), step, np.float64)], 1), axis=1)
    _x, _y, _w = run(iR[1], iR[2], iR[0]), run(iR[4], iR[5], iR[3]), run(iR[7], iR[8], iR[6])
    wi = 1.0 / _w
    x, y = _x * wi, _y * wi
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, (2.0 * x) * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    u = fx * ((x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2)) + u0
    v = fy * ((y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy) + v0
    return u.astype(np.float32), v.astype(np.float32)


def distort_forward(K, D, R, P, w, h):
    """An independent float64 statement of the same model (np.linalg.inv, no incremental sums): where the rectified pixel grid lands in the raw image"""
    K, R = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
    P = np.asarray(P, np.float64).reshape(3, -1)[:, :3]
    D = list(np.asarray(D, np.float64).reshape(-1)) + [0.0]
    k1, k2, p1, p2, k3 = D[:5]
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ray = np.linalg.inv(P @ R) @ np.stack([uu.ravel(), vv.ravel(), np.ones(w * h)])
    x, y = ray[0] / ray[2], ray[1] / ray[2]
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return (K[0, 0] * xd + K[0, 2]).reshape(h, w), (K[1, 1] * yd + K[1, 2]).reshape(h, w)
