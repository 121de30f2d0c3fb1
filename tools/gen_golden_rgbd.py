"""Writes tests/golden/slam/rgbd_tum_640x480_1000.npz: the RGB-D frame path's expected values on one seeded frame.

mvKeys / mvKeysUn are the COMPILED reference's (oracle/_ref/liborbslam.so: Frame::Frame(imGray, ...), same ExtractORB + UndistortKeyPoints as
the RGB-D constructor); depth, u_right, order, n_close, xyz_cam are tests/rgbd_ref.py's numpy restatement of src/Frame.cc:1428-1459, 1478-1491
on them, for the uint16 image (factor 1/5000) and the float32 image (with NaN, negative and +0.0 pixels under keypoints).  Camera: TUM1
intrinsics and distortion as in the mono_tum1_640x480_1000 golden, bf = 40, thDepth = 40 * bf / fx as Examples/RGB-D/TUM1.yaml gives.  The
images are not stored: gray frame and depth are regenerated from the seed (tests/texture_frames.py, tests/rgbd_ref.py).

    python tools/gen_golden_rgbd.py [--seed S]        (needs the reference build, oracle/_ref)
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import oracle_lib      # noqa: E402
import rgbd_ref        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=61)
    a = ap.parse_args()
    if oracle_lib.slam_lib() is None:
        raise SystemExit("oracle/_ref/liborbslam.so is not built")
    W, H, nf = 640, 480, 1000
    mono = np.load(ROOT / "tests" / "golden" / "slam" / "mono_tum1_640x480_1000.npz")
    cam, dist = mono["cam"], mono["dist"]
    ref = oracle_lib.ref_mono_frame(rgbd_ref.gray_frame(a.seed, W, H), nf, cam[0], cam[1], cam[2], cam[3], dist)
    kps, un = ref["kps"][:, :2].copy(), ref["kpsUn"][:, :2].copy()
    thd = rgbd_ref.th_depth(cam[0])
    raw = rgbd_ref.depth_raw(a.seed, W, H)
    img, special = rgbd_ref.depth_f32(raw, kps)
    out = dict(seed=a.seed, W=W, H=H, nfeatures=nf, cam=cam, dist=dist, bf=np.float32(rgbd_ref.BF), th_depth=thd, u16_factor=rgbd_ref.U16_FACTOR,
               kps=kps, kpsUn=un, special=np.asarray(special, np.int32))
    for tag, image, factor in (("u16", raw, rgbd_ref.U16_FACTOR), ("f32", img, None)):
        d = rgbd_ref.lookup(image, kps, factor)
        want = rgbd_ref.restate(d, un, cam, rgbd_ref.BF, thd)
        rgbd_ref.check_inputs(kps, d, want, special if tag == "f32" else None, image)
        if tag == "u16":
            base = want
            for k, v in want.items():      # (order as int16, xyz_cam as its x and y planes - z is the depth where there is one, else 0; tests/test_rgbd.py::load_golden undoes both)
                out["u16_" + k] = v.astype(np.int16) if k == "order" else v.T[:2].copy() if k == "xyz_cam" else v
        else:
            # the float32 image is the same surface: recorded as the features whose values differ from the uint16 run (the planted pixels) + the order
            diff = np.flatnonzero((want["depth"].view(np.uint32) != base["depth"].view(np.uint32)) | (want["u_right"].view(np.uint32) != base["u_right"].view(np.uint32)) |
                                  (want["xyz_cam"].view(np.uint32) != base["xyz_cam"].view(np.uint32)).any(axis=1))
            out.update(f32_diff=diff.astype(np.int32), f32_depth=want["depth"][diff], f32_u_right=want["u_right"][diff], f32_xyz_cam=want["xyz_cam"][diff],
                       f32_order=want["order"].astype(np.int16), f32_n_valid=want["n_valid"], f32_n_close=want["n_close"])
        print(tag, "n", len(kps), "n_valid", want["n_valid"], "n_close", want["n_close"])
    path = ROOT / "tests" / "golden" / "slam" / "rgbd_tum_640x480_1000.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
