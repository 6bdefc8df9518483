"""Generate tests/golden/golden_rectify.npz from the specification tests/rectify_ref.py: a 96 x 64
stereo rig (the x4 rig of tests/rectify_scene.py at 0.1 scale), its rectification, both
undistort-rectify maps and one rectified gray image of a seeded synthetic BGR image.  The vector
pins the specification and rectify.stereo_rectify against regressions.
    python tests/golden/make_golden_rectify.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import rectify_ref as ref  # noqa: E402
import rectify_scene as scene  # noqa: E402
from make_golden_ingest import synthetic_bgr  # noqa: E402


def main():
    from forest_slam_amd.rectify import stereo_rectify
    W, H = 96, 64
    K1, d1, K2, d2, R, T = scene.rig(4.0, 0.1)
    r = stereo_rectify(K1, d1, K2, d2, (W, H), R, T)
    bgr = synthetic_bgr(H, W, 11)
    out = dict(size=np.array([W, H]), K1=K1, d1=d1, K2=K2, d2=d2, R=R, T=T, R1=r.R1, R2=r.R2, P1=r.P1, P2=r.P2, Q=r.Q,
               bgr=bgr, gray=ref.rectify_gray(bgr, K1, d1, r.R1, r.P1[:, :3]))
    for k, (K, d, Rk, P) in enumerate(((K1, d1, r.R1, r.P1), (K2, d2, r.R2, r.P2))):
        out[f"map1_{k}"], out[f"map2_{k}"] = ref.rectify_map(K, d, Rk, P[:, :3], W, H)
    np.savez_compressed(os.path.join(HERE, "golden_rectify.npz"), **out)
    print("golden_rectify.npz", out["gray"].mean())


if __name__ == "__main__":
    main()
