"""Rectifying-ingest throughput on a batch of 960x600 BGR8 images resident in HBM, HIP-event times
after warm-up, the four variants alternating inside one process:
  (a) fvo_undistort_gray               the existing ingest, as the yardstick
  (b) fvo_rectify_gray                 blocks stage their source box in LDS (the budget of fvo.h)
  (c) fvo_rectify_gray, budget 0       every block gathers its taps from global memory
  (d) fvo_rectify_map once + fvo_remap_u8 per batch (the stored-map route, 3 channels out)
on the reference's calibration with the rotation of its stereo extrinsic multiplied by 4 (1.9
degrees).  Per variant: time per launch (median over the repeats, min and max as the spread),
images/s and GB/s of algorithmic traffic (channels + 1 B per pixel; (d): 3 + 3 B and 6 B of map).
Writes profiles/rectify/bench_rectify.json and prints it as one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rig():
    from forest_slam_amd import pipeline as pl
    M = np.linalg.inv(pl.T_RGB0_RGB1.reshape(4, 4))
    c = (np.trace(M[:3, :3]) - 1) / 2
    th = np.arccos(np.clip(c, -1, 1))
    v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) * (th / (2 * np.sin(th)))
    return pl.K0, pl.DIST_L, pl.K1, pl.DIST_R, v * 4.0, M[:3, 3].copy()  # a rotation vector is accepted


def main(B=128, W=960, H=600, reps=15, inner=4):
    from forest_slam_amd import _lib
    from forest_slam_amd.rectify import stereo_rectify
    K1, d1, K2, d2, om, T = _rig()
    r = stereo_rectify(K1, d1, K2, d2, (W, H), om, T)
    ctx = _lib.Context(W, H, max_batch=B, stages=_lib.STAGE_BF, kp_capacity=64)
    budget = _lib.RECTIFY_LDS_BYTES
    g = torch.Generator(device="cuda").manual_seed(0)
    bgr = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    gray = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    out3 = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    m1, m2 = ctx.rectify_map(K1, d1, r.R1, r.P1[:, :3])
    newK = r.P1[:, :3]

    def staged():
        ctx.rectify_lds_budget(budget)
        ctx.rectify_gray(bgr, K1, d1, r.R1, newK, out=gray)

    def direct():
        ctx.rectify_lds_budget(0)
        ctx.rectify_gray(bgr, K1, d1, r.R1, newK, out=gray)

    def stored():
        ctx.rectify_lds_budget(budget)
        ctx.remap(bgr, m1, m2, out=out3)

    variants = {"a_undistort_gray": (lambda: ctx.undistort_gray(bgr, K1, d1, out=gray), 4.0),
                "b_rectify_gray_staged": (staged, 4.0), "c_rectify_gray_direct": (direct, 4.0),
                "d_remap_stored_map": (stored, 12.0)}
    for fn, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, (fn, _) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    ctx.rectify_lds_budget(budget)
    res = {"images_per_launch": B, "width": W, "height": H, "repeats": reps, "launches_per_repeat": inner,
           "lds_budget_bytes": budget, "variants": {}}
    for k, (_, bpp) in variants.items():
        t = np.array(times[k])
        med = float(np.median(t))
        res["variants"][k] = {"launch_ms_median": round(med, 4), "launch_ms_min": round(float(t.min()), 4),
                              "launch_ms_max": round(float(t.max()), 4), "images_per_s": round(B / med * 1e3, 1),
                              "algorithmic_gbs": round(bpp * W * H * B / med / 1e6, 1)}
    v = res["variants"]
    res["b_over_a"] = round(v["b_rectify_gray_staged"]["launch_ms_median"] / v["a_undistort_gray"]["launch_ms_median"], 3)
    res["c_over_b"] = round(v["c_rectify_gray_direct"]["launch_ms_median"] /
                            v["b_rectify_gray_staged"]["launch_ms_median"], 3)
    os.makedirs(os.path.join(ROOT, "profiles", "rectify"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rectify", "bench_rectify.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
