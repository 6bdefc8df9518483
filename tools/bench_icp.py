#!/usr/bin/env python3
"""ICP registration on the GPU (fvo_registration_icp) against the map tools/bench_outlier.py and
tools/bench_normals.py use: synthetic forest -> StereoSGBM -> PointMap.add_disparity(voxel_size=0.5)
over --frames frames placed by their ground-truth poses (0.6 million points at the defaults) is the
target, with normals from the hybrid search (radius 1 m, max_nn 30).  The source is a voxel-thinned
copy (voxel_down_sample at --thin metres) moved by the inverse of a small known motion about the
centroid.  Timed with HIP events, the calls alternated in one process (--reps rounds, median and min):
  * evaluate_registration (max_iteration 0): the target grid, the source order and one pass,
  * 8 more passes with criteria 0 (the loop never stops early): the time of one pass = the difference / 8,
  * a whole registration with the default criteria, point-to-point and point-to-plane, and the updates
    it took,
  * fvo_radius_outliers(5, r) at cell = r on the target and on the source: the yardstick, the parent's
    code doing one sort, one gather and a 27-cell walk per point.
    python tools/bench_icp.py [--frames F] [--reps N] [--out profiles/icp/bench_icp.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    k = w / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=384)
    ap.add_argument("--stride", type=int, default=1, help="every stride-th frame of the sequence")
    ap.add_argument("--step", type=int, default=1, help="pixel step of add_disparity")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.5, help="max_correspondence_distance")
    ap.add_argument("--thin", type=float, default=1.0, help="voxel size of the source")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp", "bench_icp.json"))
    a = ap.parse_args()
    from forest_slam_amd import _lib, synth
    from forest_slam_amd.mapping import PointMap
    B, W, H = a.frames, 960, 600
    seq = synth.StereoSequence(seed=0, n_frames=B * a.stride, W=W, H=H, device="cuda")
    idx = list(range(0, B * a.stride, a.stride))
    ctx = _lib.Context(W, H, max_batch=16, stages=_lib.STAGE_SGBM)
    pm = PointMap(B * H * W // (a.step * a.step) + 16, ctx=ctx)
    for c in range(0, B, 16):
        ii = idx[c:c + 16]
        L, R = seq.frames(ii)
        disp = ctx.sgbm(L, R)
        pm.add_disparity(disp, seq.K, synth.BASELINE, np.stack([seq.T_wc[i] for i in ii]), step=a.step,
                         voxel_size=0.5)
    nt = len(pm)
    pm.estimate_normals(30, 1.0)
    tgt, nrm = pm.xyz64[:nt].contiguous(), pm.normals64[:nt].contiguous()
    thin, nv, _ = ctx.voxel_down_sample(tgt, a.thin)
    ns = int(nv.item())
    # the known motion x -> c + R (x - c) + t; the source is the thinned cloud moved by its inverse
    center = tgt.mean(0).cpu().numpy()
    Rm, t = rodrigues((0.0004, -0.0006, 0.0008)), np.array([0.06, -0.05, 0.04])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rm, center - Rm @ center + t
    src = thin[:ns].clone()
    ctx.transform_points(src, np.linalg.inv(M))
    print(f"target: {nt} points, source: {ns} points", file=sys.stderr, flush=True)
    r = a.radius
    ws = torch.empty((ctx.icp_workspace_bytes(ns, nt),), dtype=torch.uint8, device="cuda")
    ows = torch.empty((ctx.outlier_workspace_bytes(nt, 1),), dtype=torch.uint8, device="cuda")

    def icp(est, it, rel=1e-6):
        return ctx.registration_icp(src, tgt, r, None, est, nrm if est else None, rel, rel, it, workspace=ws)

    calls = {"evaluate_point": lambda: icp(0, 0), "evaluate_plane": lambda: icp(1, 0),
             "passes9_point": lambda: icp(0, 8, 0.0), "passes9_plane": lambda: icp(1, 8, 0.0),
             "registration_point": lambda: icp(0, 30), "registration_plane": lambda: icp(1, 30),
             "radius_target": lambda: ctx.radius_outliers(tgt, 5, r, workspace=ows),
             "radius_source": lambda: ctx.radius_outliers(src, 5, r, workspace=ows)}
    for f in calls.values():  # warm-up
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(a.reps):  # alternated
        for name, f in calls.items():
            ms[name].append(timed(f))
        print("round: " + ", ".join(f"{name} {v[-1]:.3f} ms" for name, v in ms.items()), file=sys.stderr, flush=True)
    res = {name: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4)} for name, v in ms.items()}
    for name, est in (("point", 0), ("plane", 1)):
        out = icp(est, 30)[0].cpu().numpy()
        res["registration_" + name].update(updates=int(out[19]), fitness=round(float(out[16]), 6),
                                           inlier_rmse=round(float(out[17]), 6),
                                           max_abs_T_minus_motion=float(np.abs(out[:16].reshape(4, 4) - M).max()))
        ev = icp(est, 0)[0].cpu().numpy()
        res["evaluate_" + name].update(fitness=round(float(ev[16]), 6), inlier_rmse=round(float(ev[17]), 6))
        res["pass_" + name] = {"ms": round((res["passes9_" + name]["ms"] - res["evaluate_" + name]["ms"]) / 8, 4)}
    per_query = res["radius_target"]["ms"] / nt
    rec = {"bench": "icp", "target_points": nt, "source_points": ns, "frames": B, "frame_stride": a.stride,
           "step": a.step, "reps": a.reps, "max_correspondence_distance": r, "cell": r, "thin": a.thin, **res,
           "pass_per_query_over_yardstick_per_point": {
               name: round(res["pass_" + name]["ms"] / ns / per_query, 3) for name in ("point", "plane")},
           "yardstick": "fvo_radius_outliers(5, r) at cell = r: one sort, one gather and a 27-cell walk per point"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
