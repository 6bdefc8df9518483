#!/usr/bin/env python3
"""Normal estimation on the GPU (fvo_estimate_normals) on the map tools/bench_outlier.py uses:
synthetic forest -> StereoSGBM -> PointMap.add_disparity(voxel_size=0.5) over --frames frames placed
by their ground-truth poses (0.6 million points at the defaults).
Timed with HIP events, the calls alternated in one process (--reps rounds, median and min):
  * hybrid search (radius 1 m, max_nn 30) at cell = radius,
  * k-NN search (max_nn 30) at cell 1 and 2 m,
  * fvo_statistical_outliers (30, 2.0) at the same cells: the yardstick, the parent's code doing the
    same search (its ring walk, its exact pass) without the covariance and the eigen-solve,
  * fvo_orient_normals towards a camera location.
All at max_rings 2.  Untimed: the queries each call sends to the exact pass and the points with
fewer than 3 neighbours (stats), the histogram's ends of the hybrid search's neighbour counts.
    python tools/bench_normals.py [--frames F] [--step S] [--reps N] [--out profiles/normals/bench_normals.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=384)
    ap.add_argument("--stride", type=int, default=1, help="every stride-th frame of the sequence")
    ap.add_argument("--step", type=int, default=1, help="pixel step of add_disparity")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-nn", type=int, default=30)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals", "bench_normals.json"))
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
    n = len(pm)
    print(f"map: {n} points", file=sys.stderr, flush=True)
    pts = pm.xyz64[:n].contiguous()
    ext = (pts.max(0).values - pts.min(0).values).cpu().numpy().round(1).tolist()
    k, radius = a.max_nn, a.radius
    ws = torch.empty((ctx.normals_workspace_bytes(n, k),), dtype=torch.uint8, device="cuda")
    ows = torch.empty((ctx.outlier_workspace_bytes(n, k),), dtype=torch.uint8, device="cuda")
    nrm = ctx.estimate_normals(pts, k, radius, workspace=ws)[0].clone()
    cam = tuple(float(v) for v in seq.T_wc[idx[0]][:3, 3])
    calls = {"hybrid": lambda: ctx.estimate_normals(pts, k, radius, radius, 2, workspace=ws),
             "knn_cell1": lambda: ctx.estimate_normals(pts, k, cell=1.0, max_rings=2, workspace=ws),
             "knn_cell2": lambda: ctx.estimate_normals(pts, k, cell=2.0, max_rings=2, workspace=ws),
             "statistical_cell1": lambda: ctx.statistical_outliers(pts, k, 2.0, 1.0, 2, workspace=ows),
             "statistical_cell2": lambda: ctx.statistical_outliers(pts, k, 2.0, 2.0, 2, workspace=ows),
             "orient": lambda: ctx.orient_normals(pts, nrm, camera_location=cam)}
    for f in calls.values():  # warm-up
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(a.reps):  # alternated
        for name, f in calls.items():
            ms[name].append(timed(f))
        print("round: " + ", ".join(f"{name} {v[-1]:.3f} ms" for name, v in ms.items()), file=sys.stderr, flush=True)
    res = {name: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4)} for name, v in ms.items()}
    for name in ("hybrid", "knn_cell1", "knn_cell2"):
        s = calls[name]()[3].cpu().numpy()
        res[name].update(exact_queries=int(s[0]), fewer_than_3=int(s[1]))
    for name in ("statistical_cell1", "statistical_cell2"):
        res[name]["exact_queries"] = int(calls[name]()[2][5].item())
    cnt = ctx.estimate_normals(pts, k, radius, radius, 2, n_neighbors=True, workspace=ws)[2]
    rec = {"bench": "normals", "points": n, "extent_m": ext, "frames": B, "frame_stride": a.stride, "step": a.step,
           "reps": a.reps, "max_nn": k, "radius": radius, "max_rings": 2, **res,
           "hybrid_neighbours": {"full": int((cnt == k).sum().item()), "mean": round(float(cnt.double().mean().item()), 3)},
           "yardstick": "fvo_statistical_outliers(max_nn, 2.0) on the same cloud, cell and max_rings"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
