#!/usr/bin/env python3
"""Outlier removal on the GPU (fvo_statistical_outliers, fvo_radius_outliers) on a map made by the
existing path: synthetic forest -> StereoSGBM -> PointMap.add_disparity(voxel_size=0.5) over
--frames frames placed by their ground-truth poses (0.6 million points at the defaults, 2.5 million
at --frames 960).
Timed with HIP events, the calls alternated in one process (--reps rounds, median and min):
  * fvo_statistical_outliers (20, 2.0) at cell 0.5, 1 and 2 (max_rings 2),
  * fvo_radius_outliers (nb_points 5, radius 0.5, cell = radius),
  * fvo_select_points by the statistical mask (both outputs),
  * fvo_voxel_down_sample(0.5) on the same cloud: the yardstick, one sort of the same points
    (0.32 ms per 1 M in profiles/r1/bench_map.jsonl).
Untimed, per cell: the queries left unresolved after max_rings = 0 .. 8 (stats[5]; their
differences are the share resolved at each ring) and the number sent to the exact pass at
max_rings 2.  The exact pass alone: a call with max_rings 0 at cell 1/64 m resolves nothing in
the rings (a cell holds one point), so its time less the time of the same call's grid (the
radius call at a tiny radius: sort + a near-empty walk) is the exact pass over n queries x n
points, measured on the first --exact-n points; per (query, point) pair it prices the exact pass
of the full runs (their unresolved count x n pairs): reported as an estimate, named so (an upper
bound: the per-query share of the pass weighs less at large n).
    python tools/bench_outlier.py [--frames F] [--step S] [--reps N] [--out profiles/outlier/bench_outlier.json]
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
    ap.add_argument("--exact-n", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier", "bench_outlier.json"))
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
    ws = torch.empty((ctx.outlier_workspace_bytes(n, 20),), dtype=torch.uint8, device="cuda")
    vws = torch.empty((int(ctx.L.fvo_voxel_workspace_bytes(n)),), dtype=torch.uint8, device="cuda")
    cells = (0.5, 1.0, 2.0)
    radius = 0.5
    keep0 = ctx.statistical_outliers(pts, 20, 2.0, 1.0, 2, workspace=ws)[0]
    o64, o32 = torch.empty_like(pts), torch.empty((n, 3), dtype=torch.float32, device="cuda")
    calls = {f"statistical_cell{c}": (lambda c=c: ctx.statistical_outliers(pts, 20, 2.0, c, 2, workspace=ws))
             for c in cells}
    calls["radius"] = lambda: ctx.radius_outliers(pts, 5, radius, workspace=ws)
    calls["select"] = lambda: ctx.select_points(pts, keep0, o64, o32)
    calls["voxel_down_sample"] = lambda: ctx.voxel_down_sample(pts, 0.5, workspace=vws)
    for f in calls.values():  # warm-up
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.reps):  # alternated
        for k, f in calls.items():
            ms[k].append(timed(f))
        print("round: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in ms.items()), file=sys.stderr, flush=True)
    res = {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4)} for k, v in ms.items()}
    # what each ring resolves (untimed)
    rings = {}
    for c in cells:
        left = []
        for r in range(8, -1, -1):  # the cheap calls first
            left.insert(0, int(ctx.statistical_outliers(pts, 20, 2.0, c, r, workspace=ws)[2][5].item()))
            print(f"cell {c} max_rings {r}: {left[0]} unresolved", file=sys.stderr, flush=True)
        rings[f"cell{c}"] = {"unresolved_after_ring": left,
                             "resolved_share_by_ring": [round((p - q) / n, 5) for p, q in zip([n] + left[:-1], left)],
                             "exact_queries_at_max_rings_2": left[2]}
    stats = ctx.statistical_outliers(pts, 20, 2.0, 1.0, 2, workspace=ws)[2].cpu().numpy()
    keep_r = ctx.radius_outliers(pts, 5, radius, workspace=ws)[0]
    # the exact pass alone, on m points: nothing resolves in the rings at cell 1/64
    m = min(a.exact_n, n)
    sub = pts[:m].contiguous()
    tiny = 1.0 / 64
    full = lambda: ctx.statistical_outliers(sub, 20, 2.0, tiny, 0, workspace=ws)
    grid = lambda: ctx.radius_outliers(sub, 5, tiny, workspace=ws)
    sent = int(full()[2][5].item())
    grid()
    tf, tg = [], []
    for _ in range(a.reps):
        tf.append(timed(full))
        tg.append(timed(grid))
    exact_ms = statistics.median(tf) - statistics.median(tg)
    ns_per_pair = exact_ms * 1e6 / (sent * m) if sent else float("nan")
    for c in cells:
        q = rings[f"cell{c}"]["exact_queries_at_max_rings_2"]
        rings[f"cell{c}"]["exact_pass_ms_estimate"] = round(q * n * ns_per_pair * 1e-6, 4)
    rec = {"bench": "outlier", "points": n, "extent_m": ext, "frames": B, "frame_stride": a.stride, "step": a.step,
           "reps": a.reps, "nb_neighbors": 20, "std_ratio": 2.0, "max_rings": 2, "radius": radius, "nb_points": 5,
           **res, "rings": rings,
           "statistical_stats_cell1": [float(v) for v in stats], "radius_kept": int(keep_r.sum().item()),
           "exact_pass_alone": {"points": m, "queries": sent, "ms": round(exact_ms, 4),
                                "ns_per_pair": round(ns_per_pair, 6)},
           "yardstick": "voxel_down_sample 0.32 ms per 1 M points (profiles/r1/bench_map.jsonl)"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
