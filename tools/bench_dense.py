#!/usr/bin/env python3
"""Dense stereo mapping on the GPU (fvo_dense_map_append): the disparity maps of B=64 synthetic
960x600 pairs (StereoSGBM, 96 disparities) appended to a map as a world-frame point cloud, at
step 1 (8-byte loads) and step 4 (scalar loads), min_disp16 1, 0.1 < Z < 1000.  Each call is
timed with HIP events on its stream (count reset outside the events); reported per step: ms per
64 frames (median and min over --reps calls), emitted points, and achieved bytes per second
counting 2 B per sample read in each of the two passes plus 36 B per emitted point (fp64 + float32
records).  Yardstick: k_map_xform's recorded 3.8 TB/s (profiles/r1/bench_map.jsonl).
    python tools/bench_dense.py [--batch B] [--reps N] [--out profiles/dense/bench_dense.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense", "bench_dense.json"))
    a = ap.parse_args()
    from forest_slam_amd import _lib, synth
    B, W, H = a.batch, 960, 600
    seq = synth.StereoSequence(seed=0, n_frames=B, W=W, H=H, device="cuda")
    L, R = seq.frames(range(B))
    ctx = _lib.Context(W, H, max_batch=B, stages=_lib.STAGE_SGBM)
    disp = ctx.sgbm(L, R)
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    T = np.tile(np.eye(4), (B, 1, 1))
    T[:, :3, 3] = rng.uniform(-50, 50, (B, 3))
    T = torch.from_numpy(T).cuda()
    cap = B * H * W
    m64 = torch.empty((cap, 3), dtype=torch.float64, device="cuda")
    m32 = torch.empty((cap, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    n_added = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ws = torch.empty((ctx.dense_workspace_bytes(B, H, W, 1),), dtype=torch.uint8, device="cuda")
    steps = {}
    for step in (1, 4):
        def once():
            ctx.dense_map_append(disp, seq.K, synth.BASELINE, T, cnt, m64, m32, step=step, n_added=n_added,
                                 workspace=ws)
        for _ in range(3):
            cnt.zero_()
            once()
        torch.cuda.synchronize()
        points = int(cnt.item())
        ms = []
        for _ in range(a.reps):
            cnt.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            once()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        samples = B * ((H - 1) // step + 1) * ((W - 1) // step + 1)
        nbytes = 2 * 2 * samples + 36 * points
        med = statistics.median(ms)
        steps[f"step{step}"] = {"ms_per_64_frames": round(med * 64 / B, 4), "ms_min": round(min(ms) * 64 / B, 4),
                                "samples": samples, "points": points, "bytes": nbytes,
                                "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
    rec = {"bench": "dense", "batch": B, "size": [W, H], "num_disparities": int(ctx.cfg.num_disparities),
           "reps": a.reps, "min_disp16": 1, "z_range": [0.1, 1000.0], **steps,
           "yardstick": "map_transform 3.8 TB/s (profiles/r1/bench_map.jsonl)"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
