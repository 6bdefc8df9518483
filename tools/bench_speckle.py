#!/usr/bin/env python3
"""Speckle filter beside SGBM on the GPU: B=64 synthetic 960x600 pairs, 96 disparities,
speckleWindowSize 100, speckleRange 2.  Per-kernel times (HIP events, fvo_timing_enable) of
sgbm_vert / sgbm_rows / sgbm_median and the four speckle kernels over the same disparity maps,
the filter's multiple of sgbm_median (one full-frame pass over the same buffer) and its share
of the in-order SGBM time:
    python tools/bench_speckle.py [--batch B] [--window N] [--range R] [--reps N] [--out FILE]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SGBM = ("sgbm_vert", "sgbm_rows", "sgbm_median")
SPECKLE = ("speckle_local", "speckle_seams", "speckle_sum", "speckle_apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--range", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from forest_slam_amd import _lib, synth
    B, W, H = a.batch, 960, 600
    seq = synth.StereoSequence(seed=0, n_frames=B, W=W, H=H, device="cuda")
    L, R = seq.frames(range(B))
    ctx = _lib.Context(W, H, max_batch=B, stages=_lib.STAGE_SGBM)
    disp = torch.empty((B, H, W), dtype=torch.int16, device="cuda")
    ws = torch.empty((ctx.speckle_workspace_bytes(B, H, W),), dtype=torch.uint8, device="cuda")
    new_val, max_diff = (int(ctx.cfg.min_disparity) - 1) * 16, 16 * a.range

    def once():
        ctx.sgbm(L, R, out=disp)
        ctx.filter_speckles(disp, new_val, a.window, max_diff, workspace=ws)

    ctx.sgbm(L, R, out=disp)
    raw = disp.clone()
    for _ in range(2):
        once()
    torch.cuda.synchronize()
    removed = int((disp != raw).sum().item())
    valid = int((raw != new_val).sum().item())
    ctx.timing_enable(None)
    for _ in range(a.reps):
        once()
    torch.cuda.synchronize()
    t = ctx.timing_read()
    ctx.timing_enable([])
    ms = {k: round(t[k][0] / a.reps, 4) for k in SGBM + SPECKLE if k in t}
    sgbm_ms = sum(ms[k] for k in SGBM)
    spk_ms = sum(ms[k] for k in SPECKLE if k in ms)
    rec = {"bench": "speckle", "batch": B, "size": [W, H], "num_disparities": int(ctx.cfg.num_disparities),
           "window": a.window, "range": a.range, "reps": a.reps, "kernels_ms": ms,
           "sgbm_ms": round(sgbm_ms, 4), "speckle_ms": round(spk_ms, 4),
           "speckle_over_median": round(spk_ms / ms["sgbm_median"], 3),
           "speckle_share_of_sgbm": round(spk_ms / sgbm_ms, 4),
           "valid_px": valid, "removed_px": removed, "workspace_mb": round(ws.numel() / 1e6, 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
