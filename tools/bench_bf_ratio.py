#!/usr/bin/env python3
"""Ratio-test matcher beside the cross-checked matcher on the GPU, at the benchmark's matcher
shape: 128 sets of 1000 x 1000 ORB-sized descriptors, capacity 1024.  Per-kernel times (HIP
events, fvo_timing_enable) of bf_argmin + bf_finish (fvo_bf_match) and of bf_knn + bf_ratio
(fvo_bf_ratio_match, mutual), the two calls alternating over the same descriptor sets:
    python tools/bench_bf_ratio.py [--batch B] [--n N] [--ratio R] [--reps N] [--out FILE]
Two thirds of the query rows are train rows with 0..89 flipped bits, the rest random.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROSS = ("bf_argmin", "bf_finish")
RATIO = ("bf_knn", "bf_ratio")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from forest_slam_amd import _lib
    B, n, cap = a.batch, a.n, -(-a.n // 1024) * 1024
    ctx = _lib.Context(64, 64, max_batch=B, stages=_lib.STAGE_BF, kp_capacity=cap)
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randint(0, 256, (B, cap, 32), dtype=torch.uint8, device="cuda", generator=g)
    q = torch.randint(0, 256, (B, cap, 32), dtype=torch.uint8, device="cuda", generator=g)
    ncopy = 2 * n // 3
    flips = torch.rand((B, ncopy, 256), device="cuda", generator=g) < (
        torch.randint(0, 90, (B, ncopy, 1), device="cuda", generator=g) / 256.0)
    weights = (1 << torch.arange(8, device="cuda")).to(torch.int32)
    mask = (flips.view(B, ncopy, 32, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)
    q[:, :ncopy] = t[:, :ncopy] ^ mask
    cnt = torch.full((B,), n, dtype=torch.int32, device="cuda")
    out_c = (torch.empty((B, cap, 3), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"))
    out_r = (torch.empty_like(out_c[0]), torch.empty_like(out_c[1]))

    def once():
        ctx.bf_match(q, cnt, t, cnt, out=out_c)
        ctx.bf_ratio_match(q, cnt, t, cnt, a.ratio, mutual=True, out=out_r)

    for _ in range(3):
        once()
    torch.cuda.synchronize()
    ctx.timing_enable(None)
    for _ in range(a.reps):
        once()
    torch.cuda.synchronize()
    tm = ctx.timing_read()
    ctx.timing_enable([])
    ms = {k: round(tm[k][0] / a.reps, 4) for k in CROSS + RATIO}
    cross_ms, ratio_ms = sum(ms[k] for k in CROSS), sum(ms[k] for k in RATIO)
    rec = {"bench": "bf_ratio", "batch": B, "n": n, "cap": cap, "ratio": a.ratio, "reps": a.reps, "kernels_ms": ms,
           "bf_match_ms": round(cross_ms, 4), "bf_ratio_match_ms": round(ratio_ms, 4),
           "ratio_over_match": round(ratio_ms / cross_ms, 3),
           "matches_per_set": round(float(out_c[1].float().mean().item()), 1),
           "ratio_matches_per_set": round(float(out_r[1].float().mean().item()), 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
