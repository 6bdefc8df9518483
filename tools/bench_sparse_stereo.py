#!/usr/bin/env python3
"""Sparse stereo on the GPU (fvo_sparse_stereo) against the dense path it replaces in the front end.

stage      HIP events over B=64 synthetic 960x600 pairs with 1000 features (the GPU's own ORB):
           fvo_sparse_stereo against fvo_sgbm + fvo_keypoint_stereo on the same pairs, the two
           alternated call by call in one process; ms per 64 pairs (median, min, max).
front_end  frames/s and workspace of StereoFrontEnd(depth="sparse") against the default, through
           bench.py's loop (SequenceRank.step over the ping-pong batches, overlap_sgbm, local BA
           K=10), --runs runs of each, interleaved.
accuracy   ATE (Sim(3)-aligned RMSE, eval.ate) of both modes on bench.py's 200-frame synthetic
           sequence; no threshold.
    python tools/bench_sparse_stereo.py [--batch B] [--reps N] [--runs R] [--steps K] [--ate-frames F]
                                        [--out profiles/sparse_stereo/bench_sparse_stereo.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(ms, scale):
    return {"median": round(statistics.median(ms) * scale, 4), "min": round(min(ms) * scale, 4),
            "max": round(max(ms) * scale, 4)}


def stage(B, W, H, nfeatures, reps):
    from forest_slam_amd import _lib, synth
    seq = synth.StereoSequence(seed=0, n_frames=B, W=W, H=H, device="cuda")
    L, R = seq.frames(range(B))
    ctx = _lib.Context(W, H, max_batch=2 * B, nfeatures=nfeatures, sgbm_max_batch=B,
                       stages=_lib.STAGE_ORB | _lib.STAGE_BF | _lib.STAGE_SGBM | _lib.STAGE_BA)
    kp, desc, cnt = ctx.orb(torch.cat([L, R]))
    cap = ctx.kp_cap
    disp = torch.empty((B, H, W), dtype=torch.int16, device="cuda")
    dense_rec = torch.empty((B, cap, 4), dtype=torch.float32, device="cuda")
    sparse_rec = torch.zeros((B, cap, 4), dtype=torch.float32, device="cuda")
    info = torch.zeros((B, cap, 4), dtype=torch.int32, device="cuda")
    ws = torch.empty((ctx.sparse_stereo_workspace_bytes(B, cap),), dtype=torch.uint8, device="cuda")
    params = ctx.sparse_stereo_params()
    scales = ctx.level_scales()

    def sgbm():
        ctx.sgbm(L, R, out=disp)

    def kstereo():
        ctx.keypoint_stereo(disp, kp[:B], cnt[:B], seq.K, synth.BASELINE, out=dense_rec)

    def sparse(inf=None):
        ctx.sparse_stereo(L, R, kp[:B], cnt[:B], desc[:B], kp[B:], cnt[B:], desc[B:], seq.K, synth.BASELINE,
                          params=params, level_scale=scales, workspace=ws, out=sparse_rec, info=inf)

    for _ in range(3):
        sgbm()
        kstereo()
        sparse()
    torch.cuda.synchronize()
    t = {"sgbm": [], "keypoint_stereo": [], "sparse_stereo": []}
    for _ in range(reps):  # alternated, so that both see the same clocks and neighbours
        t["sgbm"].append(_ms(sgbm))
        t["keypoint_stereo"].append(_ms(kstereo))
        t["sparse_stereo"].append(_ms(sparse))
    sparse(info)
    torch.cuda.synchronize()
    n = cnt[:B].clamp(min=0).cpu().numpy()
    st = info.cpu().numpy()[..., 3]
    hist = np.zeros(7, np.int64)
    for b in range(B):
        hist += np.bincount(st[b, :n[b]], minlength=7)
    dz, sz = dense_rec.cpu().numpy()[..., 2], sparse_rec.cpu().numpy()[..., 2]
    both = sum(int(((dz[b, :n[b]] != 0) & (sz[b, :n[b]] != 0)).sum()) for b in range(B))
    k = 64.0 / B
    dense_ms = [a + b for a, b in zip(t["sgbm"], t["keypoint_stereo"])]
    return {"batch": B, "size": [W, H], "nfeatures": nfeatures, "reps": reps, "keypoints_per_left_image": float(n.mean()),
            "ms_per_64_pairs": {"sparse_stereo": _stats(t["sparse_stereo"], k), "sgbm": _stats(t["sgbm"], k),
                                "keypoint_stereo": _stats(t["keypoint_stereo"], k),
                                "sgbm_plus_keypoint_stereo": _stats(dense_ms, k)},
            "ratio_dense_over_sparse": round(statistics.median(dense_ms) / statistics.median(t["sparse_stereo"]), 2),
            "status_counts": hist.tolist(), "points_per_pair": {"sparse": round(hist[0] / B, 1),
                                                               "dense": round(float((dz != 0).sum()) / B, 1),
                                                               "both": round(both / B, 1)}}


def front_end(B, W, H, nfeatures, runs, steps, warmup):
    from forest_slam_amd import dist as fdist
    from forest_slam_amd import synth, vo
    seq = synth.StereoSequence(seed=0, n_frames=B + 1, W=W, H=H, device="cuda")
    L_all, R_all = seq.frames(range(B + 1))
    torch.cuda.synchronize()
    fwd = (L_all[1:].contiguous(), R_all[1:].contiguous())
    bwd = (L_all[:B].flip(0).contiguous(), R_all[:B].flip(0).contiguous())
    out = {}
    rigs = {}
    for depth in ("sgbm", "sparse"):
        fe = vo.StereoFrontEnd(W, H, seq.K, synth.DIST_L, synth.BASELINE, batch=B, nfeatures=nfeatures, ba_window=10,
                               overlap_sgbm=True, depth=depth)
        fe.prime(L_all[0], R_all[0])
        total = runs * (steps + warmup) + 2
        rigs[depth] = (fe, fdist.SequenceRank(fe, map_capacity=total * B * fe.cap), [0])
        out[depth] = {"workspace_gb": round(fe.ctx.workspace_bytes / 1e9, 2), "frames_per_s": []}

    def step(depth):
        fe, rank, k = rigs[depth]
        Lb, Rb = fwd if k[0] % 2 == 0 else bwd
        k[0] += 1
        return rank.step(Lb, Rb)

    for _ in range(runs):  # interleaved: sgbm, sparse, sgbm, sparse, ...
        for depth in ("sgbm", "sparse"):
            for _ in range(warmup):
                step(depth)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                last = step(depth)
            torch.cuda.synchronize()
            out[depth]["frames_per_s"].append(round(steps * B / (time.perf_counter() - t0), 1))
            out[depth]["valid_poses_last_step"] = int((last[1] == 1).sum().item())
    out["loop"] = {"batch": B, "steps": steps, "warmup": warmup, "runs": runs, "ba_window": 10, "overlap_sgbm": 1}
    return out


def accuracy(W, H, nfeatures, frames):
    from forest_slam_amd import eval as ev
    from forest_slam_amd import synth, vo
    seq = synth.StereoSequence(seed=100, n_frames=frames, W=W, H=H, device="cuda")
    La, Ra = seq.frames(range(seq.n))
    gt = ev.tum_rows(seq.t, seq.T_wc)
    out = {"frames": int(seq.n)}
    for depth in ("sgbm", "sparse"):
        fe = vo.StereoFrontEnd(W, H, seq.K, synth.DIST_L, synth.BASELINE, batch=32, nfeatures=nfeatures, ba_window=10,
                               depth=depth)
        rows, _, st = vo.run_sequence(fe, La, Ra, seq.t, use_ba=True)
        rows_p, _, _ = vo.run_sequence(fe, La, Ra, seq.t, use_ba=False)
        out[depth] = {"ate_rmse_m": round(ev.ate(gt, rows)["rmse"], 4),
                      "ate_rmse_m_pnp_only": round(ev.ate(gt, rows_p)["rmse"], 4),
                      "pnp_failures": int((st == 0).sum()), "skipped": int((st == -1).sum())}
        del fe
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ate-frames", type=int, default=200, help="0 = skip the accuracy leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_stereo", "bench_sparse_stereo.json"))
    a = ap.parse_args()
    W, H, N = 960, 600, 1000
    rec = {"bench": "sparse_stereo", "stage": stage(a.batch, W, H, N, a.reps)}
    torch.cuda.empty_cache()
    rec["front_end"] = front_end(a.batch, W, H, N, a.runs, a.steps, a.warmup)
    torch.cuda.empty_cache()
    if a.ate_frames > 1:
        rec["accuracy"] = accuracy(W, H, N, a.ate_frames)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
