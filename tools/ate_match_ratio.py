#!/usr/bin/env python3
"""ATE of the stereo front end with and without the ratio test, on bench.py's ATE sequence
(synthetic forest, seed 100): one vo.run_sequence per match_ratio, evaluated by eval.ate
(Sim(3) alignment) against the sequence's ground truth.
    python tools/ate_match_ratio.py [--frames N] [--ratios 0,0.8] [--nfeatures N] [--ba-window K] [--out FILE]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--ratios", default="0,0.8")
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--ba-window", type=int, default=10)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from forest_slam_amd import eval as ev
    from forest_slam_amd import synth, vo
    W, H = a.width, a.height
    seq = synth.StereoSequence(seed=100, n_frames=a.frames, W=W, H=H, device="cuda")
    L, R = seq.frames(range(seq.n))
    gt = ev.tum_rows(seq.t, seq.T_wc)
    runs = []
    for ratio in (float(x) for x in a.ratios.split(",")):
        fe = vo.StereoFrontEnd(W, H, seq.K, synth.DIST_L, synth.BASELINE, batch=32, nfeatures=a.nfeatures,
                               ba_window=a.ba_window, match_ratio=ratio)
        rows, _, st = vo.run_sequence(fe, L, R, seq.t, use_ba=bool(a.ba_window))
        r = ev.ate(gt, rows)
        runs.append({"match_ratio": ratio, "ate_rmse_m": round(r["rmse"], 4), "poses": r["n"],
                     "pnp_failures": int((st == 0).sum()), "skipped": int((st == -1).sum())})
    rec = {"bench": "ate_match_ratio", "frames": int(seq.n), "size": [W, H], "nfeatures": a.nfeatures,
           "ba_window": a.ba_window, "runs": runs}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
