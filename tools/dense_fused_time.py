#!/usr/bin/env python3
"""Frame pushed -> island + quaternion on the host, for the dense decoders at 1080p: the fused form (ofps_hip_lk_push_frame_fused_async /
ofps_hip_lk_frame_fused_wait, records and their count stay on the device) against the stage-wise loop it replaces (lk_push_frame_async /
lk_frame_wait -> ofps_hip_detect + ofps_hip_almeida on the host records: a D2H + H2D round trip and two more waits per frame).  Both loops keep
two tickets in flight, frames come from page-locked memory.  hip_flow and hip_lk; the default 150 x 84 grid (luma) and the reduced mode (BGR);
least squares and RANSAC.  One JSON line: ms per frame, median of 7 timed runs (min, max) with CPython's collector held off.
  python tools/dense_fused_time.py [--frames N] [--mode fused|stagewise|both]
(--mode stagewise uses nothing but entry points older than the fused form: the same file measures an older checkout.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_legs import QuietGC, median_min_max  # noqa: E402
from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--mode", choices=("fused", "stagewise", "both"), default="both")
args = ap.parse_args()
N, W, H = args.frames, 1920, 1080
CAM = (16 / 9, 39.6 * 9 / 16)
DET = dict(min_size=0.05, subdivide=3, target_motion=0.003)

ctx = HipContext(0)
y = synth.flatten_regions(synth.luma_sequence(4, W, H, max_step=3, seed=11), region=96, seed=3)      # about half of every mask survives
bgr = np.clip(y[..., None].astype(int) + np.array([-20, 0, 15]), 0, 255).astype(np.uint8)
pins_y = [ctx.pinned_frame(H, W) for _ in range(4)]
pins_bgr = [ctx.pinned_frame(H, 3 * W).reshape(H, W, 3) for _ in range(4)]
for k in range(4):
    np.copyto(pins_y[k], y[k]); np.copyto(pins_bgr[k], bgr[k])
out = [np.zeros((150 * 150, 4), np.float32) for _ in range(2)]


def fused(frames, n, kw, est):
    prev, r = None, None
    for k in range(n):
        t = ctx.lk_push_frame_fused_async(frames[k % 4], **kw, **DET, aspect=CAM[0], fov_y_deg=CAM[1], seed=k, **est)
        if prev is not None:
            r = ctx.lk_frame_fused_wait(prev, want_entries=False, want_field=False)
        prev = t
    return ctx.lk_frame_fused_wait(prev, want_entries=False, want_field=False)["n_vectors"]


def stagewise(frames, n, kw, est):
    def tail(res):
        if res is None:
            return 0
        ctx.detect(res[0], **DET)
        ctx.almeida(res[0], *CAM, seed=0, **est)
        return len(res[0])
    prev, cnt = None, 0
    for k in range(n):
        t = ctx.lk_push_frame_async(frames[k % 4], **kw)
        if prev is not None:
            cnt = tail(ctx.lk_frame_wait(prev, out[k & 1]))
        prev = t
    return tail(ctx.lk_frame_wait(prev, out[n & 1]))


FLOW = dict(levels=5, radius=6, iters=3, farneback=True, use_previous=True, contrast_mask=True)
LK = dict(levels=3, radius=4, iters=3, contrast_mask=True)
LSQ, RANSAC = dict(use_ransac=False), dict(use_ransac=True, num_iters=200, inlier_deg=0.05, num_samples=1000)
rows = {}
loops = [m for m in ("fused", "stagewise") if args.mode in (m, "both")]
with QuietGC():
    for dec, base in (("hip_flow", FLOW), ("hip_lk", LK)):
        for grid, frames, kw in (("default_grid_luma", pins_y, dict(base)), ("reduced_bgr", pins_bgr, dict(base, reduced=True, fmt=ctx.FMT_BGR))):
            for solver, est in (("lsq", LSQ), ("ransac", RANSAC)):
                row = {}
                for name in loops:                         # interleaved: fused, stage-wise, fused, ... per configuration
                    fn = fused if name == "fused" else stagewise
                    ctx.lk_reset(); fn(frames, 8, kw, est)
                    vals = []
                    for _ in range(7):
                        t0 = time.perf_counter(); n_rec = fn(frames, N, kw, est); vals.append((time.perf_counter() - t0) / N * 1e3)
                    row[name] = dict(median_min_max(vals), records=int(n_rec))          # ms per frame
                rows[f"{dec}/{grid}/{solver}"] = row
ctx.lk_reset(); ctx.close()
print(json.dumps({"tool": "dense_fused_time", "geometry": [W, H], "frames": N, "runs": 7, "rows": rows}))
