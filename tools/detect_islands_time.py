#!/usr/bin/env python3
"""Device time of the island list (include/ofps_hip.h A5i) beside the detector's, in one process on one GPU, median of 7 behind 2 warm-up
samples.  The launches are shorter than an event pair's own resolution, so one sample is 200 calls back to back between two HIP events on
the context's stream, divided by 200: the time per call of a saturated queue, launch overhead included -- not a kernel time.  Every call is
densify + one kernel, so three rows per size: ofps_hip_densify_dev alone, ofps_hip_detect_dev (densify + detect_kernel) and
ofps_hip_detect_islands_dev (densify + islands_kernel); the two steps are the differences.
  dim 14   8,040 records (a 1080p frame's 16 x 16 blocks), the plugin's default grid, K = 16
  dim 160  one record per cell, the 6,400-island lattice of tests/detect_cases.py (area 1 qualifies: min_size = 1 / 160^2), K = 16 and 6400
  frame    the fused per-frame step (ofps_hip_push_frame, 1080p, 16 x 16, +-16, detector + least-squares estimator) at K = 0 and K = 16: host
           clock around calls that end in the ticket's wait, one sample is the mean of 24 frames
  python tools/detect_islands_time.py [--out run.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

BURST, FRAMES = 200, 24
TARGET = 0.003


def _row(ts):
    return {"median_ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}


def median_ms(ctx, call, reps=7, warm=2, burst=BURST):
    ts = []
    for it in range(warm + reps):
        ctx.sync(); ctx.timer_start()
        for _ in range(burst):
            call()
        ms = ctx.timer_stop() / burst
        if it >= warm:
            ts.append(ms)
    return _row(ts)


def lattice_records(d):
    """one record per cell; the cells (2i, 2j) move"""
    p = np.clip(np.arange(d, dtype=np.float32) / np.float32(d - 1), 1e-4, 1 - 1e-4).astype(np.float32)
    ys, xs = np.mgrid[0:d, 0:d]
    e = np.zeros((d * d, 4), np.float32)
    e[:, 0], e[:, 1] = p[xs.reshape(-1)], p[ys.reshape(-1)]
    e[((xs % 2 == 0) & (ys % 2 == 0)).reshape(-1), 2] = 0.01
    return e


def stage_rows(ctx, name, e, min_size, subdivide, ks):
    d = ctx.block_dim(min_size, subdivide)
    n = e.shape[0]
    d_ent = torch.from_numpy(e.reshape(-1)).cuda()
    d_fld = torch.zeros(2 * d * d, dtype=torch.float32, device="cuda")
    d_res = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_lab = torch.zeros(d * d, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    out = {"dim": d, "records": n}
    out["densify"] = median_ms(ctx, lambda: ctx.densify_dev(d_ent.data_ptr(), n, 1, d, d, d_fld.data_ptr()))
    out["detect"] = median_ms(ctx, lambda: ctx.detect_dev(d_ent.data_ptr(), n, 1, min_size, subdivide, TARGET, d_res.data_ptr(), d_fld.data_ptr()))
    out["detect_kernel_us"] = round((out["detect"]["median_ms"] - out["densify"]["median_ms"]) * 1e3, 2)
    for K in ks:
        d_tab = torch.zeros(8 * K, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        row = median_ms(ctx, lambda: ctx.detect_islands_dev(d_ent.data_ptr(), n, 1, min_size, subdivide, TARGET, K, d_cnt.data_ptr(), d_tab.data_ptr(),
                                                            d_lab.data_ptr(), d_fld.data_ptr()))
        ctx.sync()
        row["islands_kernel_us"] = round((row["median_ms"] - out["densify"]["median_ms"]) * 1e3, 2)
        row["counts"] = d_cnt.cpu().numpy().tolist()
        out[f"islands_K{K}"] = row
    return {name: out}


def frame_rows(ctx):
    W, H = 1920, 1080
    fr = synth.luma_sequence(FRAMES + 1, W, H, max_step=8)
    pin = ctx.pinned_frame(H, W)
    out = {}
    for K in (0, 16, 0, 16):
        ctx.set_detect_islands(K)
        ts = []
        for it in range(2 + 7):
            ctx.reset_frames()
            np.copyto(pin, fr[0]); ctx.push_frame(pin, block=16, search_range=16)
            t0 = time.perf_counter()
            for k in range(1, FRAMES + 1):
                np.copyto(pin, fr[k])
                ctx.push_frame(pin, block=16, search_range=16, seed=k)
            if it >= 2:
                ts.append((time.perf_counter() - t0) * 1e3 / FRAMES)
        out.setdefault(f"K{K}", []).append(_row(ts))
    ctx.set_detect_islands(0)
    return {"frame_1080p_16x16_r16_lsq_ms_per_frame": out}


def main():
    ctx = HipContext(0)
    res = {}
    rng = np.random.default_rng(5)
    e14 = np.empty((8040, 4), np.float32)
    e14[:, :2] = rng.uniform(0.001, 0.999, (8040, 2))
    e14[:, 2:] = rng.normal(0.003, 0.002, (8040, 2))
    res.update(stage_rows(ctx, "dim14_8040_records", e14, 0.05, 3, (16,)))
    res.update(stage_rows(ctx, "dim160_lattice_6400_islands", lattice_records(160), float(np.float32(1.0 / 160 ** 2)), 1, (16, 6400)))
    res.update(frame_rows(ctx))
    text = json.dumps(res, indent=1)
    print(text)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
