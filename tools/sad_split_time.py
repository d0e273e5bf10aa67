#!/usr/bin/env python3
"""Device time of hip_sad's split step (include/ofps_hip.h N1s), median of 7 behind 2 warm-up samples, in one process on one GPU.  One pair
is shorter than an event pair resolves well, so one sample is BURST calls back to back between two events, divided by BURST: the time per
call of a saturated queue, launch overhead included.
  search    the plain one-pair search (ofps_hip_sad_flow_dev, 2 frames) at cfg2's geometry (1080p, 16x16, +-16) and cfg4's (4K, 8x8, +-32).
            With --lib the same rows run against another build of the library (the parent commit's): the yardstick beside the step.
  split     ofps_hip_sad_split_dev alone on the same pair, parents = that search's winners, T = 16, with and without raw records; the number
            of distinct predictors per block on this content (own winner, four neighbours, zero; host count) and the share of split blocks.
  flow      ofps_hip_sad_flow_split_dev (search + split + one compaction + count) beside the search alone.
  frame     the fused per-frame step (ofps_hip_push_frame, 1080p, 16x16, +-16, detector + least-squares estimator, records read back) at
            T = 0 and at T = --threshold: host clock around calls that end in the ticket's wait, one sample is the mean of 24 frames.
  islands   --islands: the detector's island area per frame on the clip with an independently moving object (tools/accuracy_clips.py's
            mixed_sine_dyn, 24 pairs) at T = 0 and at every T of --thresholds.
  python tools/sad_split_time.py [--lib <libofps_hip.so>] [--only search,split] [--threshold 16] [--out run.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("ofps_hip_set_sad_split", "ofps_hip_get_sad_split", "ofps_hip_sad_record_capacity", "ofps_hip_sad_split", "ofps_hip_sad_split_dev",
       "ofps_hip_sad_flow_split_dev")
if "--lib" in sys.argv:
    from ofps_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import ctypes
    import torch  # noqa: F401  (before the library: both then share one HIP runtime, as ofps_amd._lib.load does)
    for _name in NEW:                                    # a build from before the feature: the search rows only
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), _name):
            _lib.PROTOTYPES.pop(_name, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

GEOMETRIES = (("cfg2_1080p_16x16_r16", 1920, 1080, 16, 16), ("cfg4_4k_8x8_r32", 3840, 2160, 8, 32))
BURST, FRAMES = 50, 24


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


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
    row = _row(ts)
    row["us_per_call"] = round(row["median_ms"] * 1e3, 2)
    return row


def distinct_predictors(best, nbx, nby):
    """per block: the distinct vectors among its own winner, its lattice neighbours' (those that exist) and zero"""
    v = best[:, :2].reshape(nby, nbx, 2).astype(np.int64)
    key = v[..., 0] * 4096 + v[..., 1]
    out = np.zeros((nby, nbx), np.int64)
    for y in range(nby):
        for x in range(nbx):
            s = {0, int(key[y, x])}
            for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= x + ox < nbx and 0 <= y + oy < nby:
                    s.add(int(key[y + oy, x + ox]))
            out[y, x] = len(s)
    return out


def geometry_rows(ctx, has, T, want):
    out = {}
    for name, W, H, B, R in GEOMETRIES:
        nblk = (W // B) * (H // B)
        d = torch.from_numpy(np.ascontiguousarray(synth.luma_sequence(2, W, H, max_step=8))).cuda()
        d_ent = torch.empty((4 * nblk, 4), dtype=torch.float32, device="cuda")
        d_best = torch.empty((nblk, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        search = lambda: ctx.sad_flow_dev(d.data_ptr(), 2, W, H, W, W * H, 0, B, R, d_ent.data_ptr(), d_best.data_ptr())
        row = {"blocks": nblk, "calls_per_sample": BURST}
        if want("search"):
            row["search"] = median_ms(ctx, search)
        if has and (want("split") or want("flow")):
            search(); ctx.sync()
            best = d_best.cpu().numpy()
            d_sub = torch.empty((nblk, 12), dtype=torch.int32, device="cuda")
            d_split = torch.empty(nblk, dtype=torch.uint8, device="cuda")
            d_slot = torch.empty(4 * nblk, dtype=torch.uint8, device="cuda")
            d_cnt = torch.empty(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            step = lambda ent: ctx.sad_split_dev(d[0].data_ptr(), d[1].data_ptr(), W, H, W, B, d_best.data_ptr(), None, R, T, d_sub.data_ptr(),
                                                 d_split.data_ptr(), d_ent.data_ptr() if ent else None, d_slot.data_ptr() if ent else None)
            if want("split"):
                row["split_step"] = median_ms(ctx, lambda: step(True))
                row["split_step_without_records"] = median_ms(ctx, lambda: step(False))
                n = distinct_predictors(best, W // B, H // B)
                row["distinct_predictors_per_block"] = {"mean": round(float(n.mean()), 3), "histogram_1_to_6": [int((n == k).sum()) for k in range(1, 7)]}
                row["split_blocks_at_T"] = int(d_split.cpu().numpy().sum())
                if "search" in row:
                    row["split_step_over_search"] = round(row["split_step"]["median_ms"] / row["search"]["median_ms"], 4)
            if want("flow"):
                row["search_split_compact"] = median_ms(ctx, lambda: ctx.sad_flow_split_dev(d[0].data_ptr(), d[1].data_ptr(), W, H, W, B, R, 0, 0, 0, T,
                                                                                            d_ent.data_ptr(), d_cnt.data_ptr()))
                row["records_at_T"] = int(d_cnt.cpu().numpy()[0])
        out[name] = row
    return out


def frame_row(ctx, frames, pin, reps=7, warm=2):
    ts = []
    for it in range(warm + reps):
        ctx.reset_frames()
        np.copyto(pin, frames[0])
        ctx.push_frame(pin, 16, 16, want_entries=True)
        ctx.sync()
        t0 = time.perf_counter()
        for k in range(1, FRAMES + 1):
            np.copyto(pin, frames[k % len(frames)])
            ctx.push_frame(pin, 16, 16, want_entries=True)
        ms = (time.perf_counter() - t0) * 1e3 / FRAMES
        if it >= warm:
            ts.append(ms)
    row = _row(ts)
    row["frames_per_sample"] = FRAMES
    return row


def frame_rows(ctx, has, T):
    frames = synth.luma_sequence(9, 1920, 1080, max_step=8)
    pin = ctx.pinned_frame(1080, 1920)
    out = {"T0": frame_row(ctx, frames, pin)}
    if has:
        ctx.set_sad_split(T)
        out[f"T{T}"] = frame_row(ctx, frames, pin)
        out[f"T{T}"]["added_ms_by_difference"] = round(out[f"T{T}"]["median_ms"] - out["T0"]["median_ms"], 5)
        ctx.set_sad_split(0)
    ctx.reset_frames()
    ctx.free_pinned(pin)
    return out


def island_rows(ctx, thresholds):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import accuracy_clips as ac
    W, H, fov, eul, dis = ac.clip_table(quick=True)["mixed_sine_dyn"]
    frames, _ = synth.rotation_clip(eul, W, H, fov, seed=28, distractor=dis)
    pin = ctx.pinned_frame(H, W)
    out = {}
    for T in (0,) + tuple(thresholds):
        ctx.set_sad_split(T)
        ctx.reset_frames()
        areas, records = [], []
        for f in frames:
            np.copyto(pin, f)
            r = ctx.push_frame(pin, 16, 16, estimator=False)
            if r["have_vectors"]:
                areas.append(0 if r["motion"] is None else int(r["motion"][0]))
                records.append(r["n_vectors"])
        out[f"T{T}"] = {"mean_island_area_cells": round(float(np.mean(areas)), 2), "frames_with_island": int(np.count_nonzero(areas)),
                        "pairs": len(areas), "mean_records": round(float(np.mean(records)), 1)}
    ctx.set_sad_split(0)
    ctx.reset_frames()
    ctx.free_pinned(pin)
    return out


def main():
    only = set(_arg("--only", "").split(",")) - {""}
    want = lambda name: not only or name in only
    T = int(_arg("--threshold", "16"))
    ctx = HipContext(0)
    from ofps_amd import _lib
    has = "ofps_hip_set_sad_split" in _lib.PROTOTYPES
    res = {"device": torch.cuda.get_device_name(0), "library": "--lib" if "--lib" in sys.argv else "in-tree", "split_entry_points": has, "T": T}
    if want("search") or want("split") or want("flow"):
        ctx.use_torch_stream()
        res["geometry"] = geometry_rows(ctx, has, T, want)
        ctx.use_own_stream()
    if want("frame"):
        res["frame"] = frame_rows(ctx, has, T)
    if has and "--islands" in sys.argv:
        res["islands"] = island_rows(ctx, [int(t) for t in _arg("--thresholds", "8,16,32,64").split(",")])
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
