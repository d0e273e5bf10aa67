#!/usr/bin/env python3
"""Device time of hip_sad's intra test (include/ofps_hip.h N1i), median of 7 behind 2 warm-up calls, in one process on one GPU:
  off       with the test off: the search on bench.py's step (256 pairs, 1080p, 16x16, +-16) and on cfg4 (64 pairs, 4K, 8x8, +-32), HIP
            events on the context's stream, and the fused per-frame step of `frame` below.  With --lib the same rows run against another
            build of the library (the parent commit's): the yardstick for "ratio 0 enqueues exactly the parent's launches".  Run three fresh
            processes of each build, interleaved, and compare the worst median with the other's best.
  launch    ofps_hip_block_activity_dev alone on a 1080p frame at 16x16 (8,040 blocks) and a 4K frame at 8x8 (129,600 blocks), beside
            ofps_hip_block_contrast_dev on the same frames in the same process, and ofps_hip_sad_intra_dev (verdict + counters + cut veto) at
            the same lattices.  Launches of this size are shorter than an event pair's own resolution, so one sample is 200 launches back to
            back between two events, divided by 200: the time per launch of a saturated queue, launch overhead included -- not a kernel time.
  frame     the fused per-frame step (ofps_hip_push_frame, 1080p, 16x16, +-16, detector + least-squares estimator, records read back) at
            ratio 0, at ratio 8 and at ratio 8 with the cut rule at 50: host clock around calls that end in the ticket's wait, one sample is
            the mean of 24 frames.
  python tools/sad_intra_time.py [--lib <libofps_hip.so>] [--only off] [--out profiles/r18/run.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("ofps_hip_set_sad_intra", "ofps_hip_get_sad_intra", "ofps_hip_set_sad_cut", "ofps_hip_get_sad_cut", "ofps_hip_block_activity",
       "ofps_hip_block_activity_dev", "ofps_hip_sad_intra", "ofps_hip_sad_intra_dev", "ofps_hip_sad_flow_intra_dev")
if "--lib" in sys.argv:
    from ofps_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import ctypes
    import torch  # noqa: F401  (before the library: both then share one HIP runtime, as ofps_amd._lib.load does)
    for _name in NEW:                                    # a build from before the feature: ratio 0 only
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), _name):
            _lib.PROTOTYPES.pop(_name, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

STEPS = (("bench_step_1080p_16x16_r16_256pairs", 1920, 1080, 16, 16, 256), ("cfg4_4k_8x8_r32_64pairs", 3840, 2160, 8, 32, 64))
LATTICES = (("1080p_16x16_8040_blocks", 1920, 1080, 16), ("4k_8x8_129600_blocks", 3840, 2160, 8))
BURST, FRAMES = 200, 24


def _row(ts):
    return {"median_ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}


def median_ms(ctx, call, reps=7, warm=2, burst=1):
    ts = []
    for it in range(warm + reps):
        ctx.sync(); ctx.timer_start()
        for _ in range(burst):
            call()
        ms = ctx.timer_stop() / burst
        if it >= warm:
            ts.append(ms)
    return _row(ts)


def resident_batch(W, H, pairs, gen_pairs=8, max_step=8):
    fr = synth.luma_sequence(gen_pairs + 1, W, H, max_step=max_step)
    frames = np.ascontiguousarray(np.concatenate([fr] + [fr[1:]] * ((pairs + gen_pairs - 1) // gen_pairs - 1))[:pairs + 1])
    return torch.from_numpy(frames).cuda()


def batch_row(ctx, d, W, H, B, R, pairs):
    nblk = (W // B) * (H // B)
    o = torch.empty((pairs, nblk, 4), dtype=torch.float32, device="cuda")
    row = median_ms(ctx, lambda: ctx.sad_flow_dev(d.data_ptr(), pairs + 1, W, H, W, W * H, 0, B, R, o.data_ptr(), None))
    row["us_per_pair"] = round(row["median_ms"] * 1e3 / pairs, 3)
    return row


def launch_rows(ctx):
    out = {}
    rng = np.random.default_rng(3)
    for name, W, H, B in LATTICES:
        nblk = (W // B) * (H // B)
        d_frame = torch.from_numpy(synth.luma_sequence(2, W, H, max_step=8)[1]).cuda()
        d_act = torch.empty(nblk, dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(nblk, dtype=torch.int32, device="cuda")
        tri = np.zeros((nblk, 3), np.int32)
        tri[:, 2] = rng.integers(0, 4000, nblk)
        d_best = torch.from_numpy(tri).cuda()
        d_kin = torch.from_numpy((rng.random(nblk) < 0.8).astype(np.uint8)).cuda()
        d_keep = torch.empty(nblk, dtype=torch.uint8, device="cuda")
        d_two = torch.empty(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        out[name] = {
            "blocks": nblk, "launches_per_sample": BURST,
            "block_activity_dev": median_ms(ctx, lambda: ctx.block_activity_dev(d_frame.data_ptr(), W, H, W, B, d_act.data_ptr()), burst=BURST),
            "block_contrast_dev": median_ms(ctx, lambda: ctx.block_contrast_dev(d_frame.data_ptr(), W, H, W, B, d_cnt.data_ptr()), burst=BURST),
            "sad_intra_dev_cut50": median_ms(ctx, lambda: ctx.sad_intra_dev(d_best.data_ptr(), d_act.data_ptr(), d_kin.data_ptr(), W, H, B, 8, 50,
                                                                            d_keep.data_ptr(), d_two.data_ptr()), burst=BURST)}
        for k in ("block_activity_dev", "block_contrast_dev", "sad_intra_dev_cut50"):
            out[name][k]["us_per_launch"] = round(out[name][k]["median_ms"] * 1e3, 3)
        out[name]["block_activity_dev"]["frame_GB_per_s"] = round(W * H / (out[name]["block_activity_dev"]["median_ms"] * 1e-3) / 1e9, 1)
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


def frame_rows(ctx, has, only_off=False):
    frames = synth.luma_sequence(9, 1920, 1080, max_step=8)
    pin = ctx.pinned_frame(1080, 1920)
    out = {"intra0": frame_row(ctx, frames, pin)}
    if has and not only_off:
        ctx.set_sad_intra(8)
        out["intra8"] = frame_row(ctx, frames, pin)
        ctx.set_sad_cut(50)
        out["intra8_cut50"] = frame_row(ctx, frames, pin)
        ctx.set_sad_cut(0); ctx.set_sad_intra(0)
        for a in ("intra8", "intra8_cut50"):
            out[a]["added_ms_by_difference"] = round(out[a]["median_ms"] - out["intra0"]["median_ms"], 5)
    ctx.reset_frames()
    ctx.free_pinned(pin)
    return out


def main():
    only = set(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else None        # one section or a comma list
    want = lambda name: only is None or name in only
    ctx = HipContext(0)
    from ofps_amd import _lib
    has = "ofps_hip_set_sad_intra" in _lib.PROTOTYPES
    res = {"device": torch.cuda.get_device_name(0), "library": "--lib" if "--lib" in sys.argv else "in-tree", "intra_test_entry_points": has}
    if want("off"):
        ctx.use_torch_stream()
        res["off"] = {name: batch_row(ctx, resident_batch(W, H, pairs), W, H, B, R, pairs) for name, W, H, B, R, pairs in STEPS}
        ctx.use_own_stream()
        res["off"]["fused_frame_1080p_16x16_r16"] = frame_rows(ctx, has, only_off=True)["intra0"]
    if has and want("launch"):
        ctx.use_torch_stream()
        res["launch"] = launch_rows(ctx)
        ctx.use_own_stream()
    if has and want("frame"):
        res["frame"] = frame_rows(ctx, has)
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
