#!/usr/bin/env python3
"""Per-frame time of the batched stream form with hip_sad's gate, consistency check and median test (include/ofps_hip.h N1b), median of 7
behind 2 warm-up samples, in one process on one GPU.  1080p, 16x16, +-16, detector + least-squares estimator, records read back, frames and
records in page-locked memory; host clock around calls that end in the last ticket's wait.
  batched   ofps_hip_push_frames_async, 16 frames per ticket, two tickets in flight, one sample = 8 tickets = 128 frames, with the batch
            filter switch on at: off, gate 1, median 2, gate 1 + median 2, check 1, all three.
  single    the same 128 frames as single ofps_hip_push_frame_async pushes, two in flight, at the same settings in the same process: what a
            caller has without the switch -- the baseline.
  off       (also the only section with --lib <another build's libofps_hip.so>, the parent commit's) the batched row with every criterion
            off and the switch off, and bench.py's search step (256 pairs, 1080p, 16x16, +-16) on HIP events: the yardstick for "with the
            switch at 0 every batched entry point enqueues what the parent enqueues".  Run three fresh processes of each build, interleaved.
  --trace N pushes 3 tickets of N frames with all three criteria on and exits: the program for one `rocprofv3 --kernel-trace` listing
            (the launches per ticket must not depend on N).
  python tools/sad_batch_filter_time.py [--lib <libofps_hip.so>] [--only off] [--trace N] [--out profiles/r16/run.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("ofps_hip_sad_flow_filtered_dev", "ofps_hip_set_sad_batch_filter", "ofps_hip_get_sad_batch_filter")
if "--lib" in sys.argv:
    from ofps_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import ctypes
    import torch  # noqa: F401  (before the library: both then share one HIP runtime, as ofps_amd._lib.load does)
    for _name in NEW:                                    # a build from before the feature: the off rows only
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), _name):
            _lib.PROTOTYPES.pop(_name, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

W, H, B, R = 1920, 1080, 16, 16
NBLK = (W // B) * (H // B)
PER_TICKET, TICKETS = 16, 8
SETTINGS = (("off", 0, 0, 0), ("gate1", 1, 0, 0), ("median2", 0, 0, 2), ("gate1_median2", 1, 0, 2), ("check1", 0, 1, 0), ("all_three", 1, 1, 2))


def _row(ts):
    return {"median_ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}


def _apply(ctx, gate, check, median):
    ctx.set_sad_gate(gate); ctx.set_sad_consistency(check); ctx.set_sad_median(median)


def batched_row(ctx, bufs, ents, n=PER_TICKET, tickets=TICKETS, reps=7, warm=2):
    """per-frame ms; bufs / ents: two page-locked [n, H, W] / [n, NBLK, 4] blocks that alternate"""
    ts = []
    for it in range(warm + reps):
        ctx.reset_frames()
        ctx.frames_wait(ctx.push_frames_async(bufs[0][:1], B, R, out_entries=ents[0][:1]))       # the stream's first frame: no pair
        t0 = time.perf_counter()
        pending = []
        for k in range(tickets):
            if len(pending) == 2:
                ctx.frames_wait(pending.pop(0))
            pending.append(ctx.push_frames_async(bufs[k % 2], B, R, out_entries=ents[k % 2]))
        for t in pending:
            ctx.frames_wait(t)
        ms = (time.perf_counter() - t0) * 1e3 / (tickets * n)
        if it >= warm:
            ts.append(ms)
    ctx.reset_frames()
    row = _row(ts)
    row["frames_per_sample"] = tickets * n
    return row


def single_row(ctx, bufs, ents, n=PER_TICKET, tickets=TICKETS, reps=7, warm=2):
    ts = []
    for it in range(warm + reps):
        ctx.reset_frames()
        ctx.frame_wait(ctx.push_frame_async(bufs[0][0], B, R, out_entries=ents[0][0]))
        t0 = time.perf_counter()
        pending = []
        for k in range(tickets * n):
            if len(pending) == 2:
                ctx.frame_wait(pending.pop(0))
            j = k % (2 * n)
            pending.append(ctx.push_frame_async(bufs[j // n][j % n], B, R, out_entries=ents[j // n][j % n]))
        for t in pending:
            ctx.frame_wait(t)
        ms = (time.perf_counter() - t0) * 1e3 / (tickets * n)
        if it >= warm:
            ts.append(ms)
    ctx.reset_frames()
    row = _row(ts)
    row["frames_per_sample"] = tickets * n
    return row


def step_row(ctx, pairs=256, reps=7, warm=2):
    fr = synth.luma_sequence(9, W, H, max_step=8)
    frames = np.ascontiguousarray(np.concatenate([fr] + [fr[1:]] * (pairs // 8 - 1))[:pairs + 1])
    d = torch.from_numpy(frames).cuda()
    o = torch.empty((pairs, NBLK, 4), dtype=torch.float32, device="cuda")
    ts = []
    for it in range(warm + reps):
        ctx.sync(); ctx.timer_start()
        ctx.sad_flow_dev(d.data_ptr(), pairs + 1, W, H, W, W * H, 0, B, R, o.data_ptr(), None)
        ms = ctx.timer_stop()
        if it >= warm:
            ts.append(ms)
    row = _row(ts)
    row["us_per_pair"] = round(row["median_ms"] * 1e3 / pairs, 3)
    return row


def blocks(ctx, n):
    fr = synth.luma_sequence(2 * n, W, H, max_step=8)
    bufs = [ctx.pinned_array((n, H, W), np.uint8) for _ in range(2)]
    ents = [ctx.pinned_array((n, NBLK, 4)) for _ in range(2)]
    for k in range(2):
        np.copyto(bufs[k], fr[k * n:(k + 1) * n])
    return bufs, ents


def trace(ctx, n):
    bufs, ents = blocks(ctx, n)
    ctx.set_sad_batch_filter(1)
    _apply(ctx, 1, 1, 2)
    ctx.frames_wait(ctx.push_frames_async(bufs[0][:1], B, R, out_entries=ents[0][:1]))
    for k in range(3):
        res = ctx.frames_wait(ctx.push_frames_async(bufs[k % 2], B, R, out_entries=ents[k % 2]))
        print(f"ticket {k}: {n} frames, kept", [r["n_vectors"] for r in res])
    ctx.close()


def main():
    only = set(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else None
    want = lambda name: only is None or name in only
    ctx = HipContext(0)
    if "--trace" in sys.argv:
        return trace(ctx, int(sys.argv[sys.argv.index("--trace") + 1]))
    from ofps_amd import _lib
    has = "ofps_hip_set_sad_batch_filter" in _lib.PROTOTYPES
    res = {"device": torch.cuda.get_device_name(0), "library": "--lib" if "--lib" in sys.argv else "in-tree", "batch_filter_entry_points": has,
           "geometry": f"{W}x{H} {B}x{B} +-{R}, {PER_TICKET} frames per ticket"}
    bufs, ents = blocks(ctx, PER_TICKET)
    if want("off"):
        ctx.use_torch_stream()
        res["off"] = {"bench_step_1080p_16x16_r16_256pairs": step_row(ctx)}
        ctx.use_own_stream()
        res["off"]["batched_per_frame"] = batched_row(ctx, bufs, ents)
    if has and want("price"):
        res["price"] = {}
        for name, gate, check, median in SETTINGS:
            _apply(ctx, gate, check, median)
            ctx.set_sad_batch_filter(1)
            b = batched_row(ctx, bufs, ents)
            ctx.set_sad_batch_filter(0)
            s = single_row(ctx, bufs, ents)
            res["price"][name] = {"batched_per_frame": b, "single_pushes_per_frame": s,
                                  "batched_over_single": round(b["median_ms"] / s["median_ms"], 3)}
        _apply(ctx, 0, 0, 0)
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
