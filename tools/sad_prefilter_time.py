#!/usr/bin/env python3
"""Device time of hip_sad's mean removal (include/ofps_hip.h N1m), HIP events on the context's stream, median of 7 behind 2 warm-up calls,
in one process on one GPU:
  off       the search at radius 0 on bench.py's step (256 pairs, 1080p, 16x16, +-16) and on cfg4 (64 pairs, 4K, 8x8, +-32).  With --lib the
            same two rows run against another build of the library (the parent commit's): the yardstick for "radius 0 enqueues exactly the
            parent's launches".  Run three fresh processes of each build, interleaved, and compare the worst median with the other's best.
  filter    ofps_hip_sad_prefilter_dev alone, one launch on one 1080p and one 4K frame, at radius 4 and 8, beside its HBM floor: the bytes
            read + written over the achievable and the peak bandwidth of MI355X_MICROARCH.md (6.3 and 8 TB/s)
  step      the two steps of `off` at radius 0, 4 and 8, at levels 1 and 2: the whole step with and without the filter.  The batched filter
            launch (257 or 65 frames, grid z) has no entry point of its own: its time is the difference to radius 0 of the same row (the
            EXHAUSTIVE search's time does not depend on the content), set beside the floor of that many frames.
  python tools/sad_prefilter_time.py [--lib <libofps_hip.so>] [--only off] [--out profiles/r14/run.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("ofps_hip_set_sad_prefilter", "ofps_hip_get_sad_prefilter", "ofps_hip_sad_prefilter", "ofps_hip_sad_prefilter_dev")
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12
if "--lib" in sys.argv:
    from ofps_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import ctypes
    import torch  # noqa: F401  (before the library: both then share one HIP runtime, as ofps_amd._lib.load does)
    for _name in NEW:                                    # a build from before the feature: radius 0 only
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), _name):
            _lib.PROTOTYPES.pop(_name, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

RADII = (4, 8)
STEPS = (("bench_step_1080p_16x16_r16_256pairs", 1920, 1080, 16, 16, 256), ("cfg4_4k_8x8_r32_64pairs", 3840, 2160, 8, 32, 64))


def median_ms(ctx, call, reps=7, warm=2):
    ts = []
    for it in range(warm + reps):
        ctx.sync(); ctx.timer_start()
        call()
        ms = ctx.timer_stop()
        if it >= warm:
            ts.append(ms)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def resident_batch(W, H, pairs, gen_pairs=8, max_step=8):
    fr = synth.luma_sequence(gen_pairs + 1, W, H, max_step=max_step)
    frames = np.ascontiguousarray(np.concatenate([fr] + [fr[1:]] * ((pairs + gen_pairs - 1) // gen_pairs - 1))[:pairs + 1])
    return torch.from_numpy(frames).cuda()


def floor_us(W, H, frames):
    """bytes read (W x H) + written (rows of (W + 63) & ~63 bytes) per frame over the HBM bandwidth -> (achievable, peak) in microseconds"""
    b = frames * (W * H + ((W + 63) & ~63) * H)
    return {"bytes": b, "hbm_floor_us_at_6.3TBps": round(b / HBM_ACHIEVABLE * 1e6, 2), "hbm_floor_us_at_8TBps": round(b / HBM_PEAK * 1e6, 2)}


def batch_row(ctx, d, W, H, B, R, pairs, levels, radius):
    nblk = (W // B) * (H // B)
    o = torch.empty((pairs, nblk, 4), dtype=torch.float32, device="cuda")
    if levels != 1:
        ctx.set_sad_levels(levels)
    if radius:
        ctx.set_sad_prefilter(radius)
    row = median_ms(ctx, lambda: ctx.sad_flow_dev(d.data_ptr(), pairs + 1, W, H, W, W * H, 0, B, R, o.data_ptr(), None))
    if levels != 1:
        ctx.set_sad_levels(1)
    if radius:
        ctx.set_sad_prefilter(0)
    row["us_per_pair"] = round(row["median_ms"] * 1e3 / pairs, 3)
    return row


def filter_alone(ctx):
    out = {}
    for name, W, H in (("1080p", 1920, 1080), ("4k", 3840, 2160)):
        fr = resident_batch(W, H, 1, gen_pairs=1)
        dst = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        out[name] = {f"r{r}": median_ms(ctx, lambda: ctx.sad_prefilter_dev(fr.data_ptr(), W, H, W, r, dst.data_ptr(), W)) for r in RADII}
        out[name]["floor"] = floor_us(W, H, 1)
    return out


def main():
    only = set(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else None        # one section or a comma list
    want = lambda name: only is None or name in only
    ctx = HipContext(0)
    from ofps_amd import _lib
    has = "ofps_hip_set_sad_prefilter" in _lib.PROTOTYPES
    ctx.use_torch_stream()
    res = {"device": torch.cuda.get_device_name(0), "library": "--lib" if "--lib" in sys.argv else "in-tree", "mean_removal_entry_points": has}
    batches = {name: resident_batch(W, H, pairs) for name, W, H, _, _, pairs in STEPS}
    if want("off"):
        res["off"] = {name: batch_row(ctx, batches[name], W, H, B, R, pairs, 1, 0) for name, W, H, B, R, pairs in STEPS}
    if has and want("filter"):
        res["filter"] = filter_alone(ctx)
    if has and want("step"):
        res["step"] = {}
        for name, W, H, B, R, pairs in STEPS:
            rows = {}
            for levels in (1, 2):
                base = batch_row(ctx, batches[name], W, H, B, R, pairs, levels, 0)
                rows[f"levels{levels}_r0"] = base
                for r in RADII:
                    row = batch_row(ctx, batches[name], W, H, B, R, pairs, levels, r)
                    row["filter_ms_by_difference"] = round(row["median_ms"] - base["median_ms"], 4)
                    row["share_of_step"] = round(row["filter_ms_by_difference"] / row["median_ms"], 4)
                    rows[f"levels{levels}_r{r}"] = row
            rows["floor_of_the_batched_filter"] = floor_us(W, H, pairs + 1)
            res["step"][name] = rows
    ctx.use_own_stream()
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
