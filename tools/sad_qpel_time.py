#!/usr/bin/env python3
"""Device time of the SAD search with and without the quarter-pel refinement (motion scale 1 and 4, include/ofps_hip.h N1q), in one
process on one GPU: the 256-pair 1080p 16x16 +-16 resident batch (bench.py's step) and the 64-pair 4K 8x8 +-32 batch (cfg4), HIP events,
median of 7; and the per-frame push_frame p50 (the cfg5 shape: SAD + detector + LSQ estimator per 1080p frame) both ways, reported only.
With --lib the same measurement runs against another build of the library (the parent commit's, for the scale-1 yardstick).
  python tools/sad_qpel_time.py [--lib <libofps_hip.so>] [--out profiles/r07/sad_qpel_time.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--lib" in sys.argv:
    from ofps_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import ctypes
    import torch  # noqa: F401  (before the library: both then share one HIP runtime, as ofps_amd._lib.load does)
    for _name in ("ofps_hip_set_sad_motion_scale", "ofps_hip_get_sad_motion_scale"):     # a build from before the feature: scale 1 only
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), _name):
            _lib.PROTOTYPES.pop(_name, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402


def batch_ms(ctx, W, H, B, R, pairs, gen_pairs, scales):
    fr = synth.luma_sequence(gen_pairs + 1, W, H, max_step=min(R, 8))
    frames = np.ascontiguousarray(np.concatenate([fr] + [fr[1:]] * ((pairs + gen_pairs - 1) // gen_pairs - 1))[:pairs + 1])
    d = torch.from_numpy(frames).cuda()
    nblk = (W // B) * (H // B)
    o = torch.empty((pairs, nblk, 4), dtype=torch.float32, device="cuda")
    out = {}
    for scale in scales:
        if scale != 1:
            ctx.set_sad_motion_scale(scale)
        ts = []
        for it in range(2 + 7):
            ctx.sync(); ctx.timer_start()
            ctx.sad_flow_dev(d.data_ptr(), pairs + 1, W, H, W, W * H, 0, B, R, o.data_ptr(), None)
            ms = ctx.timer_stop()
            if it >= 2:
                ts.append(ms)
        out[f"scale{scale}_ms"] = round(statistics.median(ts), 4)
        out[f"scale{scale}_us_per_pair"] = round(statistics.median(ts) * 1e3 / pairs, 3)
    if 4 in scales:
        ctx.set_sad_motion_scale(1)
        out["scale4_over_scale1"] = round(out["scale4_ms"] / out["scale1_ms"], 4)
    return out


def push_p50_ms(ctx, scale, frames=120):
    W, H = 1920, 1080
    fr = synth.luma_sequence(8, W, H, max_step=8)
    if scale != 1:
        ctx.set_sad_motion_scale(scale)
    ctx.reset_frames()
    buf = ctx.pinned_frame(H, W)
    ts = []
    for k in range(frames):
        np.copyto(buf, fr[k % 8])
        t0 = time.perf_counter()
        ctx.push_frame(buf, 16, 16, detector=True, estimator=True)
        ts.append((time.perf_counter() - t0) * 1e3)
    if scale != 1:
        ctx.set_sad_motion_scale(1)
    return round(statistics.median(ts[10:]), 4)


def main():
    ctx = HipContext(0)
    from ofps_amd import _lib
    has_qpel = "ofps_hip_set_sad_motion_scale" in _lib.PROTOTYPES
    scales = (1, 4) if has_qpel else (1,)
    ctx.use_torch_stream()
    res = {"device": torch.cuda.get_device_name(0), "library": "--lib" if "--lib" in sys.argv else "in-tree", "quarter_pel_entry_points": has_qpel,
           "1080p_16x16_r16_256pairs": batch_ms(ctx, 1920, 1080, 16, 16, 256, 8, scales),
           "cfg4_4k_8x8_r32_64pairs": batch_ms(ctx, 3840, 2160, 8, 32, 64, 8, scales)}
    ctx.use_own_stream()
    res["push_frame_1080p_p50_ms"] = {f"scale{s}": push_p50_ms(ctx, s) for s in scales}
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
