#!/usr/bin/env python3
"""Device time of hip_sad's search levels (include/ofps_hip.h N1h), HIP events on the context's stream, median of 7 behind 2 warm-up calls,
in one process on one GPU:
  levels1   the plain search at levels 1 on bench.py's step (256 pairs, 1080p, 16x16, +-16) and on cfg4 (64 pairs, 4K, 8x8, +-32).  With
            --lib the same two rows run against another build of the library (the parent commit's): the yardstick for "levels 1 enqueues
            exactly the parent's launches".  Run three fresh processes of each build, interleaved, and compare the min-max.
  pieces    ofps_hip_sad_down2_dev and ofps_hip_sad_refine_dev alone, one frame / one pair per launch, at 1080p block 16 and 4K block 8
  levels2   the same two geometries at levels 2 (1080p +-16, 4K +-32), for the same comparison against a build that has the levels
  cfg4      the cfg4 geometry (4K, 8x8, 64 pairs) at L 1 / R 32 (reach 32), L 2 / R 16 (reach 35), L 2 / R 32 (reach 67), L 3 / R 28 (reach 121)
--predictors {0,1}: the predictor mode (N1p) of `pieces` (ofps_hip_sad_refine_pred_dev), `levels2` and `cfg4`; 1 needs a build that has it.
--content {regions,camera}: bench.py's two generators; with mode 1 the duplicate skip makes the refinement's time depend on the content.
  python tools/sad_hier_time.py [--lib <libofps_hip.so>] [--only levels1] [--predictors 1] [--content camera] [--out profiles/r13/run.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("ofps_hip_set_sad_levels", "ofps_hip_get_sad_levels", "ofps_hip_sad_reach", "ofps_hip_sad_down2", "ofps_hip_sad_down2_dev", "ofps_hip_sad_refine",
       "ofps_hip_sad_refine_dev", "ofps_hip_set_sad_predictors", "ofps_hip_get_sad_predictors", "ofps_hip_sad_refine_pred", "ofps_hip_sad_refine_pred_dev")
PRED = int(sys.argv[sys.argv.index("--predictors") + 1]) if "--predictors" in sys.argv else 0
CONTENT = sys.argv[sys.argv.index("--content") + 1] if "--content" in sys.argv else "regions"
assert PRED in (0, 1) and CONTENT in ("regions", "camera")
if "--lib" in sys.argv:
    from ofps_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import ctypes
    import torch  # noqa: F401  (before the library: both then share one HIP runtime, as ofps_amd._lib.load does)
    for _name in NEW:                                    # a build from before the feature: levels 1 only
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), _name):
            _lib.PROTOTYPES.pop(_name, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402


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
    fr = synth.luma_sequence(gen_pairs + 1, W, H, max_step=max_step, **({} if CONTENT == "regions" else dict(region=1 << 14, noise=1)))
    frames = np.ascontiguousarray(np.concatenate([fr] + [fr[1:]] * ((pairs + gen_pairs - 1) // gen_pairs - 1))[:pairs + 1])
    return torch.from_numpy(frames).cuda()


def batch_row(ctx, d, W, H, B, R, pairs, levels):
    nblk = (W // B) * (H // B)
    o = torch.empty((pairs, nblk, 4), dtype=torch.float32, device="cuda")
    if levels != 1:
        ctx.set_sad_levels(levels)
        if PRED:
            ctx.set_sad_predictors(PRED)
    row = median_ms(ctx, lambda: ctx.sad_flow_dev(d.data_ptr(), pairs + 1, W, H, W, W * H, 0, B, R, o.data_ptr(), None))
    if levels != 1:
        ctx.set_sad_levels(1)
        if PRED:
            ctx.set_sad_predictors(0)
    row["us_per_pair"] = round(row["median_ms"] * 1e3 / pairs, 3)
    return row


def pieces(ctx):
    out = {}
    for name, W, H, B in (("1080p_b16", 1920, 1080, 16), ("4k_b8", 3840, 2160, 8)):
        fr = resident_batch(W, H, 1, gen_pairs=1)
        Wo, Ho = W >> 1, H >> 1
        so = (Wo + 63) & ~63
        half = torch.empty((Ho, so), dtype=torch.uint8, device="cuda")
        pnbx, pnby = Wo // B, Ho // B
        parent = torch.zeros((pnby, pnbx, 3), dtype=torch.int32, device="cuda")
        nblk = (W // B) * (H // B)
        best = torch.empty((nblk, 3), dtype=torch.int32, device="cuda")
        ent = torch.empty((nblk, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out[name] = {"down2_one_frame": median_ms(ctx, lambda: ctx.sad_down2_dev(fr.data_ptr(), W, H, W, half.data_ptr(), so)),
                     "refine_one_pair_level0": median_ms(ctx, (lambda: ctx.sad_refine_pred_dev(fr.data_ptr(), fr.data_ptr() + W * H, W, H, W, B, parent.data_ptr(),
                                                                                                  pnbx, pnby, 35, PRED, best.data_ptr(), ent.data_ptr())) if PRED else
                                                         (lambda: ctx.sad_refine_dev(fr.data_ptr(), fr.data_ptr() + W * H, W, H, W, B, parent.data_ptr(),
                                                                                     pnbx, pnby, 35, best.data_ptr(), ent.data_ptr()))),
                     "blocks": nblk}
    return out


def main():
    only = set(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else None        # one section or a comma list
    want = lambda name: only is None or name in only
    ctx = HipContext(0)
    from ofps_amd import _lib
    has_levels = "ofps_hip_set_sad_levels" in _lib.PROTOTYPES
    ctx.use_torch_stream()
    res = {"device": torch.cuda.get_device_name(0), "library": "--lib" if "--lib" in sys.argv else "in-tree", "search_levels_entry_points": has_levels,
           "predictors": PRED, "content": CONTENT}
    assert not PRED or "ofps_hip_set_sad_predictors" in _lib.PROTOTYPES, "--predictors 1 needs a library with ofps_hip_set_sad_predictors"
    d4k = resident_batch(3840, 2160, 64)
    if want("levels1"):
        d1080 = resident_batch(1920, 1080, 256)
        res["levels1"] = {"bench_step_1080p_16x16_r16_256pairs": batch_row(ctx, d1080, 1920, 1080, 16, 16, 256, 1),
                          "cfg4_4k_8x8_r32_64pairs": batch_row(ctx, d4k, 3840, 2160, 8, 32, 64, 1)}
        del d1080
    if has_levels and want("levels2"):
        d1080 = resident_batch(1920, 1080, 256)
        res["levels2"] = {"bench_step_1080p_16x16_r16_256pairs": batch_row(ctx, d1080, 1920, 1080, 16, 16, 256, 2),
                          "cfg4_4k_8x8_r32_64pairs": batch_row(ctx, d4k, 3840, 2160, 8, 32, 64, 2)}
        del d1080
    if has_levels and want("pieces"):
        res["pieces"] = pieces(ctx)
    if has_levels and want("cfg4"):
        res["cfg4_4k_8x8_64pairs"] = {f"L{levels}_R{R}_reach{ctx.sad_reach(R, levels)}": batch_row(ctx, d4k, 3840, 2160, 8, R, 64, levels)
                                       for levels, R in ((1, 32), (2, 16), (2, 32), (3, 28))}
    ctx.use_own_stream()
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
