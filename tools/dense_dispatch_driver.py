#!/usr/bin/env python3
"""The program for a `rocprofv3 --kernel-trace` listing of the dense decoders' host paths (dense_decoder.hip), and the bytes they return: for
a change that must move neither.  Frames: tests/dense_fused_cases.py's texture, halfflat, move0, move1, movehalf, halfflat at 480 x 270 with
LK = (1, 2, 1) and FB = (5, 6, 3), cap (24, 24) unless said; hip_klt on the six 128 x 96 frames of tests/klt_batch_cases.py at SMALL_SETS[1]:
  decode    ofps_hip_lk_decode on the five pairs: plain, masked, full-resolution records masked, reduced at cap (150, 150), reduced BGR,
            Farneback, sparse;
  plain     the stream of ofps_hip_lk_push_frame_async, two tickets in flight: LK masked, Farneback with use_previous, reduced BGR from a
            page-locked frame (the front-end gathers from host memory) and from a pageable one (staged);
  fused     the stream of ofps_hip_lk_push_frame_fused_async, two in flight: LK masked with least squares and with RANSAC, Farneback masked,
            reduced masked at cap (300, 300) -- 50,400 records, above the single-workgroup compaction's 32,768 --, sparse without and with
            klt_prediction;
  sync      ofps_hip_lk_push_frame_fused with a plain ofps_hip_lk_push_frame as every third call;
  geometry  480 x 270 and then 128 x 96 on one stream with nothing in flight.
Prints one line per case with the SHA-256 of everything the case returned; --out writes the lines to a file.
  rocprofv3 --kernel-trace [--memory-copy-trace] --output-format csv [json] -d <dir> -- python tools/dense_dispatch_driver.py [--lib <libofps_hip.so>] [--out <file>]
  python tools/dense_dispatch_driver.py --list <dir>      the listing of tools/sad_dispatch_driver.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from sad_dispatch_driver import listing

KINDS = ("texture", "halfflat", "move0", "move1", "movehalf", "halfflat")
CAP = (24, 24)


def main():
    if "--list" in sys.argv:
        return listing(sys.argv[sys.argv.index("--list") + 1])
    if "--lib" in sys.argv:
        from ofps_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import numpy as np

    import dense_fused_cases as fc
    import klt_batch_cases as bc
    from ofps_amd.runtime import HipContext

    ctx = HipContext(0)
    lines = []
    frames = [np.ascontiguousarray(fc.frame(k)) for k in KINDS]
    bgr = [np.ascontiguousarray(fc.bgr_of(f)) for f in frames]
    small = [np.ascontiguousarray(f) for f in bc.sequence(bc.SMALL)]
    klt_set = bc.SMALL_SETS[1]
    klt = dict(levels=klt_set[5], radius=klt_set[6], iters=klt_set[7], sparse=True)
    tail = dict(detector=True, estimator=True, aspect=fc.CAM[0], fov_y_deg=fc.CAM[1], num_iters=fc.RANSAC_ITERS, inlier_deg=fc.INLIER_DEG,
                num_samples=300, **fc.DETECTOR)

    def done(case, parts):
        h = hashlib.sha256()
        for p in parts:
            h.update(np.ascontiguousarray(p).tobytes())
        lines.append(f"{case:44s} {h.hexdigest()}")

    def kw(params=fc.LK, cap=CAP, **flags):
        return dict(levels=params[0], radius=params[1], iters=params[2], max_w=cap[0], max_h=cap[1], **flags)

    def plain_bytes(got):
        return [np.zeros(1, np.int64)] if got is None else [np.array([1, len(got[0]), *got[1]], np.int64), got[0]]

    def fused_bytes(r):
        area, field = (-1, np.zeros(0)) if r["motion"] is None else r["motion"]
        return [np.array([r["have_vectors"], r["n_vectors"], area, *r["grid"]], np.int64), r["quat"], field,
                r["entries"] if r["have_vectors"] else np.zeros(0)]

    # ---- ofps_hip_lk_decode
    ctx.set_klt(*klt_set[:5])
    for case, seq, k in (("plain", frames, kw()), ("masked", frames, kw(contrast_mask=True)),
                         ("fullres records masked", frames, kw(contrast_mask=True, fullres_records=True)),
                         ("reduced cap 150", frames, kw(cap=(150, 150), contrast_mask=True, reduced=True)),
                         ("reduced bgr", bgr, kw(contrast_mask=True, reduced=True, fmt=ctx.FMT_BGR)),
                         ("farneback", frames, kw(fc.FB, contrast_mask=True, farneback=True)), ("sparse", small, klt)):
        parts = []
        for prev, cur in zip(seq, seq[1:]):
            parts += plain_bytes(ctx.lk_decode(prev, cur, **k))
        done(f"decode {case}", parts)

    # ---- the streams, two tickets in flight
    def stream(seq, push, wait, to_bytes, page_locked=False):
        ctx.lk_reset()
        pins = [ctx.pinned_array(seq[0].shape, np.uint8) for _ in range(3)] if page_locked else None
        parts, pending = [], []
        for j, f in enumerate(seq):
            if len(pending) == 2:
                parts += to_bytes(wait(pending.pop(0)))
            if pins:
                np.copyto(pins[j % 3], f)
                f = pins[j % 3]
            pending.append(push(f, j))
        while pending:
            parts += to_bytes(wait(pending.pop(0)))
        for p in pins or ():
            ctx.free_pinned(p)
        ctx.lk_reset()
        return parts

    def plain_stream(seq, k, page_locked=False):
        return stream(seq, lambda f, j: ctx.lk_push_frame_async(f, **k), ctx.lk_frame_wait, plain_bytes, page_locked)

    def fused_stream(seq, k, **t):
        return stream(seq, lambda f, j: ctx.lk_push_frame_fused_async(f, seed=fc.SEED + j, **k, **dict(tail, **t)), ctx.lk_frame_fused_wait, fused_bytes)

    done("plain lk masked", plain_stream(frames, kw(contrast_mask=True)))
    done("plain farneback use_previous", plain_stream(frames, kw(fc.FB, contrast_mask=True, farneback=True, use_previous=True)))
    done("plain reduced bgr page-locked", plain_stream(bgr, kw(contrast_mask=True, reduced=True, fmt=ctx.FMT_BGR), page_locked=True))
    done("plain reduced bgr pageable", plain_stream(bgr, kw(contrast_mask=True, reduced=True, fmt=ctx.FMT_BGR)))
    done("fused lk masked least squares", fused_stream(frames, kw(contrast_mask=True)))
    done("fused lk masked ransac", fused_stream(frames, kw(contrast_mask=True), use_ransac=True))
    done("fused farneback masked", fused_stream(frames, kw(fc.FB, contrast_mask=True, farneback=True)))
    done("fused reduced masked cap 300", fused_stream(frames, kw(cap=(300, 300), contrast_mask=True, reduced=True)))
    klt_tail = dict(min_size=0.05, subdivide=2)
    done("fused sparse", fused_stream(small, klt, **klt_tail))
    ctx.set_klt_prediction(1)
    done("fused sparse prediction", fused_stream(small, klt, **klt_tail))
    ctx.set_klt_prediction(0)
    ctx.set_klt()

    # ---- the synchronous form with a plain push in the middle
    ctx.lk_reset()
    parts = []
    for j, f in enumerate(frames):
        if j % 3 == 2:
            parts += plain_bytes(ctx.lk_push_frame(f, **kw(contrast_mask=True)))
        else:
            parts += fused_bytes(ctx.lk_push_frame_fused(f, seed=fc.SEED + j, **kw(contrast_mask=True), **tail))
    done("sync fused with plain pushes", parts)

    # ---- a geometry change with nothing in flight: the stream restarts
    ctx.lk_reset()
    parts = []
    for j, f in enumerate(frames[:3] + small[:3]):
        parts += fused_bytes(ctx.lk_push_frame_fused(f, seed=fc.SEED + j, **kw(contrast_mask=True), **tail))
    done("geometry 480x270 -> 128x96", parts)
    ctx.lk_reset()
    ctx.close()
    print("\n".join(lines))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
