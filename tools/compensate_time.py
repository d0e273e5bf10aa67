#!/usr/bin/env python3
"""Times the compensation stage (csrc/compensate.hip) and the price of detect-compensation mode 1.  Needs the GPU; prints one JSON line.

  python tools/compensate_time.py --kernel
      ofps_hip_compensate_dev on 2,073,600 records (one per pixel of a 1080p frame: cfg3's record count), HIP-event timed on the context's
      stream, median of 7 -- and, in the same run with the same bytes, a hipMemcpyDtoDAsync of the records (33.2 MB).  The kernel reads
      33.2 MB and writes 33.2 MB; the copy does the same.
  python tools/compensate_time.py --latency --mode 0|1 [--ransac]
      cfg5-shaped: 1080p luma frames through ofps_hip_push_frame (block 16, range 16, detector + estimator), host wall time per frame
      (frame pushed -> island + quaternion on the host), p50 over --frames frames after a warm-up.  One process per (mode, estimator):
      run it from fresh processes, the modes interleaved, and take the median of the p50s.
      --lib PATH: another build of libofps_hip.so (e.g. the parent commit's, which has no compensation stage: mode 0 only) for an A/B on one device."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ofps_amd import _lib, synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

CAM = (16 / 9, 39.6 * 9 / 16)


def kernel(reps=7):
    ctx = HipContext(0)
    hip = C.CDLL("libamdhip64.so.7")         # the SONAME: the runtime the library already runs on, not a second copy
    hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    n = 1920 * 1080
    rng = np.random.default_rng(0)
    e = np.empty((n, 4), np.float32)
    e[:, :2] = rng.random((n, 2), np.float32)
    e[:, 2:] = (rng.random((n, 2), np.float32) - 0.5) * 0.02
    q = np.array([0.99998, 0.002, -0.001, 0.004], np.float32)
    nbytes = e.nbytes
    d_in, d_out, d_q = ctx.malloc(nbytes), ctx.malloc(nbytes), ctx.malloc(16)
    ctx.memcpy_h2d(d_in, e)
    ctx.memcpy_h2d(d_q, q)
    stream = ctx.get_stream()

    def timed(fn):
        for _ in range(3):
            fn()
        ctx.sync()
        ms = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            ms.append(ctx.timer_stop())
        return ms

    k_ms = timed(lambda: ctx.compensate_dev(d_in, n, 1, *CAM, d_q, d_out))
    c_ms = timed(lambda: hip.hipMemcpyDtoDAsync(C.c_void_p(d_out), C.c_void_p(d_in), nbytes, C.c_void_p(stream)))
    for p in (d_in, d_out, d_q):
        ctx.free(p)
    ctx.close()
    med = lambda v: float(np.median(v))
    return {"records": n, "bytes_read": nbytes, "bytes_written": nbytes,
            "compensate_ms": {"median": med(k_ms), "min": min(k_ms), "max": max(k_ms)},
            "compensate_GBps": 2 * nbytes / med(k_ms) / 1e6,
            "dtod_copy_ms": {"median": med(c_ms), "min": min(c_ms), "max": max(c_ms)},
            "dtod_copy_GBps": 2 * nbytes / med(c_ms) / 1e6,
            "kernel_over_copy_rate": med(c_ms) / med(k_ms)}


def use_library(path):
    """bind another build; one from before the compensation stage lacks its four entry points"""
    _lib.LIB_PATH = os.path.abspath(path)
    try:
        import torch  # noqa: F401  (first, as _lib.load does: one HIP runtime in the process)
    except Exception:
        pass
    exported = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(exported, n)]:
        del _lib.PROTOTYPES[name]


def latency(mode, use_ransac, frames, warm):
    ctx = HipContext(0)
    if mode or "ofps_hip_set_detect_compensation" in _lib.PROTOTYPES:
        ctx.set_detect_compensation(mode)
    f = synth.luma_sequence(8, 1920, 1080, max_step=6, seed=5)
    pin = ctx.pinned_frame(1080, 1920)
    ms = []
    for k in range(warm + frames):
        np.copyto(pin, f[k % 8])
        t0 = time.perf_counter()
        ctx.push_frame(pin, 16, 16, aspect=CAM[0], fov_y_deg=CAM[1], use_ransac=use_ransac, seed=k)
        if k >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    return {"mode": mode, "estimator": "ransac" if use_ransac else "lsq", "frames": frames, "p50_ms": float(np.percentile(ms, 50)),
            "p95_ms": float(np.percentile(ms, 95)), "min_ms": float(min(ms))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--latency", action="store_true")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--ransac", action="store_true")
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        use_library(a.lib)
    out = kernel() if a.kernel else latency(a.mode, a.ransac, a.frames, a.warmup)
    if a.lib:
        out["lib"] = a.lib
    print(json.dumps(out))
