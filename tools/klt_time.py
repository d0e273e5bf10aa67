#!/usr/bin/env python3
"""Times hip_klt (csrc/klt.hip, include/ofps_hip.h N3) on the device, with the plain hip_sad search and the dense hip_lk flow beside it in
the same process.  Needs the GPU; prints one JSON line.

Per geometry (1080p with cell 16, 4K with cell 8; levels 4, window radius 7, 10 iterations) and content (synth.luma_sequence: region-wise
integer jumps; synth.camera_warp_pair: a smooth sub-pixel camera motion), on frames resident in device memory:
  score    ofps_hip_klt_features_dev: one pass over the previous frame
  pyramid  the 2 * (levels - 1) ofps_hip_sad_down2_dev launches both frames' levels cost
  track    ofps_hip_klt_track_dev on the frame's own features: the pyramid and the track launch (track_alone = track - pyramid, derived)
  flow     ofps_hip_klt_flow_dev: score + pyramid + track + status flags + ordered compaction + count, everything a decoder call enqueues
  sad      ofps_hip_sad_flow_dev, 16 x 16 blocks, +-16, one pair: the plain search
  lk       ofps_hip_lk_flow_dev with the bench's parameters (3 levels, radius 4, 3 steps), records out
Protocol: time per call of a saturated queue -- `--calls` (50) calls between two HIP events on the context's stream --, the median of
`--reps` (7) such windows behind `--warm` (2) windows that are not counted.  Beside the times: the slot count, the kept count and the
status histogram of the flow (0 kept, 1 no feature, 2 flat, 3 left the frame, 4 residual).

--batch N: the batch form (N3b) in place of the table above.  Per geometry and content a chain of N + 1 frames resident in device memory
(luma_sequence: N + 1 frames of the sequence; camera_warp_pair: the pair's two frames in turn, so the pairs are the warp and its inverse), and
  batch       one ofps_hip_klt_flow_batch_dev call over the N pairs
  one_by_one  N ofps_hip_klt_flow_dev calls over the same pairs
both in microseconds per PAIR, a window holding about `--calls` pairs.  The batch form's split into score, pyramid, track and compaction is not
taken here: it is the kernel times of a `rocprofv3 --kernel-trace --stats` run of this mode (klt_score_batch_kernel, sad_down2_kernel,
klt_track_batch_kernel, compact_items_kernel), in a run of its own.

--mean-removal: the same table, or the same batch mode, with ofps_hip_set_klt_mean_removal(1) (N3m): every hip_klt row then runs
klt_track_zm_kernel / klt_track_batch_zm_kernel; the rows say so ("mean_removal": 1).  --klt-only leaves the hip_sad and hip_lk rows out.
--fb N: with ofps_hip_set_klt_fb(N) (N3f): every hip_klt row then runs the FB kernels, the backward pass inside the track launch for the slots
the forward pass kept; the rows say so ("fb_limit": N) and their "kept" and status histogram (5 = did not return) are the checked ones.
--predict: the one-pair rows also time the predictor alone ("predict") and ofps_hip_klt_flow_from_dev started from the pair's own slots
("flow_from", N3p: a steady pair, every track starts from its answer and runs the klt_track_pred kernels); the rows say so ("predict": 1).
--batch-predict (with --batch N): two more columns, the chained batch (N3pb) and what it replaces, both per pair:
  chained          one ofps_hip_klt_flow_batch_from_dev call over the N pairs, from zero: one score launch, one halving per level, N track launches
                   (klt_track_batch_pred kernels), one compaction
  one_by_one_from  N ofps_hip_klt_flow_from_dev calls over the same pairs, each given the slots of the one before
and "chained_equals_one_by_one_from" says whether the two agree in counts and records.
--intra Q [--cut P]: with ofps_hip_set_klt_intra(Q) and ofps_hip_set_klt_cut(P) (N3i): every row that runs the decoder ("flow", "flow_from", the
batch columns) then enqueues klt_activity_kernel<true> and, with P > 0, klt_cut_kernel between the track launch and the compaction; the stage
rows (score, pyramid, track) do not change.  The rows say so ("intra", "cut"), their "kept" and status histogram (6 = intra, 7 = cut) are the
filtered ones, and a one-pair row also times the activity stage alone ("activity": ofps_hip_klt_activity_dev on the frame's features)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ofps_amd import synth  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402


def window_ms(ctx, fn, calls, reps, warm):
    out = []
    for k in range(warm + reps):
        ctx.timer_start()
        for _ in range(calls):
            fn()
        ms = ctx.timer_stop() / calls
        if k >= warm:
            out.append(ms)
    return {"median_us": round(float(np.median(out)) * 1e3, 2), "min_us": round(min(out) * 1e3, 2), "max_us": round(max(out) * 1e3, 2)}


def one(ctx, name, prev, cur, cell, levels, radius, iters, max_residual, calls, reps, warm, klt_only=False, predict=False):
    H, W = prev.shape
    ctx.set_klt(cell, 2, 1, 1, max_residual)
    ns = ctx.klt_slot_count(W, H)
    d_fr = ctx.malloc(2 * W * H)
    ctx.memcpy_h2d(d_fr, np.stack([prev, cur]))
    d_prev, d_cur = d_fr, d_fr + W * H
    d_tri, d_quad, d_rec, d_cnt, d_slots = ctx.malloc(12 * ns), ctx.malloc(16 * ns), ctx.malloc(16 * ns), ctx.malloc(16), ctx.malloc(24 * ns)
    ctx.klt_features_dev(d_prev, W, H, W, d_tri)
    ctx.sync()
    tri = np.zeros((ns, 3), np.int32)
    ctx.memcpy_d2h(tri, d_tri)
    pts = np.ascontiguousarray(tri[tri[:, 0] >= 0][:, :2])
    d_pts = ctx.malloc(max(pts.nbytes, 16))
    ctx.memcpy_h2d(d_pts, pts)
    pyr = []                                                  # the levels' own buffers for the pyramid-alone timing
    w, h = W, H
    for _ in range(1, levels):
        w, h = w >> 1, h >> 1
        s = (w + 63) & ~63
        pyr.append((w, h, s, ctx.malloc(s * h), ctx.malloc(s * h)))

    def pyramid():
        sp, sc, sw, sh, ss = d_prev, d_cur, W, H, W
        for (lw, lh, ls, dp, dc) in pyr:
            ctx.sad_down2_dev(sp, sw, sh, ss, dp, ls)
            ctx.sad_down2_dev(sc, sw, sh, ss, dc, ls)
            sp, sc, sw, sh, ss = dp, dc, lw, lh, ls

    nblk = (W // 16) * (H // 16)
    d_sad = ctx.malloc(16 * nblk)
    d_lk = ctx.malloc(16 * W * H)
    t = {
        "score": window_ms(ctx, lambda: ctx.klt_features_dev(d_prev, W, H, W, d_tri), calls, reps, warm),
        "pyramid": window_ms(ctx, pyramid, calls, reps, warm),
        "track": window_ms(ctx, lambda: ctx.klt_track_dev(d_prev, d_cur, W, H, W, d_pts, len(pts), levels, radius, iters, d_quad), calls, reps, warm),
        "flow": window_ms(ctx, lambda: ctx.klt_flow_dev(d_prev, d_cur, W, H, W, levels, radius, iters, d_rec, d_cnt, d_slots), calls, reps, warm),
    }
    if not klt_only:
        t["sad_16x16_pm16"] = window_ms(ctx, lambda: ctx.sad_flow_dev(d_fr, 2, W, H, W, W * H, 0, 16, 16, d_sad, None), calls, reps, warm)
        t["lk_3_4_3"] = window_ms(ctx, lambda: ctx.lk_flow_dev(d_prev, d_cur, W, H, W, 3, 4, 3, None, d_lk), calls, reps, warm)
    if ctx.get_klt_intra() > 0:
        d_act = ctx.malloc(max(4 * len(pts), 16))
        t["activity"] = window_ms(ctx, lambda: ctx.klt_activity_dev(d_prev, W, H, W, d_pts, len(pts), radius, d_act), calls, reps, warm)
        ctx.free(d_act)
    t["track_alone_derived_us"] = round(t["track"]["median_us"] - t["pyramid"]["median_us"], 2)
    ctx.klt_flow_dev(d_prev, d_cur, W, H, W, levels, radius, iters, d_rec, d_cnt, d_slots)
    ctx.sync()
    if predict:         # N3p on a steady pair: the pair's own slots as the previous pair's, so every track starts from its answer
        d_slots0, d_guess = ctx.malloc(24 * ns), ctx.malloc(8 * ns)
        keep = np.zeros((ns, 6), np.int32)
        ctx.memcpy_d2h(keep, d_slots)
        ctx.memcpy_h2d(d_slots0, keep)
        t["predict"] = window_ms(ctx, lambda: ctx.klt_predict_dev(d_slots0, W, H, cell, d_guess), calls, reps, warm)
        t["flow_from"] = window_ms(ctx, lambda: ctx.klt_flow_from_dev(d_prev, d_cur, W, H, W, levels, radius, iters, d_slots0, d_rec, d_cnt, d_slots), calls, reps, warm)
        ctx.klt_flow_from_dev(d_prev, d_cur, W, H, W, levels, radius, iters, d_slots0, d_rec, d_cnt, d_slots)
        ctx.sync()
        ctx.free(d_slots0); ctx.free(d_guess)
    slots = np.zeros((ns, 6), np.int32)
    cnt = np.zeros(4, np.uint32)
    ctx.memcpy_d2h(slots, d_slots)
    ctx.memcpy_d2h(cnt, d_cnt)
    u, c = np.unique(slots[:, 5], return_counts=True)
    for p in [d_fr, d_tri, d_quad, d_rec, d_cnt, d_slots, d_pts, d_sad, d_lk] + [b for lv in pyr for b in lv[3:]]:
        ctx.free(p)
    return {"case": name, "geometry": f"{W}x{H}", "cell": cell, "levels": levels, "radius": radius, "iters": iters, "max_residual": max_residual,
            "mean_removal": ctx.get_klt_mean_removal(), "fb_limit": ctx.get_klt_fb(), "intra": ctx.get_klt_intra(), "cut": ctx.get_klt_cut(), "predict": int(predict), "slots": int(ns), "features": int(len(pts)), "kept": int(cnt[0]), "status_histogram": {int(a): int(b) for a, b in zip(u, c)}, "times": t}


def one_batch(ctx, name, frames, cell, levels, radius, iters, max_residual, calls, reps, warm, batch_predict=False):
    n_frames, H, W = frames.shape
    N = n_frames - 1
    ctx.set_klt(cell, 2, 1, 1, max_residual)
    ns = ctx.klt_slot_count(W, H)
    d_fr = ctx.malloc(n_frames * W * H)
    ctx.memcpy_h2d(d_fr, frames)
    d_rec, d_cnt = ctx.malloc(16 * ns * N), ctx.malloc(max(4 * N, 16))
    d_rec1, d_cnt1 = ctx.malloc(16 * ns * N), ctx.malloc(max(4 * N, 16))
    windows = max(1, (calls + N - 1) // N)

    def batch():
        ctx.klt_flow_batch_dev(d_fr, n_frames, W, H, W, W * H, 0, levels, radius, iters, d_rec, d_cnt)

    def one_by_one():
        for k in range(N):
            ctx.klt_flow_dev(d_fr + k * W * H, d_fr + (k + 1) * W * H, W, H, W, levels, radius, iters, d_rec1 + 16 * ns * k, d_cnt1 + 4 * k)

    t = {"batch": window_ms(ctx, batch, windows, reps, warm), "one_by_one": window_ms(ctx, one_by_one, windows, reps, warm)}
    chained_same = None
    if batch_predict:                                         # N3pb: the chained batch against the chain of one-pair calls it equals
        d_rec2, d_cnt2, d_sl = ctx.malloc(16 * ns * N), ctx.malloc(max(4 * N, 16)), [ctx.malloc(24 * ns), ctx.malloc(24 * ns)]

        def chained():
            ctx.klt_flow_batch_from_dev(d_fr, n_frames, W, H, W, W * H, 0, levels, radius, iters, d_rec, d_cnt, None, None)

        def one_by_one_from():
            for k in range(N):
                ctx.klt_flow_from_dev(d_fr + k * W * H, d_fr + (k + 1) * W * H, W, H, W, levels, radius, iters, d_sl[(k + 1) & 1] if k else None,
                                      d_rec2 + 16 * ns * k, d_cnt2 + 4 * k, d_sl[k & 1])

        t["chained"] = window_ms(ctx, chained, windows, reps, warm)
        t["one_by_one_from"] = window_ms(ctx, one_by_one_from, windows, reps, warm)
        chained(); one_by_one_from(); ctx.sync()
        c0, c2 = np.zeros(max(N, 4), np.uint32), np.zeros(max(N, 4), np.uint32)
        ctx.memcpy_d2h(c0, d_cnt); ctx.memcpy_d2h(c2, d_cnt2)
        r0, r2 = np.zeros((N, ns, 4), np.float32), np.zeros((N, ns, 4), np.float32)
        ctx.memcpy_d2h(r0, d_rec); ctx.memcpy_d2h(r2, d_rec2)
        chained_same = bool((c0[:N] == c2[:N]).all() and all(r0[k, :c0[k]].tobytes() == r2[k, :c0[k]].tobytes() for k in range(N)))
        chained_kept = [int(c) for c in c0[:N]]
        for p in [d_rec2, d_cnt2] + d_sl:
            ctx.free(p)
    for v in t.values():                                      # per call of N pairs -> per pair
        for key in v:
            v[key] = round(v[key] / N, 2)
    batch(); one_by_one(); ctx.sync()
    cnt, cnt1 = np.zeros(max(N, 4), np.uint32), np.zeros(max(N, 4), np.uint32)
    ctx.memcpy_d2h(cnt, d_cnt); ctx.memcpy_d2h(cnt1, d_cnt1)
    rec, rec1 = np.zeros((N, ns, 4), np.float32), np.zeros((N, ns, 4), np.float32)
    ctx.memcpy_d2h(rec, d_rec); ctx.memcpy_d2h(rec1, d_rec1)
    same = bool((cnt[:N] == cnt1[:N]).all() and all(rec[k, :cnt[k]].tobytes() == rec1[k, :cnt[k]].tobytes() for k in range(N)))
    for p in (d_fr, d_rec, d_cnt, d_rec1, d_cnt1):
        ctx.free(p)
    row = {"case": name, "geometry": f"{W}x{H}", "cell": cell, "levels": levels, "radius": radius, "iters": iters, "max_residual": max_residual,
           "mean_removal": ctx.get_klt_mean_removal(), "fb_limit": ctx.get_klt_fb(), "intra": ctx.get_klt_intra(), "cut": ctx.get_klt_cut(), "batch": N, "slots": int(ns), "kept": [int(c) for c in cnt[:N]], "batch_equals_one_by_one": same, "calls_per_window": windows,
           "us_per_pair": t}
    if batch_predict:
        row.update({"chained_kept": chained_kept, "chained_equals_one_by_one_from": chained_same})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0, help="N > 0: time the batch form over N pairs against N one-pair calls")
    ap.add_argument("--no-1080p", action="store_true")
    ap.add_argument("--content", choices=["both", "luma_sequence", "camera_warp_pair"], default="both", help="--batch: one content alone (a kernel trace per content)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--radius", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-residual", type=int, default=0)
    ap.add_argument("--no-4k", action="store_true")
    ap.add_argument("--mean-removal", action="store_true", help="hip_klt with mean removal (include/ofps_hip.h N3m)")
    ap.add_argument("--fb", type=int, default=0, metavar="N", help="hip_klt with the forward-backward check at N / 256 pixel (include/ofps_hip.h N3f)")
    ap.add_argument("--klt-only", action="store_true", help="no hip_sad and hip_lk rows beside hip_klt's")
    ap.add_argument("--predict", action="store_true", help="one-pair rows: also the predictor alone and ofps_hip_klt_flow_from_dev started from the pair's own slots "
                                                           "(include/ofps_hip.h N3p); kept and the status histogram are then that call's")
    ap.add_argument("--batch-predict", action="store_true", help="--batch: also the chained batch (include/ofps_hip.h N3pb) and the chain of "
                                                                 "ofps_hip_klt_flow_from_dev calls it equals")
    ap.add_argument("--intra", type=int, default=0, metavar="Q", help="hip_klt with the intra test at Q sixteenths (include/ofps_hip.h N3i)")
    ap.add_argument("--cut", type=int, default=0, metavar="P", help="with --intra: the scene-cut rule at P percent")
    a = ap.parse_args()
    ctx = HipContext(0)
    ctx.set_klt_mean_removal(1 if a.mean_removal else 0)
    ctx.set_klt_fb(a.fb)
    ctx.set_klt_intra(a.intra)
    ctx.set_klt_cut(a.cut)
    rows = []
    for W, H, cell in ([] if a.no_1080p else [(1920, 1080, 16)]) + ([] if a.no_4k else [(3840, 2160, 8)]):
        lum = synth.luma_sequence(max(a.batch + 1, 2), W, H, max_step=6, seed=5)
        warp = synth.camera_warp_pair(W, H, shift=(3.3 * W / 1920, -2.6 * H / 1080))
        if a.batch > 0:
            chain = np.stack([warp[k & 1] for k in range(a.batch + 1)])
            for name, fr in (("luma_sequence", lum), ("camera_warp_pair", chain)):
                if a.content not in ("both", name):
                    continue
                rows.append(one_batch(ctx, name, np.ascontiguousarray(fr), cell, a.levels, a.radius, a.iters, a.max_residual, a.calls, a.reps, a.warm, a.batch_predict))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            continue
        for name, (p, c) in (("luma_sequence", (lum[0], lum[1])), ("camera_warp_pair", (warp[0], warp[1]))):
            rows.append(one(ctx, name, np.ascontiguousarray(p), np.ascontiguousarray(c), cell, a.levels, a.radius, a.iters, a.max_residual,
                            a.calls, a.reps, a.warm, a.klt_only, a.predict))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps({"calls_per_window": a.calls, "windows": a.reps, "warm_windows": a.warm, "rows": rows}))


if __name__ == "__main__":
    main()
