#!/usr/bin/env python3
"""End-to-end accuracy in the reference's own unit: mean / max rotation error per frame, in degrees, of the
image -> vectors -> rotation path against PLANTED camera rotations -- what docs/statistics/err_av.csv tabulates for the reference's
estimators against Blender ground truth (loader ofps-suite/src/app/tracking/mod.rs:125-217, export :825-847, summary
scripts/extract_stats.py: degs(error.mean())).

Clips are rendered by ofps_amd.synth.rotation_clip from per-frame rotations through the pinhole model of StandardCamera (pan / tilt /
roll / mixed, 0.01 - 1 degree per frame, one clip with an independently moving foreground object = the reference's "dyn" clips).
Every clip runs through the tracking loop of ofps-suite/src/app/tracking/worker.rs:305-412 written with the plugin mirrors
(ofps_amd/plugins.py): decoder.process_frame -> estimator.motion_step (pose accumulation, ofps/src/estimator.rs:38-53), for
  decoders    hip_sad (16x16 blocks, +-16)  |  hip_lk (3-level pyramid, r = 4, 3 steps, contrast mask, 150 x 84 records)  |  hip_lk5 (the same
              with "Pyramid levels" = 5, the reference's Farneback depth)  |  hip_flow (Farneback's polynomial-expansion flow with
              cv-decoder's own arguments: levels 5, winsize 13, 3 iterations, poly_n 7, poly_sigma 1.5; same mask and records)
              with --quarter-pel also hip_sad_q: hip_sad with its "Quarter pel" property on (motion scale 4, include/ofps_hip.h N1q)
              with --sad-consistency N also hip_sad_c: hip_sad with its "Consistency check" property at N (include/ofps_hip.h N1c)
              with --sad-levels N also hip_sad_h: hip_sad with its "Search levels" property at N (include/ofps_hip.h N1h; reach 2 * 16 + 3 =
              35 px at N = 2, 73 px at N = 3); --fast-clips adds 1080p pans of 1.5 and 3 degrees per frame (24 and 49 px at the centre:
              beyond the plain search's +-16); --sad-only leaves the dense decoders' columns out
              with --sad-levels N --sad-predictors 1 also hip_sad_hp: the same with "Neighbour predictors" on (include/ofps_hip.h N1p)
              with --sad-prefilter R [R ...] also hip_sad_m<R>: hip_sad with its "Mean removal" property at R (include/ofps_hip.h N1m)
              with --sad-median N [N ...] also hip_sad_v<N>: hip_sad with its "Median test" property at N (include/ofps_hip.h N1v); with
              --sad-consistency C also hip_sad_cv<N>: on top of "Consistency check" = C
              with --sad-intra Q [Q ...] also hip_sad_i<Q>: hip_sad with its "Intra test" property at Q (include/ofps_hip.h N1i); --sad-cut P sets
              "Scene cut" = P in those columns; with --sad-prefilter R also hip_sad_fi<Q>: on top of "Mean removal" = R (the first R)
              with --sad-split T [T ...] also hip_sad_b<T>: hip_sad with its "Split blocks" property at T (include/ofps_hip.h N1s); with
              --sad-median N also hip_sad_xb<T>: on top of "Median test" = N (the first N)
              with --klt also hip_klt: the sparse decoder (include/ofps_hip.h N3) with its defaults -- cell 16, levels 4, window radius 7, 10
              iterations, no residual limit; --klt-cell C [C ...] and --klt-residual R [R ...] add hip_klt_c<C>r<R> for every other pair of
              "Cell size" and "Max residual"; --klt-mean-removal adds the same columns once more with "Mean removal" on (include/ofps_hip.h
              N3m) as hip_klt_m and hip_klt_c<C>r<R>_m; --klt-fb N [N ...] adds every hip_klt column once more per N with "Consistency check" = N
              (include/ofps_hip.h N3f, the round-trip limit in 1/256 pixel) as hip_klt_f<N>, and with --klt-mean-removal as hip_klt_f<N>_m; --klt-intra Q [Q ...] adds every hip_klt column once more per Q with "Intra test" = Q (include/ofps_hip.h N3i) as <column>_i<Q>, "Scene cut" at --klt-cut P in those columns; --klt-predict adds every hip_klt column once more with "Prediction" on (N3p) as <column>_p, --klt-levels L runs them all at L pyramid levels; --ramp-clips adds pans whose rate grows linearly from 0 to 1.5 and to 3 degrees per frame and swings back; --skip NAME [NAME ...] leaves decoder columns out (e.g. hip_lk5 hip_flow: most of the run time)
  cut clip    --cut-clip adds pan_0.2_cut: pan_0.2's rotations with the second half of the frames rendered from another canvas seed: one scene
              cut, the planted rotation across it unchanged.  Its rows also report the error at the cut pair
  lighting    --lighting L [L ...] runs every clip once per L, rendered once (rows "clip@L"; none = the clip as rendered): step = the exposure
              toggles by 20 grey levels every 4 frames (a quarter of the pairs straddle a step); flicker = +12 on odd frames, -12 on even
              ones (every pair differs by 24); ramp = odd frames gain 30 x/(W-1) - 10 y/(H-1) - 8 (a gradient that comes and goes); all
              rounded to nearest and clamped to 0..255
  estimators  hip_almeida LSQ  |  hip_almeida RANSAC (the reference's default: 200 hypotheses x 1000 samples, 0.05 degree inliers)
Per clip and combination: mean and max of angle_to(planted q_k, estimated r_k) over the frames, that mean relative to the clip's mean
rotation per frame (the reference's own test bound is 10 %: almeida-estimator/src/lib.rs:347-348), and the pose drift after the
last frame.  Beside it the CPU oracle chain on the same frames (all frames for hip_sad + LSQ; the first `--oracle-lk-pairs` pairs
for hip_lk + LSQ) and the largest |dq| between the two chains -- the oracle is the checker here, never the thing measured.

  python tools/accuracy_clips.py [--quick] [--out profiles/r05/accuracy.txt] [--json gpurun_out/r05/accuracy.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ofps_amd import synth  # noqa: E402


def triangle(rate, n, period):
    """+rate for period frames, -rate for 2 x period, +rate ... : constant speed, bounded accumulated angle."""
    k = np.arange(n)
    return np.where(((k + period) // (2 * period)) % 2 == 0, rate, -rate).astype(np.float64)


def clip_table(quick=False, fast_clips=False, ramp_clips=False):
    """name -> (W, H, fov_y_deg, per-frame eulers [n, 3] (roll = tilt, pitch = image roll, yaw = pan), distractor)"""
    n = 24 if quick else 60
    W, H = 1920, 1080
    z = np.zeros(n)
    k = np.arange(n)
    t = {}
    t["pan_0.2"] = (W, H, 60.0, np.stack([z, z, triangle(0.2, n, 20)], 1), None)
    t["tilt_0.2"] = (W, H, 60.0, np.stack([triangle(0.2, n, 20), z, z], 1), None)
    t["roll_0.3"] = (W, H, 60.0, np.stack([z, triangle(0.3, n, 20), z], 1), None)
    t["slow_pan_0.01"] = (W, H, 60.0, np.stack([z, z, z + 0.01], 1), None)
    t["pan_tilt_0.05"] = (W, H, 60.0, np.stack([z + 0.05, z, z - 0.05], 1), None)
    t["fast_pan_0.5"] = (W, H, 60.0, np.stack([z, z, triangle(0.5, n, 12)], 1), None)
    mixed = np.stack([0.25 * np.sin(2 * np.pi * k / 30.0), 0.3 * np.sin(2 * np.pi * k / 24.0 + 1.0), 0.3 * np.cos(2 * np.pi * k / 40.0)], 1)
    t["mixed_sine"] = (W, H, 60.0, mixed, None)
    t["mixed_sine_dyn"] = (W, H, 60.0, mixed, dict(size=(W // 5, H // 4), start=(W // 10, H // 3), velocity=(W / 1920 * 7.0, -H / 1080 * 2.0)))
    if not quick:
        t["1deg_mixed_360p"] = (640, 360, 60.0, np.stack([triangle(0.6, n, 8), triangle(0.3, n, 10), triangle(0.7, n, 6)], 1), None)
    if fast_clips:      # beyond the plain search's reach at 1080p (16.32 px per degree at the centre); the accumulated pan stays within +-9 degrees
        t["fast_pan_1.5"] = (W, H, 60.0, np.stack([z, z, triangle(1.5, n, 4)], 1), None)
        t["fast_pan_3.0"] = (W, H, 60.0, np.stack([z, z, triangle(3.0, n, 3)], 1), None)
    if ramp_clips:      # pans whose rate grows linearly from 0 to the fast clips' rates over m frames, falls back through 0 to the same rate the
        def ramp(rate, m):      # other way, and so on: smooth motion that starts at rest; the accumulated pan stays within 0 .. rate * m = 9 degrees
            ph = (k % (4 * m)) / float(m)
            return rate * np.where(ph <= 1, ph, np.where(ph <= 3, 2 - ph, ph - 4))
        t["ramp_pan_1.5"] = (W, H, 60.0, np.stack([z, z, ramp(1.5, 6)], 1), None)      # the rate changes by 0.25 degrees (4 px) per pair
        t["ramp_pan_3.0"] = (W, H, 60.0, np.stack([z, z, ramp(3.0, 3)], 1), None)      # ... by 1 degree (16 px) per pair
    return t


def track(frames, cam, decoder_cls, use_ransac, device=0, **dec_props):
    """The tracking worker's loop (worker.rs:305-412): -> (per-pair quaternions [n, 4], accumulated rotation, seconds per frame)."""
    from ofps_amd.plugins import HipAlmeidaEstimator
    dec = decoder_cls(iter(frames), device=device)
    for name, v in dec_props.items():
        assert dec.set_prop(name, v), name
    est = HipAlmeidaEstimator(device)
    est.set_prop("Use ransac", use_ransac)
    rot, pos = np.array([1.0, 0, 0, 0], np.float32), np.zeros(3, np.float32)
    out = []
    t0 = time.perf_counter()
    while True:
        field = []
        try:
            have = dec.process_frame(field)
        except EOFError:
            break
        if not have:
            continue
        new_rot, pos = est.motion_step(field, cam, None, rot, pos)     # estimator.rs:38-53: rot = r * rot, pos += rot * tr (tr = 0)
        r = _qmul64(new_rot, [rot[0], -rot[1], -rot[2], -rot[3]])      # r = new_rot * rot^-1, the estimate of this pair ...
        out.append(r / np.linalg.norm(r))                              # ... up to |rot|^2: f32 products of f32 unit quaternions drift in norm (~3e-7 per frame), as nalgebra's do
        rot = new_rot
    dt = (time.perf_counter() - t0) / max(1, len(out))
    dec.ctx.close(); est.ctx.close()
    return np.array(out), rot, dt


def _qmul(a, b):
    from ofps_amd.plugins import quat_mul
    return quat_mul(a, b)


def _qmul64(a, b):
    aw, ai, aj, ak = [float(v) for v in a]
    bw, bi, bj, bk = [float(v) for v in b]
    return np.array([aw * bw - ai * bi - aj * bj - ak * bk, aw * bi + ai * bw + aj * bk - ak * bj,
                     aw * bj - ai * bk + aj * bw + ak * bi, aw * bk + ai * bj - aj * bi + ak * bw])


def accumulate(quats):
    rot = np.array([1.0, 0, 0, 0], np.float32)
    for q in quats:
        rot = _qmul(np.asarray(q, np.float32), rot)
    return rot


def stats(est, truth):
    err = np.array([synth.quat_angle_deg(e, t) for e, t in zip(est, truth)])
    rate = np.array([synth.quat_angle_deg(t, [1, 0, 0, 0]) for t in truth])
    return {"mean_err_deg": float(err.mean()), "max_err_deg": float(err.max()), "mean_rot_deg": float(rate.mean()),
            "rel_mean": float(err.mean() / rate.mean()) if rate.mean() > 0 else None,
            "drift_deg": synth.quat_angle_deg(accumulate(est), accumulate(truth))}


def flat_third(frames, seed=5):
    """the clip with its right third replaced by constant 128 plus {0, 1} noise, fresh per frame: texture-free blocks under sensor noise"""
    out = np.array(frames, np.uint8)
    x0 = out.shape[2] * 2 // 3
    rng = np.random.default_rng(seed)
    out[:, :, x0:] = (128 + rng.integers(0, 2, out[:, :, x0:].shape)).astype(np.uint8)
    return out


def relight_clip(frames, lighting):
    """the clip under --lighting's change of brightness -> uint8 [n, H, W]"""
    if lighting == "none":
        return frames
    f = np.asarray(frames, np.uint8).astype(np.float32)
    n, H, W = f.shape
    k = np.arange(n)
    if lighting == "step":
        f += (20.0 * ((k // 4) % 2)).astype(np.float32)[:, None, None]
    elif lighting == "flicker":
        f += np.where(k % 2 == 1, 12.0, -12.0).astype(np.float32)[:, None, None]
    elif lighting == "ramp":
        ramp = 30.0 * np.arange(W, dtype=np.float32)[None, :] / (W - 1) - 10.0 * np.arange(H, dtype=np.float32)[:, None] / (H - 1) - 8.0
        f[1::2] += ramp[None]
    else:
        raise ValueError(lighting)
    return np.clip(np.floor(f + 0.5), 0, 255).astype(np.uint8)


CUT_CLIP, CUT_SEEDS = "pan_0.2_cut", (61, 62)


def run(quick=False, oracle_lk_pairs=3, with_oracle=True, only=None, log=print, quarter_pel=False, sad_gate=0, sad_consistency=0, sad_levels=0,
        fast_clips=False, sad_only=False, sad_predictors=0, lighting=("none",), sad_prefilter=(), sad_median=(), sad_intra=(), sad_cut=0,
        cut_clip=False, sad_split=(), klt=False, klt_cells=(16,), klt_residuals=(0,), skip=(),
        klt_mean_removal=False, klt_fb=(), klt_predict=False, ramp_clips=False, klt_levels=0, klt_intra=(), klt_cut=0):
    from ofps_amd.plugins import HipFlowDecoder, HipKltDecoder, HipLkDecoder, HipSadDecoder, StandardCamera
    combos = [("hip_sad", HipSadDecoder, False, {}), ("hip_sad", HipSadDecoder, True, {}), ("hip_lk", HipLkDecoder, False, {}),
              ("hip_lk", HipLkDecoder, True, {}),
              # the reference's dense decoder runs Farneback over FIVE pyramid levels (cv-decoder/src/lib.rs:188-199): the same decoder with
              # its "Pyramid levels" property at 5 (capture range x4)
              ("hip_lk5", HipLkDecoder, False, {"Pyramid levels": 5}), ("hip_lk5", HipLkDecoder, True, {"Pyramid levels": 5}),
              # Farneback's flow itself with cv-decoder's arguments (the hip_flow decoder)
              ("hip_flow", HipFlowDecoder, False, {}), ("hip_flow", HipFlowDecoder, True, {})]
    if quarter_pel:     # hip_sad with its "Quarter pel" property on (motion_scale 4: include/ofps_hip.h N1q); off by default: the -m gpu test's run time
        combos[2:2] = [("hip_sad_q", HipSadDecoder, False, {"Quarter pel": True}), ("hip_sad_q", HipSadDecoder, True, {"Quarter pel": True})]
    if sad_gate:        # hip_sad with its "Contrast gate" property at N (include/ofps_hip.h N1g), and every clip once more with a flat noisy third
        combos[2:2] = [("hip_sad_g", HipSadDecoder, False, {"Contrast gate": sad_gate}), ("hip_sad_g", HipSadDecoder, True, {"Contrast gate": sad_gate})]
    if sad_consistency:  # hip_sad with its "Consistency check" property at N (include/ofps_hip.h N1c); with --quarter-pel also on top of "Quarter pel"
        props_c = {"Consistency check": sad_consistency}
        combos[2:2] = [("hip_sad_c", HipSadDecoder, False, props_c), ("hip_sad_c", HipSadDecoder, True, props_c)]
        if quarter_pel:
            props_qc = {"Quarter pel": True, "Consistency check": sad_consistency}
            combos[2:2] = [("hip_sad_qc", HipSadDecoder, False, props_qc), ("hip_sad_qc", HipSadDecoder, True, props_qc)]
    if sad_levels:      # hip_sad with its "Search levels" property at N (include/ofps_hip.h N1h); with --quarter-pel also on top of "Quarter pel"
        props_h = {"Search levels": sad_levels}
        combos[2:2] = [("hip_sad_h", HipSadDecoder, False, props_h), ("hip_sad_h", HipSadDecoder, True, props_h)]
        if quarter_pel:
            props_qh = {"Quarter pel": True, "Search levels": sad_levels}
            combos[2:2] = [("hip_sad_qh", HipSadDecoder, False, props_qh), ("hip_sad_qh", HipSadDecoder, True, props_qh)]
        if sad_predictors:      # ... and beside them the same columns with "Neighbour predictors" on (include/ofps_hip.h N1p)
            props_hp = {"Search levels": sad_levels, "Neighbour predictors": True}
            combos[2:2] = [("hip_sad_hp", HipSadDecoder, False, props_hp), ("hip_sad_hp", HipSadDecoder, True, props_hp)]
            if sad_consistency:
                props_hpc = dict(props_hp, **{"Consistency check": sad_consistency})
                combos[2:2] = [("hip_sad_hpc", HipSadDecoder, False, props_hpc), ("hip_sad_hpc", HipSadDecoder, True, props_hpc)]
            if quarter_pel:
                props_qhp = dict(props_hp, **{"Quarter pel": True})
                combos[2:2] = [("hip_sad_qhp", HipSadDecoder, False, props_qhp), ("hip_sad_qhp", HipSadDecoder, True, props_qhp)]
    for radius in sad_prefilter:    # hip_sad with its "Mean removal" property at R (include/ofps_hip.h N1m); with --sad-levels N also on top of "Search levels"
        combos[2:2] = [(f"hip_sad_m{radius}", HipSadDecoder, False, {"Mean removal": radius}), (f"hip_sad_m{radius}", HipSadDecoder, True, {"Mean removal": radius})]
        if sad_levels:
            props_hm = {"Search levels": sad_levels, "Mean removal": radius}
            combos[2:2] = [(f"hip_sad_hm{radius}", HipSadDecoder, False, props_hm), (f"hip_sad_hm{radius}", HipSadDecoder, True, props_hm)]
    for limit in sad_median:        # hip_sad with its "Median test" property at N (include/ofps_hip.h N1v); with --sad-consistency C also on top of "Consistency check"
        combos[2:2] = [(f"hip_sad_v{limit}", HipSadDecoder, False, {"Median test": limit}), (f"hip_sad_v{limit}", HipSadDecoder, True, {"Median test": limit})]
        if sad_consistency:
            props_cv = {"Consistency check": sad_consistency, "Median test": limit}
            combos[2:2] = [(f"hip_sad_cv{limit}", HipSadDecoder, False, props_cv), (f"hip_sad_cv{limit}", HipSadDecoder, True, props_cv)]
    for ratio in sad_intra:         # hip_sad with its "Intra test" property at Q (include/ofps_hip.h N1i), "Scene cut" at --sad-cut
        props_i = {"Intra test": ratio, "Scene cut": sad_cut}
        combos[2:2] = [(f"hip_sad_i{ratio}", HipSadDecoder, False, props_i), (f"hip_sad_i{ratio}", HipSadDecoder, True, props_i)]
        if sad_prefilter:           # ... and on top of "Mean removal" at the first --sad-prefilter radius: filtered SAD against raw activity
            props_fi = dict(props_i, **{"Mean removal": sad_prefilter[0]})
            combos[2:2] = [(f"hip_sad_fi{ratio}", HipSadDecoder, False, props_fi), (f"hip_sad_fi{ratio}", HipSadDecoder, True, props_fi)]
    for thr in sad_split:           # hip_sad with its "Split blocks" property at T (include/ofps_hip.h N1s); with --sad-median N also on top of "Median test" at the first N
        combos[2:2] = [(f"hip_sad_b{thr}", HipSadDecoder, False, {"Split blocks": thr}), (f"hip_sad_b{thr}", HipSadDecoder, True, {"Split blocks": thr})]
        if sad_median:
            props_xb = {"Median test": sad_median[0], "Split blocks": thr}
            combos[2:2] = [(f"hip_sad_xb{thr}", HipSadDecoder, False, props_xb), (f"hip_sad_xb{thr}", HipSadDecoder, True, props_xb)]
    if sad_only:
        combos = [c for c in combos if c[1] is HipSadDecoder]
    if klt:             # the sparse decoder (include/ofps_hip.h N3): its defaults, and every other pair of "Cell size" and "Max residual" asked for
        for cell in klt_cells:
            for limit in klt_residuals:
                tag = "hip_klt" if (cell, limit) == (16, 0) else f"hip_klt_c{cell}r{limit}"
                props_k = {"Cell size": cell, "Max residual": limit}
                combos += [(tag, HipKltDecoder, False, props_k), (tag, HipKltDecoder, True, props_k)]
                if klt_mean_removal:        # ... and the same once more with "Mean removal" on (include/ofps_hip.h N3m)
                    props_km = dict(props_k, **{"Mean removal": True})
                    combos += [(tag + "_m", HipKltDecoder, False, props_km), (tag + "_m", HipKltDecoder, True, props_km)]
                for fb in klt_fb:           # ... and once more per limit of the forward-backward check (include/ofps_hip.h N3f)
                    props_kf = dict(props_k, **{"Consistency check": fb})
                    combos += [(f"{tag}_f{fb}", HipKltDecoder, False, props_kf), (f"{tag}_f{fb}", HipKltDecoder, True, props_kf)]
                    if klt_mean_removal:
                        props_kfm = dict(props_kf, **{"Mean removal": True})
                        combos += [(f"{tag}_f{fb}_m", HipKltDecoder, False, props_kfm), (f"{tag}_f{fb}_m", HipKltDecoder, True, props_kfm)]
    if klt and klt_intra:       # every hip_klt column once more per ratio of the intra test (include/ofps_hip.h N3i), "Scene cut" at --klt-cut, as <column>_i<Q>
        combos += [(f"{c[0]}_i{q}", c[1], c[2], dict(c[3], **{"Intra test": q, "Scene cut": klt_cut})) for q in klt_intra for c in combos if c[1] is HipKltDecoder]
    if klt and klt_predict:     # every hip_klt column once more with "Prediction" on (include/ofps_hip.h N3p), as <column>_p
        combos += [(c[0] + "_p", c[1], c[2], dict(c[3], **{"Prediction": True})) for c in combos if c[1] is HipKltDecoder]
    if klt and klt_levels:      # ... and all of them at another number of pyramid levels
        combos = [(c[0], c[1], c[2], dict(c[3], **{"Levels": klt_levels})) if c[1] is HipKltDecoder else c for c in combos]
    combos = [c for c in combos if c[0] not in skip]
    res = {}
    clips = []
    for name, geom in clip_table(quick, fast_clips, ramp_clips).items():
        if only and name not in only:
            continue
        clip_seed = 21 + len({c[2] for c in clips})                # the n-th clip that runs renders with seed 21 + n
        for light in lighting:                                      # the clip once per --lighting, rendered once
            tag = "" if light == "none" else "@" + light
            clips.append((name + tag, geom, clip_seed, False, light))
            if sad_gate:
                clips.append((name + "_flat_third" + tag, geom, clip_seed, True, light))
    if cut_clip and (not only or CUT_CLIP in only):                 # behind every other clip: their seeds stay what they are
        for light in lighting:
            clips.append((CUT_CLIP + ("" if light == "none" else "@" + light), clip_table(quick)["pan_0.2"], CUT_SEEDS[0], False, light))
    rendered = (None, None)
    for name, (W, H, fov, eul, dis), clip_seed, flat, light in clips:
        t0 = time.perf_counter()
        if rendered[0] != (name.split("@")[0].replace("_flat_third", ""), clip_seed):
            rendered = ((name.split("@")[0].replace("_flat_third", ""), clip_seed), synth.rotation_clip(eul, W, H, fov, seed=clip_seed, distractor=dis))
            if rendered[0][0] == CUT_CLIP:                          # the second half of the frames from another canvas
                other = synth.rotation_clip(eul, W, H, fov, seed=CUT_SEEDS[1], distractor=dis)[0]
                half = len(other) // 2
                rendered = (rendered[0], (np.concatenate([rendered[1][0][:half], other[half:]]), rendered[1][1]))
        frames, truth = rendered[1]
        if flat:
            frames = flat_third(frames)
        frames = relight_clip(frames, light)
        t_render = time.perf_counter() - t0
        cam = StandardCamera(W / H, fov)
        row = {"geometry": f"{W}x{H}", "fov_y_deg": fov, "frames": len(frames), "px_per_deg_at_centre": round(H / 2 / np.tan(np.radians(fov) / 2) * np.radians(1.0), 2),
               "dynamic_object": bool(dis), "render_s": round(t_render, 1)}
        per_pair = {}
        for dname, dcls, ransac, props in combos:
            q, rot, dt = track(frames, cam, dcls, ransac, **props)
            assert len(q) == len(truth), (len(q), len(truth))
            key = f"{dname}+{'ransac' if ransac else 'lsq'}"
            row[key] = dict(stats(q, truth), ms_per_frame=round(dt * 1e3, 3))
            if name.split("@")[0] == CUT_CLIP:                      # pair k relates frames k and k + 1: the cut lies in pair len(frames) // 2 - 1
                row[key]["cut_pair_err_deg"] = float(synth.quat_angle_deg(q[len(frames) // 2 - 1], truth[len(frames) // 2 - 1]))
            per_pair[key] = q
        if with_oracle:
            import oracle
            ocam = oracle.camera(W / H, fov)
            qo = np.array([oracle.solve_ypr_given(oracle.sad_flow(frames[k], frames[k + 1], 16, 16, threads=min(16, oracle.num_threads()))[0], ocam)
                           for k in range(len(truth))])
            row["cpu_oracle:sad+lsq"] = dict(stats(qo, truth), max_abs_dq_vs_hip=float(np.abs(qo - per_pair["hip_sad+lsq"]).max()))
            m = min(oracle_lk_pairs, len(truth)) if "hip_lk+lsq" in per_pair else 0
            ql = []
            for k in range(m):
                flow = oracle.lk_flow(frames[k], frames[k + 1], 3, 4, 3)
                ent = oracle.densify_to_entries(oracle.masked_flow_to_entries(flow, oracle.contrast_mask(frames[k + 1])), 150, 84)
                ql.append(oracle.solve_ypr_given(ent, ocam))
            ql = np.array(ql)
            if m:
                row["cpu_oracle:lk+lsq"] = {"pairs": m, "mean_err_deg": float(np.mean([synth.quat_angle_deg(a, b) for a, b in zip(ql, truth[:m])])),
                                            "max_abs_dq_vs_hip": float(np.abs(ql - per_pair["hip_lk+lsq"][:m]).max())}
        res[name] = row
        log(f"[accuracy] {name}: " + "  ".join(f"{k} {v['mean_err_deg']:.4f}" for k, v in row.items() if isinstance(v, dict) and "mean_err_deg" in v))
    return res


def table(res):
    cols = ["hip_sad+lsq", "hip_sad+ransac", "hip_lk+lsq", "hip_lk+ransac", "hip_lk5+lsq", "hip_lk5+ransac", "hip_flow+lsq", "hip_flow+ransac",
            "cpu_oracle:sad+lsq"]
    if any("hip_sad_q+lsq" in r for r in res.values()):
        cols[2:2] = ["hip_sad_q+lsq", "hip_sad_q+ransac"]
    if any("hip_sad_g+lsq" in r for r in res.values()):
        cols[2:2] = ["hip_sad_g+lsq", "hip_sad_g+ransac"]
    radii = sorted({int(k.split("+")[0].rsplit("m", 1)[1]) for r in res.values() for k in r if k.startswith(("hip_sad_m", "hip_sad_hm"))})
    limits = sorted({int(k.split("+")[0].rsplit("v", 1)[1]) for r in res.values() for k in r if k.startswith(("hip_sad_v", "hip_sad_cv"))})
    ratios = sorted({int(k.split("+")[0].rsplit("i", 1)[1]) for r in res.values() for k in r if k.startswith("hip_sad_i")})
    splits = sorted({int(k.split("+")[0].rsplit("b", 1)[1]) for r in res.values() for k in r if k.startswith(("hip_sad_b", "hip_sad_xb"))})
    for tag in tuple(f"hip_sad_{t}{thr}" for thr in reversed(splits) for t in ("xb", "b")) + tuple(f"hip_sad_{t}{ratio}" for ratio in reversed(ratios) for t in ("fi", "i")) + tuple(f"hip_sad_{t}{limit}" for limit in reversed(limits) for t in ("cv", "v")) + (
            "hip_sad_c", "hip_sad_qc", "hip_sad_h", "hip_sad_qh", "hip_sad_hp", "hip_sad_hpc", "hip_sad_qhp") + tuple(
            f"hip_sad_{t}{radius}" for radius in reversed(radii) for t in ("hm", "m")):
        if any(tag + "+lsq" in r for r in res.values()):
            cols[2:2] = [tag + "+lsq", tag + "+ransac"]
    if not any("hip_lk+lsq" in r for r in res.values()):       # --sad-only: no dense decoder ran
        cols = [c for c in cols if c.startswith(("hip_sad", "cpu_oracle"))]
    klt_cols = sorted({k for r in res.values() for k in r if k.startswith("hip_klt")}, key=lambda k: (k.split("+")[0], k.endswith("ransac")))
    cols[len(cols) - 1:len(cols) - 1] = klt_cols                   # in front of the CPU oracle's column
    lines = []
    lines.append("mean rotation error per frame, degrees (docs/statistics/err_av.csv's unit); clip rows, decoder+estimator columns")
    lines.append("clip,geometry,mean_rot_deg_per_frame,px_per_deg," + ",".join(cols))
    for name, r in res.items():
        lines.append(f"{name},{r['geometry']},{r['hip_sad+lsq']['mean_rot_deg']:.4f},{r['px_per_deg_at_centre']}," +
                     ",".join(f"{r[c]['mean_err_deg']:.5f}" if c in r else "" for c in cols))
    lines.append("")
    lines.append("the same as a fraction of the clip's mean rotation per frame (the reference's unit-test bound: < 0.10, almeida-estimator/src/lib.rs:347-348)")
    lines.append("clip," + ",".join(cols))
    for name, r in res.items():
        lines.append(f"{name}," + ",".join(f"{r[c]['rel_mean']:.4f}" if c in r and r[c].get("rel_mean") is not None else "" for c in cols))
    lines.append("")
    lines.append("max error of a single frame, degrees")
    lines.append("clip," + ",".join(cols))
    for name, r in res.items():
        lines.append(f"{name}," + ",".join(f"{r[c]['max_err_deg']:.5f}" if c in r else "" for c in cols))
    lines.append("")
    lines.append("pose drift after the last frame, degrees (motion_step accumulation, ofps/src/estimator.rs:38-53, vs the planted rotations accumulated the same way)")
    lines.append("clip,frames," + ",".join(cols))
    for name, r in res.items():
        lines.append(f"{name},{r['frames']}," + ",".join(f"{r[c]['drift_deg']:.4f}" if c in r else "" for c in cols))
    lines.append("")
    if any(CUT_CLIP in name for name in res):
        lines.append("error of the pair across the scene cut, degrees (the planted rotation of that pair is the clip's rate)")
        lines.append("clip," + ",".join(cols))
        for name, r in res.items():
            if CUT_CLIP in name:
                lines.append(f"{name}," + ",".join(f"{r[c]['cut_pair_err_deg']:.5f}" if c in r and "cut_pair_err_deg" in r[c] else "" for c in cols))
        lines.append("")
    lines.append("HIP chain vs CPU oracle chain on the same frames: largest |dq| component (sad+lsq: every pair; lk+lsq: the first pairs); tracking-loop ms per frame (host loop incl. PCIe)")
    lines.append("clip,sad+lsq_max_abs_dq,lk+lsq_max_abs_dq,lk_pairs_checked,ms_per_frame_hip_sad+lsq,ms_per_frame_hip_lk+lsq,ms_per_frame_hip_sad+ransac")
    for name, r in res.items():
        a, b = r.get("cpu_oracle:sad+lsq", {}), r.get("cpu_oracle:lk+lsq", {})
        lines.append(f"{name},{a.get('max_abs_dq_vs_hip', float('nan')):.2e},{b.get('max_abs_dq_vs_hip', float('nan')):.2e},{b.get('pairs', 0)},"
                     f"{r['hip_sad+lsq']['ms_per_frame']},{r.get('hip_lk+lsq', {}).get('ms_per_frame', '')},{r['hip_sad+ransac']['ms_per_frame']}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="24 frames per clip instead of 60 (what the -m gpu test runs)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--oracle-lk-pairs", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--quarter-pel", action="store_true", help="add the hip_sad_q columns: hip_sad with \"Quarter pel\" on")
    ap.add_argument("--sad-gate", type=int, default=0, metavar="N",
                    help="add the hip_sad_g columns (hip_sad with \"Contrast gate\" = N) and a variant of every clip with a flat noisy right third")
    ap.add_argument("--sad-consistency", type=int, default=0, metavar="N",
                    help="add the hip_sad_c columns (hip_sad with \"Consistency check\" = N; with --quarter-pel also hip_sad_qc: on top of \"Quarter pel\")")
    ap.add_argument("--sad-levels", type=int, default=0, metavar="N",
                    help="add the hip_sad_h columns (hip_sad with \"Search levels\" = N; with --quarter-pel also hip_sad_qh: on top of \"Quarter pel\")")
    ap.add_argument("--sad-predictors", type=int, default=0, choices=[0, 1],
                    help="with --sad-levels N: 1 adds the hip_sad_hp columns beside hip_sad_h (\"Search levels\" = N with \"Neighbour predictors\" on; with "
                         "--sad-consistency also hip_sad_hpc, with --quarter-pel also hip_sad_qhp); 0 = hip_sad_h alone")
    ap.add_argument("--lighting", nargs="+", default=["none"], choices=["none", "step", "flicker", "ramp"],
                    help="run every clip once per lighting (rendered once): none, step (+20 every other 4 frames), flicker (+-12 alternating), "
                         "ramp (a gradient on odd frames)")
    ap.add_argument("--sad-prefilter", nargs="*", type=int, default=[], metavar="R",
                    help="add the hip_sad_m<R> columns (hip_sad with \"Mean removal\" = R; with --sad-levels N also hip_sad_hm<R>: on top of \"Search levels\")")
    ap.add_argument("--sad-median", nargs="*", type=int, default=[], metavar="N",
                    help="add the hip_sad_v<N> columns (hip_sad with \"Median test\" = N; with --sad-consistency C also hip_sad_cv<N>: on top of \"Consistency check\")")
    ap.add_argument("--sad-intra", nargs="*", type=int, default=[], metavar="Q",
                    help="add the hip_sad_i<Q> columns (hip_sad with \"Intra test\" = Q sixteenths; --sad-cut P sets \"Scene cut\" = P in them)")
    ap.add_argument("--sad-split", nargs="*", type=int, default=[], metavar="T",
                    help="add the hip_sad_b<T> columns (hip_sad with \"Split blocks\" = T sixteenths; with --sad-median N also hip_sad_xb<T>: on top of \"Median test\" = N)")
    ap.add_argument("--sad-cut", type=int, default=0, metavar="P", help="\"Scene cut\" of the hip_sad_i<Q> columns, percent (0 = off)")
    ap.add_argument("--cut-clip", action="store_true", help="add pan_0.2_cut: pan_0.2 with the second half of its frames from another canvas seed")
    ap.add_argument("--fast-clips", action="store_true", help="add 1080p pans of 1.5 and 3 degrees per frame: beyond the plain search's reach")
    ap.add_argument("--sad-only", action="store_true", help="only the hip_sad columns (the dense decoders take most of the run time)")
    ap.add_argument("--klt", action="store_true", help="add the hip_klt columns: the sparse decoder with its defaults (also with --sad-only)")
    ap.add_argument("--klt-cell", nargs="*", type=int, default=[16], metavar="C", help="with --klt: \"Cell size\" values; hip_klt_c<C>r<R> beside hip_klt")
    ap.add_argument("--klt-residual", nargs="*", type=int, default=[0], metavar="R", help="with --klt: \"Max residual\" values (sixteenths of a grey level)")
    ap.add_argument("--klt-mean-removal", action="store_true", help="with --klt: every hip_klt column once more with \"Mean removal\" on, as <column>_m")
    ap.add_argument("--klt-fb", nargs="*", type=int, default=[], metavar="N", help="with --klt: \"Consistency check\" values in 1/256 pixel; hip_klt_f<N> beside hip_klt")
    ap.add_argument("--klt-intra", nargs="*", type=int, default=[], metavar="Q", help="with --klt: \"Intra test\" ratios in sixteenths; <column>_i<Q> beside every hip_klt column")
    ap.add_argument("--klt-cut", type=int, default=0, metavar="P", help="\"Scene cut\" of the <column>_i<Q> columns, percent (0 = off)")
    ap.add_argument("--klt-predict", action="store_true", help="with --klt: every hip_klt column once more with \"Prediction\" on, as <column>_p")
    ap.add_argument("--klt-levels", type=int, default=0, metavar="L", help="with --klt: \"Levels\" of every hip_klt column (0 = the decoder's 4)")
    ap.add_argument("--ramp-clips", action="store_true", help="add 1080p pans whose rate grows linearly from 0 to 1.5 and to 3 degrees per frame and falls back")
    ap.add_argument("--skip", nargs="*", default=[], metavar="NAME", help="decoder columns to leave out, e.g. hip_lk5 hip_flow")
    args = ap.parse_args()
    res = run(args.quick, args.oracle_lk_pairs, not args.no_oracle, args.only, log=lambda s: print(s, file=sys.stderr, flush=True), quarter_pel=args.quarter_pel,
              sad_gate=args.sad_gate, sad_consistency=args.sad_consistency, sad_levels=args.sad_levels, fast_clips=args.fast_clips,
              sad_only=args.sad_only, sad_predictors=args.sad_predictors, lighting=tuple(args.lighting), sad_prefilter=tuple(args.sad_prefilter),
              sad_median=tuple(args.sad_median), sad_intra=tuple(args.sad_intra), sad_cut=args.sad_cut, cut_clip=args.cut_clip, sad_split=tuple(args.sad_split),
              klt=args.klt, klt_cells=tuple(args.klt_cell), klt_residuals=tuple(args.klt_residual), skip=tuple(args.skip),
              klt_mean_removal=args.klt_mean_removal, klt_fb=tuple(args.klt_fb), klt_predict=args.klt_predict, ramp_clips=args.ramp_clips,
              klt_levels=args.klt_levels, klt_intra=tuple(args.klt_intra), klt_cut=args.klt_cut)
    txt = table(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(__doc__.split("\n\n  python")[0] + "\n\n" + txt)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
