"""Cases for the dense decoders' fused form (ofps_hip_lk_push_frame_fused[_async]: decoder -> detector + estimator in one ticket, the record
count staying on the device).  CPU only: numpy, the synthetic frames of tests/dense_output_cases.py and the CPU oracle -- never the library
under test.  Expected values are the stage-wise chain on the oracle: the oracle's records of the pair -> oracle detector, oracle least squares /
oracle RANSAC with the same seed.  tests/test_dense_fused_cpu.py checks the properties the cases are named for; tests/test_dense_fused_gpu.py
runs them."""
from functools import lru_cache

import numpy as np

import dense_output_cases as dc
import oracle

W, H = 480, 270
LK = (1, 2, 1)                    # levels, radius, iters: the flow is not what is tested here
FB = (5, 6, 3)                    # cv-decoder's Farneback call (cv-decoder/src/lib.rs:188-199)
CAM = (16 / 9, 39.6 * 9 / 16)
DETECTOR = dict(min_size=0.05, subdivide=3, target_motion=0.003)             # a 14 x 14 field: the densifier's one-pass sort / small path
DETECTOR_FINE = dict(min_size=0.05, subdivide=5, target_motion=0.003)        # 23 x 23 = 529 cells: more than 256, the two-pass sort
INLIER_DEG = 0.2
RANSAC_ITERS = 12
SEED = 11

# (cap) -> the record grid at 480 x 270 and the solver class its capacity falls in (almeida.hip: lsq_device / lsq_cluster)
DOWNSAMPLED_CAPS = {(24, 24): (24, 13), (48, 48): (48, 27), (64, 64): (64, 36), (100, 100): (100, 56), (150, 150): (150, 84)}
REDUCED_CAPS = {(150, 150): (150, 84), (300, 300): (300, 168), (480, 270): (480, 270)}
CASES = tuple((cap, False) for cap in DOWNSAMPLED_CAPS) + tuple((cap, True) for cap in REDUCED_CAPS)      # (cap, reduced)
DEFAULT_CAP = (150, 150)

KINDS = ("flat", "noise", "impulse", "halfflat", "texture")
# The frames above are unrelated to each other: a one-level, one-iteration LK finds next to no flow between them, so the oracle's detector
# answers None and its quaternions are the identity to 1e-9 -- expectations that an empty field or an estimator that did nothing would meet.
# The "move" frames are ONE smooth content (noise box-filtered twice, 9 taps, stretched to full contrast: features of ~10 pixels, inside the
# reach of a radius-2 window) moved by (3, 3) pixels per frame: "move0", "move1", and "movehalf" = flat on the left half, the content moved
# once more on the right.  Pairs move0 -> move1 and move1 -> movehalf carry a real, coherent flow: an island of most of the field and a
# rotation more than 1e-3 from the identity (tests/test_dense_fused_cpu.py pins both per capacity).
MOVE = ("move0", "move1", "movehalf")
MOVE_STEP, MOVE_BLUR, MOVE_MARGIN = 3, 9, 32
MOTION_PAIRS = (("move0", "move1"), ("move1", "movehalf"))
# consecutive tickets: 0, everything, a few dozen, under half, about half; then a real flow over most of the frame and over its right half
STREAM_CYCLE = ("flat", "noise", "impulse", "halfflat", "texture") + MOVE
# one weight-4 impulse (amplitude 6: a 10 x 10 box of mask) and the same frame moved by a pixel: under a (12, 12) cap -- cells of 40 x 45
# pixels -- the box falls into one cell or straddles two
FEW_CAP = (12, 12)
FEW_IMPULSES = {1: (145, 255), 2: (140, 250)}            # records -> (y, x)


@lru_cache(maxsize=4)
def _move_content(w, h):
    from ofps_amd import synth
    c = synth.random_luma(1, w + 2 * MOVE_MARGIN, h + 2 * MOVE_MARGIN, seed=77)[0].astype(np.float32)
    k = np.ones(MOVE_BLUR, np.float32) / MOVE_BLUR
    for _ in range(2):
        for axis in (0, 1):
            c = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, c)
    return ((c - c.min()) / (c.max() - c.min()) * 255).astype(np.uint8)


@lru_cache(maxsize=32)
def frame(kind, w=W, h=H):
    """dense_output_cases' stream frames plus one that is flat on the left half and textured on the right"""
    if kind == "halfflat":
        f = np.full((h, w), dc.BG, np.uint8)
        f[:, w // 2:] = dc.stream_frame(w, h, "texture")[:, w // 2:]
        f.setflags(write=False)
        return f
    if kind in MOVE:
        step = MOVE_STEP * MOVE.index(kind)
        o = MOVE_MARGIN - step
        f = np.ascontiguousarray(_move_content(w, h)[o:o + h, o:o + w])
        if kind == "movehalf":
            f[:, :w // 2] = dc.BG
        f.setflags(write=False)
        return f
    if kind.startswith("few"):                          # "few1", "few2" and their previous frames "few1_prev", "few2_prev"
        y, x = FEW_IMPULSES[int(kind[3])]
        f = dc.impulse_frame(w, h, [(y, x, 6)])
        f = np.roll(f, (1, 1), (0, 1)) if kind.endswith("_prev") else f
        f.setflags(write=False)
        return f
    return dc.stream_frame(w, h, kind)


def bgr_of(luma):
    """a tinted colour frame whose flat regions stay flat"""
    return np.clip(luma[..., None].astype(int) + np.array([-20, 0, 15]), 0, 255).astype(np.uint8)


def samples_for(n_max):
    """RANSAC "samples" below every non-trivial count and above the capacity"""
    return (200, n_max + 1000)


@lru_cache(maxsize=64)
def _fullres_records(kind_prev, kind_cur, farneback, params, w, h):
    prev, cur = frame(kind_prev, w, h), frame(kind_cur, w, h)
    flow = oracle.farneback_flow(prev, cur, params[0], 2 * params[1] + 1, params[2]) if farneback else oracle.lk_flow(prev, cur, *params)
    return oracle.masked_flow_to_entries(flow, oracle.contrast_mask(cur))


@lru_cache(maxsize=256)
def records(kind_prev, kind_cur, cap, reduced, farneback=False, params=LK, w=W, h=H, fmt=0):
    """the oracle's records of the pair, mask on -> (records [n, 4] read-only, (grid_w, grid_h)).  Pairs on their own (zero initial flow)."""
    if reduced:
        prev, cur = frame(kind_prev, w, h), frame(kind_cur, w, h)
        if fmt == oracle.FMT_BGR:
            prev, cur = bgr_of(prev), bgr_of(cur)
        rec, grid, _ = oracle.cv_decode(prev, cur, fmt, process_fullres=False, max_w=cap[0], max_h=cap[1], flow="farneback" if farneback else "lk",
                                        levels=params[0], radius=params[1], iters=params[2])
    else:
        grid = oracle.cv_grid(w, h, *cap)
        rec = oracle.densify_to_entries(_fullres_records(kind_prev, kind_cur, farneback, params, w, h), *grid)
    rec = np.ascontiguousarray(rec, np.float32)
    rec.setflags(write=False)
    return rec, tuple(grid)


def tail_key(rec):
    return rec.tobytes()


@lru_cache(maxsize=256)
def _expected_detector(rec_bytes, detector):
    return oracle.detect_motion(np.frombuffer(rec_bytes, np.float32).reshape(-1, 4), **dict(detector))


@lru_cache(maxsize=256)
def _expected_quat(rec_bytes, use_ransac, num_samples, seed, inlier_deg):
    rec = np.frombuffer(rec_bytes, np.float32).reshape(-1, 4)
    cam = oracle.camera(*CAM)
    if use_ransac:
        q, inl = oracle.solve_ypr_ransac(rec, cam, RANSAC_ITERS, inlier_deg, num_samples, seed=seed, want_inliers=True)
        return np.asarray(q, np.float32), len(inl)
    return np.asarray(oracle.solve_ypr_given(rec, cam), np.float32), len(rec)


def expected(rec, use_ransac=False, num_samples=1000, seed=SEED, detector=None, inlier_deg=INLIER_DEG):
    """-> (oracle detector result: None | (area, field), oracle quaternion) of these records"""
    key = tail_key(rec)
    det = _expected_detector(key, tuple(sorted((detector or DETECTOR).items())))
    return det, _expected_quat(key, bool(use_ransac), int(num_samples), int(seed), float(inlier_deg))[0]


def refit_size(rec, num_samples, seed=SEED, inlier_deg=INLIER_DEG):
    """how many inliers the oracle's RANSAC re-solves on"""
    return _expected_quat(tail_key(rec), True, int(num_samples), int(seed), float(inlier_deg))[1]


def off_identity(q):
    return float(np.abs(np.asarray(q)[1:]).max())
