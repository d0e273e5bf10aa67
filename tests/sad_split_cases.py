"""Cases for hip_sad's split blocks (include/ofps_hip.h N1s).  CPU only: numpy, ofps_amd/synth.py's value noise and the restatements
tests/indep_sad_split.py / tests/indep_sad_prefilter.py (the parents: its plain N1 search) -- never the library under test.
tests/test_sad_split_cpu.py pins that the cases hold of the restatement alone; tests/test_sad_split_gpu.py runs them.
Everything is computed once per process and handed out read-only."""
from functools import lru_cache

import numpy as np

from ofps_amd import synth

import indep_sad_prefilter as ipf
import indep_sad_split as isp

THRESHOLDS = (1, 16, 256, 4080)
MARGIN = 16                                              # of the canvas around the frame: above every |d| planted
D_LEFT, D_RIGHT = (2, 0), (-3, 1)                        # the two motions of the boundary scenes: cur(x, y) = prev(x + dx, y + dy)


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=8)
def canvas(W, H, seed=77):
    """value noise (octaves of 64, 16 and 4 px), scaled to 16..235 -> int64 [H + 2 * MARGIN, W + 2 * MARGIN], read-only"""
    t = synth._texture_grid(np.arange(W + 2 * MARGIN, dtype=np.int64), np.arange(H + 2 * MARGIN, dtype=np.int64), seed)
    t = (t - t.min()) / (t.max() - t.min())
    return _ro(np.floor(16.0 + t.astype(np.float64) * 219.0 + 0.5), np.int64)


def moved(W, H, regions, seed=77):
    """prev = the canvas cut at the margin; cur built per pixel: cur(x, y) = prev(x + dx, y + dy) with (dx, dy) of the first region
    (x_end, (dx, dy)) whose x_end lies right of x.  Noise-free -> (prev, cur) uint8, read-only"""
    c = canvas(W, H, seed)
    M = MARGIN
    prev = c[M:M + H, M:M + W]
    cur = np.empty((H, W), np.int64)
    x_begin = 0
    for x_end, (dx, dy) in regions:
        cur[:, x_begin:x_end] = c[M + dy:M + dy + H, M + dx:M + dx + W][:, x_begin:x_end]
        x_begin = x_end
    assert x_begin == W
    return _ro(prev, np.uint8), _ro(cur, np.uint8)


def boundary_pair(W, H, boundary):
    return moved(W, H, ((boundary, D_LEFT), (W, D_RIGHT)))


def flat_pair(W=64, H=48):
    f = np.full((H, W), 128, np.uint8)
    return _ro(f, np.uint8), _ro(f, np.uint8)


def noise_pair(W=64, H=48, seed=5):
    """a pair identical but for noise in {-1, 0, 1}"""
    prev = canvas(W, H)[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    cur = prev + np.random.default_rng(seed).integers(-1, 2, prev.shape)
    assert cur.min() >= 0 and cur.max() <= 255
    return _ro(prev, np.uint8), _ro(cur, np.uint8)


# name -> (pair, block, range).  Every path of the kernel: the packed forms (B 16, B 8) with all predictors inside the frame and more
# than one workgroup of four waves; the staged form through a clamped predictor (the corner scenes) and through the generic block sizes
CASES = {
    "boundary24": (lambda: boundary_pair(64, 48, 24), 16, 8),        # the boundary on a sub-block edge inside block column 1
    "boundary28": (lambda: boundary_pair(64, 48, 28), 16, 8),        # ... inside a sub-block
    "flat": (flat_pair, 16, 8),
    "noise_only": (noise_pair, 16, 8),
    "ragged": (lambda: boundary_pair(70, 50, 24), 16, 8),            # margins of 6 and 2 pixels that belong to no block
    "one_block": (lambda: boundary_pair(16, 16, 8), 16, 8),          # no neighbours: the block's winner and zero
    "small_blocks": (lambda: boundary_pair(48, 32, 20), 8, 8),       # b = 4
    "generic32": (lambda: boundary_pair(96, 64, 48), 32, 4),
    "generic12": (lambda: boundary_pair(60, 36, 30), 12, 8),         # b = 6
    "corner_minus": (lambda: moved(64, 48, ((64, (-8, -8)),)), 16, 8),   # interior winners (-8, -8) beside border blocks that cannot hold them:
    "corner_plus": (lambda: moved(64, 48, ((64, (8, 8)),)), 16, 8),      # a sub-block's clamp of a neighbour's winner differs from its sibling's
}
PAD = 12                                                 # the padded-rows form of every case: stride = W + 12


@lru_cache(maxsize=32)
def pair(name):
    return CASES[name][0]()


def geometry(name):
    prev, _ = pair(name)
    H, W = prev.shape
    return W, H, CASES[name][1], CASES[name][2]


@lru_cache(maxsize=32)
def parents(name):
    """the plain N1 search's integer winners -> int32 [nblk, 3], read-only"""
    prev, cur = pair(name)
    _, _, B, R = geometry(name)
    return _ro(ipf.full_search(prev, cur, B, R), np.int32)


def keep_pattern(nblk):
    """a keep array with dropped blocks beside kept ones: every third block dropped"""
    return _ro((np.arange(nblk) % 3 != 1), np.uint8)


@lru_cache(maxsize=128)
def expect(name, T, with_keep=False):
    """case `name` through the restatement at threshold T -> its dict, arrays read-only"""
    prev, cur = pair(name)
    _, _, B, R = geometry(name)
    best = parents(name)
    keep = keep_pattern(len(best)) if with_keep else None
    step = isp.split_step(prev, cur, B, best, keep, R, T)
    return {k: _ro(v, v.dtype) for k, v in step.items()}


def padded(a, pad=PAD):
    """-> a view of the frame inside a buffer with rows of W + pad bytes (the padding holds 255: reading it would show)"""
    H, W = a.shape
    buf = np.full((H, W + pad), 255, np.uint8)
    buf[:, :W] = a
    return buf[:, :W]


# ---- synthetic parents for the step alone: whatever the triples hold, a predictor ends inside the frame
def wild_parents(nblk, seed=3):
    rng = np.random.default_rng(seed)
    best = np.zeros((nblk, 3), np.int32)
    best[:, 0] = rng.integers(-8, 9, nblk); best[:, 1] = rng.integers(-8, 9, nblk)
    best[:, 2] = rng.integers(0, 4000, nblk)
    best[::5, 0] = 2 ** 31 - 1; best[1::5, 1] = -2 ** 31; best[2::5, 2] = -7       # out of every range, and a negative SAD
    return _ro(best, np.int32)


# ---- the rule of the boundary scenes: a sub-block wholly inside one region, its true vector valid, returns that vector with SAD 0
def true_vectors(name, boundary):
    """-> (under bool [nblk, 4], want int [nblk, 4, 2])"""
    W, H, B, _ = geometry(name)
    nbx, nby, b = W // B, H // B, B // 2
    under = np.zeros((nbx * nby, 4), bool)
    want = np.zeros((nbx * nby, 4, 2), np.int64)
    for k in range(nbx * nby):
        for s in range(4):
            sx0, sy0 = (k % nbx) * B + (s & 1) * b, (k // nbx) * B + (s >> 1) * b
            if sx0 + b <= boundary:
                d = D_LEFT
            elif sx0 >= boundary:
                d = D_RIGHT
            else:
                continue
            want[k, s] = d
            under[k, s] = 0 <= sx0 + d[0] <= W - b and 0 <= sy0 + d[1] <= H - b
    return under, want


# ---- the fused forms' stream: 128 x 96, a rectangle that moves against a pan
STREAM_W, STREAM_H, STREAM_B, STREAM_R = 128, 96, 16, 8
STREAM_FRAMES = 4
STREAM_PAN, STREAM_OBJ = (2, 1), (-3, 2)                 # per frame
STREAM_RECT = (40, 24, 88, 72)                           # x0, y0, x1, y1: edges on sub-block lines and inside sub-blocks alike
STREAM_CAM = (STREAM_W / STREAM_H, 30.0)
STREAM_DETECTOR = dict(min_size=0.05, subdivide=2, target_motion=0.003)
STREAM_T = 16


@lru_cache(maxsize=1)
def stream():
    """-> uint8 [STREAM_FRAMES, H, W], read-only: frame k + 1 is frame k with the background displaced by the pan and the rectangle's
    content displaced by the object's motion"""
    W, H = STREAM_W, STREAM_H
    M = 4 * 4 + 8
    t = synth._texture_grid(np.arange(W + 2 * M, dtype=np.int64), np.arange(H + 2 * M, dtype=np.int64), 91)
    t = (t - t.min()) / (t.max() - t.min())
    c = np.floor(16.0 + t.astype(np.float64) * 219.0 + 0.5).astype(np.int64)
    t2 = synth._texture_grid(np.arange(W + 2 * M, dtype=np.int64) + 1000, np.arange(H + 2 * M, dtype=np.int64) + 500, 92)
    t2 = (t2 - t2.min()) / (t2.max() - t2.min())
    c2 = np.floor(16.0 + t2.astype(np.float64) * 219.0 + 0.5).astype(np.int64)
    x0, y0, x1, y1 = STREAM_RECT
    out = np.empty((STREAM_FRAMES, H, W), np.int64)
    for k in range(STREAM_FRAMES):
        f = c[M - k * STREAM_PAN[1]:M - k * STREAM_PAN[1] + H, M - k * STREAM_PAN[0]:M - k * STREAM_PAN[0] + W].copy()
        obj = c2[M - k * STREAM_OBJ[1]:M - k * STREAM_OBJ[1] + H, M - k * STREAM_OBJ[0]:M - k * STREAM_OBJ[0] + W]
        f[y0:y1, x0:x1] = obj[y0:y1, x0:x1]
        out[k] = f
    return _ro(out, np.uint8)
