"""Cases for hip_sad's mean removal (include/ofps_hip.h N1m): the relit planted scenes, a relit sequence for the stream forms and the
filter-only frames.  CPU only: numpy, the scenes of tests/sad_hier_cases.py and the restatement tests/indep_sad_prefilter.py -- never the
library under test.  tests/test_sad_prefilter_cpu.py pins what holds of the restatement alone; tests/test_sad_prefilter_gpu.py runs them."""
from functools import lru_cache

import numpy as np

import indep_sad_prefilter as ip
import sad_hier_cases as hc

# ---- the planted shift INSIDE the range: (W, H, block, range, (dx, dy))
SCENES = ((192, 128, 16, 8, (5, -3)),
          (200, 136, 8, 8, (-6, 4)))
LIGHTINGS = ("step", "ramp", "gain")                     # +20; +30 x/(W-1) - 10 y/(H-1) - 8; 0.85 v + 12
RADII = (4, 8)
# (scene, lighting) -> interior blocks at r = 4 that the PLAIN search may return d for at the most; (scene, r) -> interior blocks
PLAIN_AT_MOST = {(0, "step"): 0, (0, "ramp"): 22, (0, "gain"): 28, (1, "step"): 1, (1, "ramp"): 80, (1, "gain"): 96}
INTERIOR = {(0, 4): 60, (0, 8): 60, (1, 4): 330, (1, 8): 308}
RADIUS = 4                                               # of the whole-search cases on the GPU
# the search levels' case: |d| beyond the range, relit by the step
BEYOND = (192, 128, 16, 8, 2, (15, -11))


def _ro(a, dtype=np.uint8):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


def relight(img, lighting):
    """floor(f(v) + 0.5) clamped to 0..255; f in float64, one operation order"""
    v = np.asarray(img, np.uint8).astype(np.float64)
    H, W = v.shape
    if lighting == "none":
        return _ro(img)
    if lighting == "step":
        f = v + 20.0
    elif lighting == "ramp":
        x = np.arange(W, dtype=np.float64)[None, :]; y = np.arange(H, dtype=np.float64)[:, None]
        f = v + (30.0 * x / (W - 1) - 10.0 * y / (H - 1) - 8.0)
    elif lighting == "gain":
        f = 0.85 * v + 12.0
    else:
        raise ValueError(lighting)
    return _ro(np.clip(np.floor(f + 0.5), 0, 255))


@lru_cache(maxsize=16)
def relit_pair(W, H, d, lighting):
    """hc.planted_pair with the current frame relit -> (prev, cur) read-only"""
    prev, cur = hc.planted_pair(W, H, d)
    return prev, relight(cur, lighting)


def interior(W, H, B, d, r):
    """-> bool [nblk]: the block and the block moved by d both lie at least r pixels from every frame border"""
    nbx, nby = W // B, H // B
    dx, dy = d
    x0 = np.arange(nbx) * B; y0 = np.arange(nby) * B
    okx = (x0 >= r) & (x0 + B <= W - r) & (x0 + dx >= r) & (x0 + dx + B <= W - r)
    oky = (y0 >= r) & (y0 + B <= H - r) & (y0 + dy >= r) & (y0 + dy + B <= H - r)
    return (oky[:, None] & okx[None, :]).reshape(-1)


def hits(best, d):
    return (best[:, 0] == d[0]) & (best[:, 1] == d[1])


@lru_cache(maxsize=32)
def filtered_pair(W, H, d, lighting, r):
    prev, cur = relit_pair(W, H, d, lighting)
    return _ro(ip.prefilter(prev, r)), _ro(ip.prefilter(cur, r))


@lru_cache(maxsize=32)
def expect(i, lighting, r):
    """scene i relit, through the restatement at radius r (0 = the plain search) -> (entries, best) read-only"""
    W, H, B, R, d = SCENES[i]
    prev, cur = relit_pair(W, H, d, lighting)
    ent, best = ip.search(prev, cur, B, R, r)
    return _ro(ent, np.float32), _ro(best, np.int32)


# ---- a sequence for the stream forms: scene 0's canvas walking by d per frame, every frame under another light
SEQ_W, SEQ_H, SEQ_B, SEQ_R, SEQ_D = SCENES[0]
SEQ_LIGHT = ("none", "step", "ramp", "none")
SEQ_NBLK = (SEQ_W // SEQ_B) * (SEQ_H // SEQ_B)
SEQ_CAM = (SEQ_W / SEQ_H, 22.275)
SEQ_DETECTOR = dict(min_size=0.05, subdivide=2, target_motion=0.003)
SEQ_RANSAC = dict(num_iters=100, inlier_deg=0.05, num_samples=240)
SEQ_SEED = 9


@lru_cache(maxsize=1)
def sequence():
    """uint8 [4, H, W]: frame k = the canvas cut at k * d, + noise in {-1, 0, 1} for k > 0, relit by SEQ_LIGHT[k]: pair (k - 1, k) moves by d"""
    c = hc.canvas(SEQ_W, SEQ_H)
    M = hc.MARGIN
    out = []
    for k, light in enumerate(SEQ_LIGHT):
        ox, oy = M + k * SEQ_D[0], M + k * SEQ_D[1]
        f = c[oy:oy + SEQ_H, ox:ox + SEQ_W].astype(np.int64)
        if k:
            f = f + np.random.default_rng(4000 + k).integers(-1, 2, f.shape)
        out.append(relight(np.clip(f, 0, 255).astype(np.uint8), light))
    return _ro(np.stack(out))


@lru_cache(maxsize=16)
def sequence_expect(a, b, r=RADIUS):
    """pair (a, b) of sequence() through the restatement -> (entries, best) read-only"""
    f = sequence()
    ent, best = ip.search(f[a], f[b], SEQ_B, SEQ_R, r)
    return _ro(ent, np.float32), _ro(best, np.int32)


# ---- the filter alone: (W, H, stride); frames smaller than the window among them
FILTER_SIZES = ((1, 1, 1), (5, 3, 5), (37, 23, 40), (64, 48, 64), (200, 136, 200))
FILTER_RADII = (1, 4, 16)
FILTER_KINDS = ("random", "flat0", "flat255", "blocks3")


def filter_frame(kind, W, H, stride):
    """-> uint8 [H, stride]; the stride margin always holds random junk that must not reach the result.  blocks3: a checkerboard of
    3 x 3 px blocks of 0 and 255, so that both clamps and the rounding of m act"""
    rng = np.random.default_rng(1000 * W + 10 * H + len(kind))
    f = rng.integers(0, 256, (H, stride), dtype=np.uint8)
    if kind == "flat0":
        f[:, :W] = 0
    elif kind == "flat255":
        f[:, :W] = 255
    elif kind == "blocks3":
        y, x = np.mgrid[0:H, 0:W]
        f[:, :W] = np.where(((x // 3) + (y // 3)) % 2 == 0, 0, 255)
    else:
        assert kind == "random"
    return f
