"""Cases for hip_sad's contrast gate (include/ofps_hip.h N1g: ofps_hip_block_contrast[_dev], ofps_hip_set_sad_gate, the gated
ofps_hip_sad_flow / ofps_hip_sad_flow_gated_dev and the gated fused per-frame path).  CPU only: numpy and the CPU oracle -- never the
library under test.

The restatement: oracle.contrast_mask(cur) -> per-block sums by reshaping -> count >= min_pixels -> filter, in raster order.
tests/test_sad_gate_cpu.py pins that these inputs can tell the gate from its absence; tests/test_sad_gate_gpu.py runs them."""
from functools import lru_cache

import numpy as np

import oracle

# ---- the kernel's geometries: (W, H, stride) x block 8 and 16 (the one-writer path), one generic geometry (the atomic path)
FRAME_SIZES = ((64, 16, 64),           # one tile
               (65, 17, 65), (63, 15, 63),     # tile edge +- 1, ragged margin
               (128, 32, 128),
               (80, 48, 96),           # padded stride
               (16, 16, 16), (8, 8, 8),        # smaller than the halo: reflect-101 folds twice
               (200, 120, 200))        # 120 / 16 = 7.5: 1080p's 67.5 block rows in miniature
LATTICE_BLOCKS = (8, 16)
GENERIC = (100, 60, 100, 12)           # block 12: blocks straddle the 64 x 16 tiles
CONTENTS = ("constant", "noise", "impulse", "checkerboard", "half_flat")


def content(kind, W, H, seed=0):
    """-> uint8 [H, W]"""
    rng = np.random.default_rng(7000 + seed + 13 * W + H)
    if kind == "constant":
        return np.full((H, W), 128, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "impulse":                                # one 2 x 2 impulse at a tile corner (the first tile's far corner when there is one)
        f = np.full((H, W), 40, np.uint8)
        y, x = min(15, H - 2), min(63, W - 2)
        f[y:y + 2, x:x + 2] = 255
        return f
    if kind == "checkerboard":                           # 3 x 3 squares: a period that divides neither tile nor block
        yy, xx = np.mgrid[0:H, 0:W]
        return np.where(((yy // 3) + (xx // 3)) % 2 == 0, 30, 220).astype(np.uint8)
    if kind == "half_flat":                              # texture on the left half, constant on the right
        f = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f[:, W // 2:] = 128
        return f
    raise ValueError(kind)


# ---- the restatement
def block_counts(luma, block):
    """-> uint32 [H // block, W // block]: set pixels of the contrast mask of `luma` per full lattice block"""
    m = oracle.contrast_mask(luma)
    H, W = m.shape
    nby, nbx = H // block, W // block
    return m[:nby * block, :nbx * block].reshape(nby, block, nbx, block).sum(axis=(1, 3), dtype=np.uint32)


def block_counts_loops(luma, block):
    """the same count written as loops over blocks and pixels (the check of the reshaping)"""
    m = oracle.contrast_mask(luma)
    H, W = m.shape
    out = np.zeros((H // block, W // block), np.uint32)
    for by in range(H // block):
        for bx in range(W // block):
            c = 0
            for y in range(by * block, by * block + block):
                for x in range(bx * block, bx * block + block):
                    c += 1 if m[y, x] else 0
            out[by, bx] = c
    return out


def keep_flags(cur, block, min_pixels):
    """-> bool [nblk] in raster order"""
    return (block_counts(cur, block) >= min_pixels).reshape(-1)


def gate_filter(records, keep):
    """the kept rows of a per-block array, in raster order"""
    return np.ascontiguousarray(np.asarray(records)[keep])


# ---- the half-flat PAIR of the compaction cases: 96 x 64, texture moved by (2, 1) on the left half, constant on the right
PAIR_W, PAIR_H, PAIR_RANGE = 96, 64, 8


@lru_cache(maxsize=1)
def half_flat_pair():
    rng = np.random.default_rng(77)
    big = rng.integers(0, 256, (PAIR_H + 8, PAIR_W + 8), dtype=np.uint8)
    prev = big[4:4 + PAIR_H, 4:4 + PAIR_W].copy()
    cur = big[3:3 + PAIR_H, 2:2 + PAIR_W].copy()
    prev[:, PAIR_W // 2:] = 128
    cur[:, PAIR_W // 2:] = 128
    prev.setflags(write=False); cur.setflags(write=False)
    return prev, cur


# ---- the planted stream of the fused cases: 320 x 192 luma, block 16, range 8 -> 20 x 12 = 240 blocks.  The left 192 columns are smooth
# texture that moves by (3, 2) px per frame, the right 128 columns constant 128 plus seeded uniform noise, fresh in every frame.
# The geometry that holds (tests/test_sad_gate_cpu.py asserts it of the oracle alone): the split and the motion are the first proposal's,
# the noise is not.  Uniform +-2 noise trips the mask's threshold all over the flat side (the 5 x 5 mixed derivative weighs 36 in absolute
# sum: a sum above 20 is common at amplitude 2 and still possible at +-1) and the dilation then keeps all 240 blocks.  With noise levels
# {0, 1} the derivative is at most 18 -- its positive weights sum to 18 -- so no flat pixel ever passes: the flat side keeps only what the
# 11 x 11 dilation carries 5 px across the split (block column 12), and the full search still picks winners all over +-8 among the noise.
FRAME_W, FRAME_H, BLOCK, RANGE = 320, 192, 16, 8
NBLK = (FRAME_W // BLOCK) * (FRAME_H // BLOCK)
SPLIT = 192
NOISE_LEVELS = 2                                         # 128 + {0, 1}
STEP = (3, 2)
N_FRAMES = 4
GATE = 1                                                 # min_pixels of the planted cases
FRAME_CAM = (FRAME_W / FRAME_H, 22.275)
# 12 rows of vectors cannot fill the 14 rows of the detector's default field: 9 x 9 (subdivide 2), as the compensation stage's fused case
FRAME_DETECTOR = dict(min_size=0.05, subdivide=2, target_motion=0.003)
FRAME_RANSAC = dict(num_iters=100, inlier_deg=0.05, num_samples=240)
SEED = 5


@lru_cache(maxsize=1)
def _texture():
    from ofps_amd import synth
    margin = 32
    c = synth.random_luma(1, FRAME_W + 2 * margin, FRAME_H + 2 * margin, seed=41)[0].astype(np.float32)
    k = np.ones(5, np.float32) / 5
    for axis in (0, 1):
        c = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, c)
    return ((c - c.min()) / (c.max() - c.min()) * 255).astype(np.uint8), margin


@lru_cache(maxsize=1)
def frames():
    """-> uint8 [4, 192, 320] read-only"""
    tex, margin = _texture()
    rng = np.random.default_rng(4242)
    out = np.zeros((N_FRAMES, FRAME_H, FRAME_W), np.uint8)
    for k in range(N_FRAMES):
        oy, ox = margin - STEP[1] * k, margin - STEP[0] * k
        out[k] = tex[oy:oy + FRAME_H, ox:ox + FRAME_W]
        out[k, :, SPLIT:] = (128 + rng.integers(0, NOISE_LEVELS, (FRAME_H, FRAME_W - SPLIT))).astype(np.uint8)
    out.setflags(write=False)
    return out


def flat_frame():
    """no pixel passes the mask's threshold: every block is dropped"""
    return np.full((FRAME_H, FRAME_W), 128, np.uint8)


TWO_BLOCK_GATE = BLOCK * BLOCK                           # a block is kept only when the mask covers it entirely ...


@lru_cache(maxsize=1)
def two_block_frame():
    """... which, with noise on x in [61, 99), y in [61, 83) of a constant frame, holds for blocks (4, 4) and (5, 4) alone"""
    rng = np.random.default_rng(99)
    f = np.full((FRAME_H, FRAME_W), 128, np.uint8)
    f[61:83, 61:99] = rng.integers(0, 256, (22, 38), dtype=np.uint8)
    f.setflags(write=False)
    return f


@lru_cache(maxsize=8)
def frame_vectors(k):
    """the oracle's SAD records and winners of pair (k - 1, k) -> ([240, 4], [240, 3]) read-only"""
    f = frames()
    ent, best = oracle.sad_flow(f[k - 1], f[k], BLOCK, RANGE)
    ent = np.ascontiguousarray(ent, np.float32); best = np.ascontiguousarray(best, np.int32)
    ent.setflags(write=False); best.setflags(write=False)
    return ent, best


@lru_cache(maxsize=8)
def frame_keep(k, min_pixels=GATE):
    keep = keep_flags(frames()[k], BLOCK, min_pixels)
    keep.setflags(write=False)
    return keep


def area_of(det):
    return 0 if det is None else det[0]
