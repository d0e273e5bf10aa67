"""Cases for hip_sad's intra test and scene-cut rule (include/ofps_hip.h N1i: ofps_hip_block_activity[_dev], ofps_hip_sad_intra[_dev],
ofps_hip_sad_flow_intra_dev and the one-pair / fused / batched entry points with the context's ratio set).  CPU only: numpy, the restatement
tests/indep_sad_intra.py and the CPU oracle's search -- never the library under test.  Every derived case carries values that follow from the
definition alone, worked out in its comment; tests/test_sad_intra_cpu.py asserts them of the restatement, tests/test_sad_intra_gpu.py runs the
library against the restatement."""
from functools import lru_cache

import numpy as np

import indep_sad_intra as ii
import sad_median_cases as mc

I32_MIN, I32_MAX, U32_MAX = -(1 << 31), (1 << 31) - 1, (1 << 32) - 1
RATIOS = (1, 8, ii.RATIO_MAX)


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------- activity, derived by hand
# name -> (frame [H, W] u8, block, A per block in raster order)
def _constant():
    """every pixel 77: S = 77 n, m = 77, A = 0; 35 x 29 at block 8: a 4 x 3 lattice with ragged margins"""
    return np.full((29, 35), 77, np.uint8), 8, [0] * 12


def _checkerboard():
    """0 / 255 alternating, block 8: 32 pixels of each, S = 8160, S / n = 127.5 -> m = (8160 + 32) // 64 = 128, A = 32 * 128 + 32 * 127 = 8160"""
    y, x = np.mgrid[0:16, 0:24]
    return (((x + y) & 1) * 255).astype(np.uint8), 8, [32 * 128 + 32 * 127] * 6


def _half(block):
    """n - 1 pixels of 10 and one pixel v with S = 10 n + n / 2, so S / n = 10.5 exactly -> m = 11 (rounded half up), A = (n - 1) + (v - 11).
    A mean rounded down to 10 would give v - 10.  block 4: v = 18, A = 15 + 7 = 22; block 8: v = 42, A = 63 + 31 = 94; block 16: v = 138,
    A = 255 + 127 = 382.  Two blocks side by side, the odd pixel in another place in each"""
    n = block * block
    v = 10 + n // 2
    f = np.full((block, 2 * block), 10, np.uint8)
    f[0, 0] = v
    f[block - 1, 2 * block - 1] = v
    return f, block, [(n - 1) + (v - 11)] * 2


def _largest():
    """block 64, the left half 0 and the right half 255: S = 2048 * 255 = 522240, S / n = 127.5 -> m = 128, A = 2048 * 128 + 2048 * 127 =
    522240: the largest activity there is.  A second block with the halves stacked: the same numbers"""
    f = np.zeros((64, 128), np.uint8)
    f[:, 32:64] = 255
    f[32:, 64:] = 255
    return f, 64, [522240, 522240]


def _block1():
    """block 1: S = p, m = p, A = 0 for every pixel"""
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (7, 9)).astype(np.uint8), 1, [0] * 63


ACTIVITY = {"constant": _constant, "checkerboard": _checkerboard, "half-4": lambda: _half(4), "half-8": lambda: _half(8), "half-16": lambda: _half(16),
            "largest": _largest, "block-1": _block1}

# (W, H, block, stride): ragged margins and unaligned rows; the lattice path's alignments 16 (stride 80, 192), 1 (stride 67) and the
# general path (block 5, 64, 4); 192 x 128: more than one workgroup tile in y, 133 x 70 at block 5: 26 x 14 = 364 blocks = 91 workgroups
SHAPES = ((67, 37, 8, 80), (67, 37, 8, 67), (192, 128, 16, 192), (133, 70, 5, 133), (131, 67, 64, 131), (40, 24, 4, 40),
          (300, 40, 16, 300), (300, 40, 8, 304), (75, 21, 8, 76))


@lru_cache(maxsize=None)
def shape_frame(W, H, stride, seed=0):
    """smooth ramp + noise whose amplitude grows to the right: activities from near 0 to the thousands -> [H, stride] u8 read-only; columns
    >= W hold 255 (a kernel that reads them gets another answer)"""
    rng = np.random.default_rng(300 + seed)
    y, x = np.mgrid[0:H, 0:W]
    f = 40 + (x * 3 + y * 5) % 97 + rng.integers(-1, 2, (H, W)) * (x * 60 // W)
    buf = np.full((H, stride), 255, np.uint8)
    buf[:, :W] = np.clip(f, 0, 255)
    return _ro(buf, np.uint8)


@lru_cache(maxsize=None)
def shape_activity(W, H, block, stride):
    return _ro(ii.activity(shape_frame(W, H, stride)[:, :W], block), np.uint32)


# ---------------------------------------------------------------------------------------------------------------- verdict, derived by hand
# a 4 x 3 lattice (block 8, frame 35 x 29); (SAD, A) per block and what 16 * SAD >= q * A says at q = 1, 8, 255:
#  0  (50, 100)          q 8: 800 >= 800 EQUALITY -> intra; q 1: 800 >= 100 intra; q 255: 800 < 25500 kept
#  1  (49, 100)          q 8: 784 < 800 kept; q 1 intra; q 255 kept
#  2  (0, 0)             0 >= 0: a flat block is intra at every q
#  3  (5, 0)             80 >= 0: intra at every q
#  4  (-1, 0)            -16 < 0: kept at every q (a negative SAD is what the triple holds, not what a search writes)
#  5  (I32_MIN, U32_MAX) -2^35 < q * (2^32 - 1): kept at every q
#  6  (I32_MAX, U32_MAX) 16 * SAD = 2^35 - 16 = 34359738352; q 1: >= 4294967295 intra; q 8: 8 * (2^32 - 1) = 34359738360 > it: kept BY EIGHT
#                        (32-bit arithmetic says anything); q 255 kept
#  7  (1, 16)            q 1: 16 >= 16 equality -> intra; q 8: 16 < 128 kept; q 255 kept
#  8  (1, 17)            q 1: 16 < 17 kept; kept at every q
#  9  (255, 16)          q 255: 4080 >= 4080 equality -> intra; intra at every q
# 10  (254, 16)          q 255: 4064 < 4080 kept; q 8: 4064 >= 128 intra; q 1 intra
# 11  (1000, 2000)       q 8: 16000 >= 16000 equality -> intra; q 1 intra; q 255: 16000 < 510000 kept
FIELD_NBX, FIELD_NBY, FIELD_BLOCK, FIELD_W, FIELD_H = 4, 3, 8, 35, 29
FIELD_SAD_A = ((50, 100), (49, 100), (0, 0), (5, 0), (-1, 0), (I32_MIN, U32_MAX), (I32_MAX, U32_MAX), (1, 16), (1, 17), (255, 16), (254, 16),
               (1000, 2000))
FIELD_KEEP = {1: (0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0),
              8: (0, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0),
              255: (1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1)}
# the gate's flags: an unkept block never comes back, and it is no candidate.  Gated: 0 2 3 5 6 7 8 9 10 (9 blocks); intra among them at
# q 8: 0 2 3 9 10 (5), at q 1: 0 2 3 6 7 9 10 (7), at q 255: 2 3 9 (3)
FIELD_GATE = (1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0)
FIELD_COUNTS = {(1, False): (12, 9), (8, False): (12, 6), (255, False): (12, 3), (1, True): (9, 7), (8, True): (9, 5), (255, True): (9, 3)}
# the cut rule at q 8 without the gate: 6 of 12 (0 2 3 9 10 11).  P = 50: 600 >= 600 EQUALITY a cut; P = 51: 600 < 612 none.  With the gate: 5 of 9: P = 55: 500 >= 495
# a cut, P = 56: 500 < 504 none.  P = 0: never.  A gate of all zeros: n_cand = 0, 0 >= 0: a cut at every P > 0 (and nothing was kept anyway)
FIELD_CUT = {False: (50, 51), True: (55, 56)}


def field(gated=False):
    """-> (best [12, 3] i32: dx, dy nobody reads, activity [12] u32, keep_in u8 [12] or None)"""
    best = np.array([(k - 3, 2 - k, s) for k, (s, _) in enumerate(FIELD_SAD_A)], np.int64).astype(np.int32)
    act = np.array([a for _, a in FIELD_SAD_A], np.uint32)
    return _ro(best, np.int32), _ro(act, np.uint32), _ro(FIELD_GATE, np.uint8) if gated else None


def field_keep(ratio, gated=False):
    k = np.array(FIELD_KEEP[ratio], np.uint8)
    return _ro(k & np.array(FIELD_GATE, np.uint8) if gated else k, np.uint8)


def synthetic(nbx, nby, seed=0):
    """a lattice too large to derive by hand: SADs around a quarter to twice the activity, 12 % exact equalities at q = 8 (A even: SAD = A / 2),
    5 % flat blocks, 15 % unkept -> (best, activity, keep_in) read-only"""
    rng = np.random.default_rng(2000 + seed)
    n = nbx * nby
    act = rng.integers(0, 40000, n) * 2
    sad = (act * rng.uniform(0.2, 2.0, n)).astype(np.int64)
    eq = rng.random(n) < 0.12
    sad[eq] = act[eq] // 2
    flat = rng.random(n) < 0.05
    act[flat] = 0
    sad[flat] = 0
    best = np.stack([rng.integers(-8, 9, n), rng.integers(-8, 9, n), sad], 1)
    return _ro(best, np.int32), _ro(act, np.uint32), _ro(rng.random(n) >= 0.15, np.uint8)


# ---------------------------------------------------------------------------------------------------------------- through the search
# sad_median_cases.scene(): 192 x 128, block 16, range 8, d = (5, -3), five blocks of noise.  The plain search's winners and the raw current
# frame's activities, both restated; tests/test_sad_intra_cpu.py pins what the ratios 4, 8 and 16 keep.
SCENE_RATIOS = (4, 8, 16)
SCENE_KEPT = {4: 72, 8: 73, 16: 86}
SCENE_Q, SCENE_INTRA_AT_Q = 8, 23                          # 23 of 96 blocks are intra at q 8: P = 24: 2300 < 2304 no cut; P = 23: 2300 >= 2208 a cut
SCENE_NO_CUT, SCENE_CUT = 24, 23


@lru_cache(maxsize=1)
def scene_activity():
    return _ro(ii.activity(mc.scene()[1], mc.SCENE_B), np.uint32)


@lru_cache(maxsize=1)
def scene_activity_reverse():
    return _ro(ii.activity(mc.scene()[0], mc.SCENE_B), np.uint32)


def scene_keep(ratio, keep_in=None, cut=0, reverse=False, best=None):
    """best: another search mode's integer winners of the pair (default: the plain search's)"""
    act = scene_activity_reverse() if reverse else scene_activity()
    return ii.keep_flags(mc.scene_vectors(reverse)[1] if best is None else best, act, keep_in, ratio, cut)


@lru_cache(maxsize=1)
def sparse_activity():
    return _ro(ii.activity(mc.sparse_pair()[1], mc.SCENE_B), np.uint32)


# ---------------------------------------------------------------------------------------------------------------- a stream with a cut
# scene prev, scene cur, `half` = cur with its upper five block rows (60 of 96 blocks) overwritten with uniform noise, prev, cur, cur.  The pairs:
# (prev, cur): the planted motion, 23 intra at q 8: no cut at P = 50; (cur, half): the 60 noise blocks are intra, the 36 others match themselves
# at SAD 0: 6000 >= 50 * 96, a cut BY THE RULE -- without it 36 records; (half, prev): prev's upper rows find noise: a cut by the rule as well;
# (prev, cur) again; (cur, cur): SAD 0 against activities in the thousands, every block kept.  tests/test_sad_intra_cpu.py pins the counts
STREAM_Q, STREAM_P = 8, 50
STREAM_KEPT = (None, 73, 0, 0, 73, 96)
STREAM_KEPT_WITHOUT_CUT = {2: 36}


@lru_cache(maxsize=1)
def stream_frames():
    prev, cur = mc.scene()
    half = np.array(cur)
    half[:5 * mc.SCENE_B] = np.random.default_rng(99).integers(0, 256, (5 * mc.SCENE_B, mc.SCENE_W))
    return _ro(np.stack([prev, cur, half, prev, cur, cur]), np.uint8)


@lru_cache(maxsize=None)
def stream_expect(k, ratio=STREAM_Q, cut=STREAM_P):
    """pair (k - 1, k) of the stream through the restated search and the restated verdicts -> (kept records, kept winners, (n_cand, n_intra))"""
    import indep_sad_hier as ih
    f = stream_frames()
    ent, best, _ = ih.search(f[k - 1], f[k], mc.SCENE_B, mc.SCENE_R, 1)
    keep, counts, _ = ii.verdict(best, ii.activity(f[k], mc.SCENE_B), None, ratio, cut)
    return _ro(ent[keep.astype(bool)], np.float32), _ro(best[keep.astype(bool)], np.int32), counts
