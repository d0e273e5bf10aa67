"""Cases for gate, consistency check and median test in the batched forms (include/ofps_hip.h N1b: ofps_hip_sad_flow_filtered_dev,
ofps_hip_set_sad_batch_filter and the batched stream forms behind it).  CPU only: numpy, the CPU oracle and the three criteria's own
restatements (tests/sad_gate_cases.py, tests/sad_consistency_cases.py, tests/indep_sad_median.py) -- never the library under test.

The expected kept set of an item: the gate's flags AND the check's flags, then the median restatement on the integer winners with those as
keep_in.  tests/test_sad_batch_filter_cpu.py pins that these inputs tell the feature from its absence and from its likely bugs;
tests/test_sad_batch_filter_gpu.py runs them."""
from functools import lru_cache

import numpy as np

import indep_sad_median as im
import oracle
import sad_consistency_cases as cc
import sad_gate_cases as gc

GATE, LIMIT, MEDIAN = gc.GATE, cc.LIMIT, 2               # the planted cases' values: gate 1, an exact round trip, the README's median limit
# each criterion alone, every pair of them, all three
CRITERIA = tuple((g, c, m) for g in (0, GATE) for c in (0, LIMIT) for m in (0, MEDIAN) if g or c or m)


def criteria_id(crit):
    return "-".join(n + str(v) for n, v in zip(("gate", "check", "median"), crit) if v) or "off"


_vectors = {}


def vectors(prev, cur, block, rng):
    """the oracle's records and integer winners of the pair -> ([nblk, 4] f32, [nblk, 3] i32) read-only, cached by content"""
    key = (prev.shape, hash(prev.tobytes()), hash(cur.tobytes()), block, rng)
    if key not in _vectors:
        ent, best = oracle.sad_flow(prev, cur, block, rng)
        ent = np.ascontiguousarray(ent, np.float32); best = np.ascontiguousarray(best, np.int32)
        ent.setflags(write=False); best.setflags(write=False)
        _vectors[key] = (ent, best)
    return _vectors[key]


def keep_of(prev, cur, block, rng, gate, limit, median, F=None, G=None):
    """-> bool [nblk]: what the pair (prev, cur) keeps.  F, G: the integer winners of the forward and the backward search when they are not
    the plain search's (the caller's own, in a search mode the oracle does not restate)"""
    H, W = cur.shape
    nbx, nby = W // block, H // block
    if F is None:
        F = vectors(prev, cur, block, rng)[1]
    keep = np.ones(nbx * nby, bool)
    if gate:
        keep &= gc.keep_flags(cur, block, gate)
    if limit:
        if G is None:
            G = vectors(cur, prev, block, rng)[1]
        keep &= cc.keep_flags(F, G, W, H, block, limit)
    if median:
        keep = im.keep_flags(F, keep.astype(np.uint8) if (gate or limit) else None, nbx, nby, median) != 0
    return keep


def pairs_of(frames, ref_mode):
    """(prev, cur) per pair as ofps_hip_sad_flow_dev forms them: ref_mode 0 (k, k + 1), ref_mode 1 (0, k + 1)"""
    return [(frames[0] if ref_mode else frames[k], frames[k + 1]) for k in range(len(frames) - 1)]


# ---- the mixed batch: a gate that keeps only blocks the mask covers entirely -> items with some, none, two and all blocks kept
def noise_frame():
    return gc.content("noise", gc.FRAME_W, gc.FRAME_H, seed=3)


@lru_cache(maxsize=1)
def mixed_frames():
    """-> uint8 [5, 192, 320]: [textured, flat, two-block, textured, noise]; at gate gc.TWO_BLOCK_GATE the four pairs' current frames keep
    0, 2, some and all of the 240 blocks"""
    f = np.stack([gc.frames()[0], gc.flat_frame(), gc.two_block_frame(), gc.frames()[0], noise_frame()])
    f.setflags(write=False)
    return f


MIXED_KEPT_2 = 2

# ---- the compaction's geometry: 41 x 33 = 1,353 blocks of 8 px: two scan rounds of 1,024, the second partial and no multiple of 64
SCAN_W, SCAN_H, SCAN_B, SCAN_R, SCAN_FRAMES = 328, 264, 8, 4, 4
SCAN_NBLK = (SCAN_W // SCAN_B) * (SCAN_H // SCAN_B)
# ... and 63 x 49 = 3,087 blocks: four scan rounds, the last partial, 3,087 = 48 * 64 + 15
SCAN3_W, SCAN3_H = 504, 392
SCAN3_NBLK = (SCAN3_W // SCAN_B) * (SCAN3_H // SCAN_B)


def _moving(n, W, H, seed, step=(2, 1), split=None):
    """n frames of smooth texture moving by `step` per frame; right of a split that moves by two blocks of 8 per frame constant 128 + {0, 1}
    noise, fresh per frame: every pair keeps another number of blocks under every criterion"""
    from ofps_amd import synth
    margin = 16
    c = synth.random_luma(1, W + 2 * margin, H + 2 * margin, seed=seed)[0].astype(np.float32)
    k = np.ones(5, np.float32) / 5
    for axis in (0, 1):
        c = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, c)
    tex = ((c - c.min()) / (c.max() - c.min()) * 255).astype(np.uint8)
    rng = np.random.default_rng(seed)
    out = np.zeros((n, H, W), np.uint8)
    for j in range(n):
        oy, ox = margin - step[1] * j, margin - step[0] * j
        out[j] = tex[oy:oy + H, ox:ox + W]
        if split is not None:
            at = split + 16 * j
            out[j, :, at:] = (128 + rng.integers(0, 2, (H, W - at))).astype(np.uint8)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=1)
def scan_frames():
    return _moving(SCAN_FRAMES, SCAN_W, SCAN_H, seed=61, split=200)


@lru_cache(maxsize=1)
def scan3_frames():
    return _moving(3, SCAN3_W, SCAN3_H, seed=62, split=300)


# ---- more than 8,192 blocks: 728 x 728 at block 8 = 91 x 91 = 8,281, range 4: the estimator's launch-per-step solver with per-item counts
BIG_W = BIG_H = 728
BIG_B, BIG_R, BIG_FRAMES = 8, 4, 4
BIG_NBLK = (BIG_W // BIG_B) * (BIG_H // BIG_B)
BIG_CAM = (1.0, 30.0)


@lru_cache(maxsize=1)
def big_frames():
    return _moving(BIG_FRAMES, BIG_W, BIG_H, seed=63, split=480)
