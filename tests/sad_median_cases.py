"""Cases for hip_sad's median test (include/ofps_hip.h N1v: ofps_hip_sad_median[_dev], ofps_hip_sad_flow_median_dev and the one-pair / fused
entry points with the context's limit set).  CPU only: numpy, the restatement tests/indep_sad_median.py and the CPU oracle -- never the
library under test.  Every FIELD case carries flags that follow from the definition alone, derived in its comment;
tests/test_sad_median_cpu.py asserts them of the restatement, tests/test_sad_median_gpu.py runs the library against the restatement."""
from functools import lru_cache

import numpy as np

import indep_sad_hier as ih
import indep_sad_median as im
import sad_hier_cases as hc

LIMITS = (1, 2, im.LIMIT_MAX)


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


def _field(nbx, nby, dx, dy, keep_in=None):
    """dx, dy: functions of (bx, by) -> (nbx, nby, best [nblk, 3] i32 with a SAD column nobody reads, keep_in u8 [nblk] or None)"""
    best = np.array([(dx(bx, by), dy(bx, by), 1000 + by * nbx + bx) for by in range(nby) for bx in range(nbx)], np.int32)
    return nbx, nby, _ro(best, np.int32), None if keep_in is None else _ro(keep_in, np.uint8)


# ---- stepped field with planted outliers: lattice 12 x 8, dx = 3 + (by >> 1), dy = -2 + bx // 3: lattice neighbours differ by at most 1 per
# component, so every middle order statistic of a block's neighbours lies within 1 of the block's own component: r2 <= 2, kept at limit 2.
# Six blocks get (+6, 0) or (0, -6); they lie pairwise at Chebyshev distance >= 3, so no 3 x 3 neighbourhood holds two; (0, 0) is a corner
# block, (6, 0) an edge block.  At limit 2 exactly those six are dropped: an outlier's own component is 6 away from values that are at most
# 1 away from its unshifted value, r2 >= 12 - 2 = 10 >= 4; a neighbour of an outlier has n >= 3 neighbours with that one outlier among them,
# which sorts to an end of the list and reaches neither middle order statistic.
STEPPED_OUTLIERS = (((0, 0), (6, 0)), ((6, 0), (0, -6)), ((3, 3), (6, 0)), ((9, 3), (0, -6)), ((2, 6), (6, 0)), ((7, 6), (0, -6)))


def stepped_field():
    nbx, nby, best, _ = _field(12, 8, lambda bx, by: 3 + (by >> 1), lambda bx, by: -2 + bx // 3)
    best = best.copy()
    want = np.ones(nbx * nby, np.uint8)
    for (bx, by), (ox, oy) in STEPPED_OUTLIERS:
        best[by * nbx + bx, 0] += ox
        best[by * nbx + bx, 1] += oy
        want[by * nbx + bx] = 0
    return nbx, nby, _ro(best, np.int32), None, {2: _ro(want, np.uint8)}


# ---- incoming flags are honoured: lattice 12 x 8, keep_in = 0 with vector (0, 0) for bx < 6 or by < 4, elsewhere the constant (9, -7).
# Every kept block's kept neighbours hold its own vector: r2 = 0, kept at limit 1; block (6, 4) has five unkept neighbours ((5, 3), (6, 3),
# (7, 3), (5, 4), (5, 5)) and three kept ones: an implementation that ignores keep_in takes the median 0 of the eight and drops it.  No unkept
# block comes back: the output equals keep_in at every limit.
def masked_field():
    kin = np.array([0 if bx < 6 or by < 4 else 1 for by in range(8) for bx in range(12)], np.uint8)
    nbx, nby, best, kin = _field(12, 8, lambda bx, by: 0 if bx < 6 or by < 4 else 9, lambda bx, by: 0 if bx < 6 or by < 4 else -7, kin)
    return nbx, nby, best, kin, {limit: kin for limit in LIMITS}


# ---- no neighbour: the centre of a 5 x 5 lattice is the one kept block, its vector (-9, 4) among unkept (50, 50): n = 0, r2 = 0, kept at
# every limit; a 1 x 1 lattice has no neighbour at all.
def lone_field():
    kin = np.zeros(25, np.uint8)
    kin[12] = 1
    nbx, nby, best, kin = _field(5, 5, lambda bx, by: -9 if (bx, by) == (2, 2) else 50, lambda bx, by: 4 if (bx, by) == (2, 2) else 50, kin)
    return nbx, nby, best, kin, {limit: kin for limit in LIMITS}


def single_field():
    nbx, nby, best, _ = _field(1, 1, lambda bx, by: 77, lambda bx, by: -77)
    return nbx, nby, best, None, {limit: _ro([1], np.uint8) for limit in LIMITS}


# ---- thin lattices.  5 x 1, dx = 0, 1, 3, 3, 8 (dy = 0): block 0 sees {1}: M = 2, r2 = 2; block 1 sees {0, 3}: M = 3 (the half-pixel
# median 1.5), r2 = |2 - 3| = 1; block 2 sees {1, 3}: M = 4, r2 = 2; block 3 sees {3, 8}: M = 11, r2 = |6 - 11| = 5; block 4 sees {3}: M = 6,
# r2 = 10.  1 x 5: the same numbers in dy down one column.  2 x 2, dx = 0, 2, 5, 9: every block sees the other three (n = 3): M = 2 * 5,
# 2 * 5, 2 * 2, 2 * 2, r2 = 10, 6, 6, 14.
THIN_R2 = (2, 1, 2, 5, 10)
THIN_WANT = {1: (0, 1, 0, 0, 0), 2: (1, 1, 1, 0, 0), im.LIMIT_MAX: (1, 1, 1, 1, 1)}
QUAD_R2 = (10, 6, 6, 14)
QUAD_WANT = {1: (0, 0, 0, 0), 2: (0, 0, 0, 0), 4: (0, 1, 1, 0), im.LIMIT_MAX: (1, 1, 1, 1)}


def thin_field(vertical):
    v = (0, 1, 3, 3, 8)
    f = _field(1, 5, lambda bx, by: 0, lambda bx, by: v[by]) if vertical else _field(5, 1, lambda bx, by: v[bx], lambda bx, by: 0)
    return f[0], f[1], f[2], None, {limit: _ro(w, np.uint8) for limit, w in THIN_WANT.items()}


def quad_field():
    v = (0, 2, 5, 9)
    nbx, nby, best, _ = _field(2, 2, lambda bx, by: v[by * 2 + bx], lambda bx, by: 0)
    return nbx, nby, best, None, {limit: _ro(w, np.uint8) for limit, w in QUAD_WANT.items()}


# ---- even n with a half-pixel median, at the limit's edge: 3 x 1 lattices, the verdict in question is block 1's (n = 2).
# "below": dx = 4, 4, 7: M = 11 (median 5.5), r2 = |8 - 11| = 3 < 4: KEPT at limit 2; a median rounded up to 6 gives 2 px = the limit: dropped.
# "above": dx = 4, 7, 7: M = 11, r2 = |14 - 11| = 3: KEPT at limit 2; a median rounded down to 5 gives 2 px: dropped.
# (Rounding towards the block's own value never changes a verdict; rounding away does, and which way that is depends on the side the block
# lies on: hence one case per side.)  The end blocks see block 1 alone: "below": r2 = 0 and |14 - 8| = 6; "above": 6 and 0.
def half_pixel_field(side):
    v = {"below": (4, 4, 7), "above": (4, 7, 7)}[side]
    nbx, nby, best, _ = _field(3, 1, lambda bx, by: v[bx], lambda bx, by: 0)
    return nbx, nby, best, None, {2: _ro({"below": (1, 1, 0), "above": (0, 1, 1)}[side], np.uint8)}


FIELDS = {"stepped": stepped_field, "masked": masked_field, "lone": lone_field, "single": single_field,
          "thin-5x1": lambda: thin_field(False), "thin-1x5": lambda: thin_field(True), "quad": quad_field,
          "half-pixel-below": lambda: half_pixel_field("below"), "half-pixel-above": lambda: half_pixel_field("above")}
BLOCK = 8                                                # of the frame the field cases' lattices are cut from: W = nbx * 8 + 3, H = nby * 8 + 5


def field_frame(nbx, nby):
    """a ragged margin on both sides: the lattice counts full blocks only"""
    return nbx * BLOCK + 3, nby * BLOCK + 5


def synthetic_field(nbx, nby, seed=0, amplitude=6, big=None):
    """a lattice too large to derive by hand (the restatement is the yardstick): smooth steps plus 7 % random outliers, 15 % unkept blocks;
    big: the outliers hold +-big instead"""
    rng = np.random.default_rng(1000 + seed)
    bx, by = np.meshgrid(np.arange(nbx), np.arange(nby))
    dx = (3 + by // 4 - bx // 7).reshape(-1); dy = (-2 + bx // 5).reshape(-1)
    out = rng.random(nbx * nby) < 0.07
    ox = rng.integers(-amplitude, amplitude + 1, nbx * nby); oy = rng.integers(-amplitude, amplitude + 1, nbx * nby)
    if big is not None:
        ox = np.where(ox < 0, -big, big) - dx; oy = np.where(oy < 0, -big, big) - dy
    best = np.stack([dx + out * ox, dy + out * oy, rng.integers(0, 1 << 16, nbx * nby)], 1)
    return _ro(best, np.int32), _ro(rng.random(nbx * nby) >= 0.15, np.uint8)


# ---- a planted scene through the search: sad_hier_cases.planted_pair(192, 128, d = (5, -3)), block 16, range 8: a 12 x 8 lattice.  Five
# blocks of `cur` are overwritten with independent uniform noise; they lie pairwise at Chebyshev distance >= 3 (every 3 x 3 neighbourhood
# holds at most one), (0, 5) is an edge block.
SCENE_W, SCENE_H, SCENE_B, SCENE_R, SCENE_D = 192, 128, 16, 8, (5, -3)
SCENE_NBX, SCENE_NBY = SCENE_W // SCENE_B, SCENE_H // SCENE_B
SCENE_NBLK = SCENE_NBX * SCENE_NBY
SCENE_NOISE = ((2, 2), (8, 2), (5, 5), (10, 6), (0, 5))
SCENE_LIMIT = 2
SCENE_CAM = (SCENE_W / SCENE_H, 30.0)
SCENE_DETECTOR = dict(min_size=0.05, subdivide=2, target_motion=0.003)
SCENE_RANSAC = dict(num_iters=100, inlier_deg=0.05, num_samples=96)
SCENE_SEED = 11


@lru_cache(maxsize=1)
def scene():
    """-> (prev, cur) read-only"""
    prev, cur = hc.planted_pair(SCENE_W, SCENE_H, SCENE_D)
    cur = cur.copy()
    rng = np.random.default_rng(77)
    for bx, by in SCENE_NOISE:
        cur[by * SCENE_B:(by + 1) * SCENE_B, bx * SCENE_B:(bx + 1) * SCENE_B] = rng.integers(0, 256, (SCENE_B, SCENE_B))
    return hc.planted_pair(SCENE_W, SCENE_H, SCENE_D)[0], _ro(cur, np.uint8)


@lru_cache(maxsize=4)
def scene_vectors(reverse=False):
    """the pair (or the pair exchanged) through the restatements' full search (levels 1: the CPU oracle's plain search)
    -> (records [nblk, 4] f32, integer winners [nblk, 3] i32), read-only"""
    prev, cur = scene()
    if reverse:
        prev, cur = cur, prev
    ent, best, _ = ih.search(prev, cur, SCENE_B, SCENE_R, 1)
    return _ro(ent, np.float32), _ro(best, np.int32)


def scene_keep(limit=SCENE_LIMIT, keep_in=None, reverse=False):
    return im.keep_flags(scene_vectors(reverse)[1], keep_in, SCENE_NBX, SCENE_NBY, limit)


def scene_safe_blocks():
    """the untouched blocks whose whole 3 x 3 neighbourhood is interior: none of its nine blocks lies on the lattice's border, where the
    planted vector would leave the frame -> bool [nblk]"""
    out = np.zeros((SCENE_NBY, SCENE_NBX), bool)
    out[2:SCENE_NBY - 2, 2:SCENE_NBX - 2] = True
    for bx, by in SCENE_NOISE:
        out[by, bx] = False
    return out.reshape(-1)


def filtered(rows, keep):
    """the rows whose flag is set, in raster order"""
    return np.asarray(rows)[np.asarray(keep, bool)]


# ---- fewer than three kept records: two frames of independent uniform noise, 64 x 48, block 16, range 8: twelve winners that have nothing to
# do with each other; at limit 1 the test leaves two of them, blocks 7 and 9 (tests/test_sad_median_cpu.py pins that on the restatement)
SPARSE_W, SPARSE_H, SPARSE_KEPT = 64, 48, 2


@lru_cache(maxsize=1)
def sparse_pair():
    """-> (prev, cur, records [12, 4], integer winners [12, 3]) read-only"""
    rng = np.random.default_rng(7)
    prev, cur = rng.integers(0, 256, (2, SPARSE_H, SPARSE_W)).astype(np.uint8)
    ent, best, _ = ih.search(prev, cur, SCENE_B, SCENE_R, 1)
    return _ro(prev, np.uint8), _ro(cur, np.uint8), _ro(ent, np.float32), _ro(best, np.int32)
