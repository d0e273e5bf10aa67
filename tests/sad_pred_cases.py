"""Cases for the neighbour and zero predictors of hip_sad's search levels (include/ofps_hip.h N1p).  CPU only: numpy, the restatements
tests/indep_sad_pred.py / tests/indep_sad_hier.py and the CPU oracle -- never the library under test.  tests/test_sad_pred_cpu.py pins that
the cases hold of the restatement alone; tests/test_sad_pred_gpu.py runs them."""
from functools import lru_cache

import numpy as np

import indep_sad_pred as ip
import sad_hier_cases as hc

# ---- two motions: the frame's columns left of `boundary` move by d_left, the others by d_right, and the boundary lies in the middle of a
# parent block's column, so the parent that straddles it holds one vector for children on both sides.
# (W, H, block, range, levels, boundary x, d_left, d_right, blocks under the rule, lattice blocks, blocks under the rule that mode 0 misses)
# The rule: a block wholly on one side of the boundary for which sad_hier_cases.reachable(W, H, B, L, d_side) holds returns d_side.  The last
# three columns are the restatement's own counts (tests/test_sad_pred_cpu.py asserts them).
TWO_MOTIONS = ((192, 128, 16, 8, 2, 80, (10, -6), (-9, 7), 72, 96, 4),
               (192, 128, 16, 8, 2, 112, (3, 2), (-5, -4), 72, 96, 4),
               (200, 136, 8, 8, 2, 104, (12, 5), (-11, -8), 362, 425, 22),
               (320, 192, 16, 8, 3, 144, (21, -14), (-19, 12), 160, 240, 4))


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=8)
def two_motion_pair(W, H, boundary, d_left, d_right, seed=2024):
    """prev = the canvas cut at the margin; cur = the cut at d_left left of the boundary column joined to the cut at d_right from it on,
    + uniform noise in {-1, 0, 1} -> (prev, cur) read-only"""
    c = hc.canvas(W, H, seed)
    M = hc.MARGIN
    prev = c[M:M + H, M:M + W]
    cur = np.empty((H, W), np.int64)
    for (dx, dy), cols in ((d_left, slice(0, boundary)), (d_right, slice(boundary, W))):
        cur[:, cols] = c[M + dy:M + dy + H, M + dx:M + dx + W][:, cols]
    cur = cur + np.random.default_rng(seed + 7 * boundary + W).integers(-1, 2, cur.shape)
    assert cur.min() >= 0 and cur.max() <= 255
    return _ro(prev, np.uint8), _ro(cur, np.uint8)


def rule(W, H, B, levels, boundary, d_left, d_right):
    """-> (under [nblk] bool, want [nblk, 2]: the planted vector of the block's side; rows of blocks across the boundary are zero)"""
    nbx, nby = W // B, H // B
    x0 = np.tile(np.arange(nbx) * B, nby)
    left, right = x0 + B <= boundary, x0 >= boundary
    under = (left & hc.reachable(W, H, B, levels, d_left)) | (right & hc.reachable(W, H, B, levels, d_right))
    want = np.zeros((nbx * nby, 2), np.int64)
    want[left] = d_left
    want[right] = d_right
    return under, want


def inside(W, H, B, want, boundary):
    """-> [nblk] bool: wholly on one side, and the block displaced by its side's vector lies inside the frame"""
    nbx, nby = W // B, H // B
    x0 = np.tile(np.arange(nbx) * B, nby); y0 = np.repeat(np.arange(nby) * B, nbx)
    one_side = (x0 + B <= boundary) | (x0 >= boundary)
    return one_side & (x0 + want[:, 0] >= 0) & (x0 + want[:, 0] <= W - B) & (y0 + want[:, 1] >= 0) & (y0 + want[:, 1] <= H - B)


@lru_cache(maxsize=16)
def two_motion_expect(i, mode):
    """scene i through the restatement in `mode` -> (prev, cur, entries, best, level-0 keys), arrays read-only"""
    W, H, B, R, L, bnd, dl, dr = TWO_MOTIONS[i][:8]
    prev, cur = two_motion_pair(W, H, bnd, dl, dr)
    ent, best, _, keys = ip.search(prev, cur, B, R, L, mode)
    return prev, cur, _ro(ent, np.float32), _ro(best, np.int32), tuple(keys)


def misses(best, under, want):
    return under & ((best[:, 0] != want[:, 0]) | (best[:, 1] != want[:, 1]))
