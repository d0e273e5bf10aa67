"""CPU: the cases of tests/sad_median_cases.py hold of the restatement tests/indep_sad_median.py alone -- the flags each case derives from
the definition (include/ofps_hip.h N1v) are the restatement's, and the planted scene separates test-on from test-off.  No library call.

The planted scene, measured here (restatement behind the CPU oracle's full search, limit 2): the five overwritten blocks return the winners
(8, -8), (-3, 8), (-6, -3), (6, 4), (1, 5) instead of the planted (5, -3); all five lie 2 px or more from their neighbours' median and are
dropped -- none happened to return a winner within the limit.  72 of the 96 blocks are kept: beyond the five the test drops blocks of the
top row and the right column, where the planted vector leaves the frame.  At limit 1: 68 kept; at limit 255: all 96."""
import numpy as np
import pytest

import indep_sad_median as im
import sad_median_cases as mc


@pytest.mark.parametrize("name", list(mc.FIELDS))
def test_derived_flags_hold_of_the_restatement(name):
    nbx, nby, best, kin, want = mc.FIELDS[name]()
    assert best.shape == (nbx * nby, 3) and want
    for limit, flags in want.items():
        np.testing.assert_array_equal(im.keep_flags(best, kin, nbx, nby, limit), flags, err_msg=f"{name} at limit {limit}")
    for limit in mc.LIMITS:                              # no unkept block ever comes back
        out = im.keep_flags(best, kin, nbx, nby, limit)
        if kin is not None:
            np.testing.assert_array_equal(out & kin, out)


def test_stepped_field_is_what_its_comment_says():
    nbx, nby, best, _, want = mc.stepped_field()
    pos = [p for p, _ in mc.STEPPED_OUTLIERS]
    assert len(pos) == 6 and (0, 0) in pos and any(by == 0 and 0 < bx < nbx - 1 for bx, by in pos)
    for i, a in enumerate(pos):
        for b in pos[i + 1:]:
            assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3
    r2 = im.residual2(best, None, nbx, nby)
    out = ~want[2].astype(bool)
    assert int(out.sum()) == 6 and (r2[out] >= 10).all() and (r2[~out] <= 2).all()
    clean = mc._field(nbx, nby, lambda bx, by: 3 + (by >> 1), lambda bx, by: -2 + bx // 3)[2]
    assert (im.residual2(clean, None, nbx, nby) <= 2).all()


def test_ignoring_the_incoming_flags_would_drop_block_6_4():
    nbx, nby, best, kin, want = mc.masked_field()
    k = 4 * nbx + 6
    nb = im.neighbours(6, 4, nbx, nby)
    assert len(nb) == 8 and sum(int(kin[y * nbx + x]) for x, y in nb) == 3
    assert want[1][k] == 1 and im.keep_flags(best, None, nbx, nby, 1)[k] == 0


def test_thin_lattice_residuals():
    for vertical in (False, True):
        nbx, nby, best, _, _ = mc.thin_field(vertical)
        np.testing.assert_array_equal(im.residual2(best, None, nbx, nby), mc.THIN_R2)
    nbx, nby, best, _, _ = mc.quad_field()
    np.testing.assert_array_equal(im.residual2(best, None, nbx, nby), mc.QUAD_R2)


@pytest.mark.parametrize("side", ["below", "above"])
def test_a_rounded_median_flips_block_1_at_limit_2(side):
    nbx, nby, best, _, want = mc.half_pixel_field(side)
    r2 = im.residual2(best, None, nbx, nby)
    assert r2[1] == 3 and want[2][1] == 1                # 1.5 px: inside limit 2
    lo, hi = sorted((int(best[0, 0]), int(best[2, 0])))
    assert (lo + hi) % 2 == 1
    away = hi // 2 + lo // 2 + 1 if side == "below" else (lo + hi) // 2          # 6 | 5: the median rounded away from block 1's value
    assert abs(int(best[1, 0]) - away) == 2              # ... is the limit itself: dropped


def test_doubled_median_and_saturation():
    assert im.doubled_median([5]) == 10 and im.doubled_median([1, 2]) == 3 and im.doubled_median([9, 1, 4]) == 8
    assert im.doubled_median([4, 1, 3, 2]) == 5 and im.doubled_median(range(8)) == 7
    best = np.array([[2 ** 31 - 1, 0, 0], [-2 ** 31, 0, 0]], np.int64)
    np.testing.assert_array_equal(im.residual2(best, None, 2, 1), [im.R2_MAX, im.R2_MAX])


def test_planted_scene_separates_on_from_off():
    prev, cur = mc.scene()
    assert prev.shape == cur.shape == (mc.SCENE_H, mc.SCENE_W)
    pos = mc.SCENE_NOISE
    for i, a in enumerate(pos):
        for b in pos[i + 1:]:
            assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3
    _, best = mc.scene_vectors()
    keep = mc.scene_keep()
    safe = mc.scene_safe_blocks()
    assert int(safe.sum()) == (mc.SCENE_NBX - 4) * (mc.SCENE_NBY - 4) - 3        # three of the five overwritten blocks lie in that interior
    assert (best[safe, :2] == mc.SCENE_D).all()
    assert keep[safe].all(), "an untouched block with an interior 3 x 3 neighbourhood was dropped"
    noise = [by * mc.SCENE_NBX + bx for bx, by in pos]
    dropped = [k for k in noise if not keep[k]]
    print(f"overwritten blocks: winners {[tuple(int(v) for v in best[k, :2]) for k in noise]}, dropped at limit {mc.SCENE_LIMIT}: {len(dropped)} of {len(noise)}; "
          f"kept in all: {int(keep.sum())} of {mc.SCENE_NBLK}")
    assert 0 < int(keep.sum()) < mc.SCENE_NBLK           # the GPU tests can tell test-on from test-off
    # the reversed pair (the fused stream's second ticket) is a case of its own
    assert 0 < int(mc.scene_keep(reverse=True).sum()) < mc.SCENE_NBLK


def test_sparse_pair_leaves_fewer_than_three():
    _, _, ent, best = mc.sparse_pair()
    keep = im.keep_flags(best, None, mc.SPARSE_W // mc.SCENE_B, mc.SPARSE_H // mc.SCENE_B, 1)
    assert len(best) == 12 and int(keep.sum()) == mc.SPARSE_KEPT < 3 and list(np.flatnonzero(keep)) == [7, 9]
