"""-m gpu: the strip SAD kernel on frames whose block rows are clipped by the frame edge.

strip_body skips the dy that the frame clips: interior strips take the straight-line walk, clipped strips walk dy in
chunks and branch past the chunks with no valid dy; the dx = +R pass gives dy = +R to all lanes of a block.  Every
clip state of those branches is hit here on small frames (one full strip plus a ragged one), bit for bit against the
CPU oracle: the (dx, dy, SAD) triples and the f32 records.
"""
import numpy as np
import pytest

import oracle
from ofps_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _planted(W, H, B, R):
    """True motion that points out of the frame: block row 0 of the current frame shows what lies R lines ABOVE the previous
    frame (dy = -R, clipped), the last block row what lies R lines below its place (dy = +R, clipped unless H leaves room)."""
    base = synth.luma_sequence(1, W, H + 2 * R, max_step=0, noise=0, seed=synth.SEED0 + 7 * W + H)[0]
    prev = np.ascontiguousarray(base[R:R + H])
    cur = prev.copy()
    y_last = (H // B - 1) * B
    cur[y_last:y_last + B] = base[y_last + 2 * R:y_last + 2 * R + B]
    cur[0:B] = base[0:B]
    return np.stack([prev, cur])


def _frames(W, H, B, R, kind):
    if kind == "seq":
        return synth.luma_sequence(2, W, H, max_step=R, seed=synth.SEED0 + W + H)
    if kind == "flat":
        return np.full((2, H, W), 77, np.uint8)
    assert kind == "planted"
    return _planted(W, H, B, R)


def _check(ctx, fr, B, R):
    ent_o, best_o = oracle.sad_flow(fr[0], fr[1], B, R)
    ent_g, best_g = ctx.sad_flow(fr[0], fr[1], B, R, want_best=True)
    assert best_g.shape == best_o.shape
    np.testing.assert_array_equal(best_g, best_o)
    np.testing.assert_array_equal(ent_g.view(np.uint32), ent_o.view(np.uint32))


KINDS = ("seq", "flat", "planted")

# <16,16>, W = 144: a full strip of 8 blocks and a ragged one of 1
#   16: one block row, only dy = 0          24: one row, dy 0..8            40: two rows, both clipped on both sides
#   48: bottom row with hi = R exactly      56: three rows, bottom hi = R+8  88: an interior row between the clipped ones
H_16_16 = (16, 24, 40, 48, 56, 88)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", H_16_16)
def test_clip_states_16_16(ctx, H, kind):
    _check(ctx, _frames(144, H, 16, 16, kind), 16, 16)


# <8,32>, W = 72 (strips of 4 blocks).  40: every row clipped on both sides.  76: exactly one interior row (y0 = 32); tops clipped
# at 32/24/16/8, bottoms at 4/12/20/28 -- not on chunk edges
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", (40, 76))
def test_clip_states_8_32(ctx, H, kind):
    _check(ctx, _frames(72, H, 8, 32, kind), 8, 32)


# the other table entries and a range whose lanes per block exceed its dx groups (+-24): a clipped and an interior row each,
# one full strip plus a ragged one
OTHER = [
    # (W, H, B, R)
    (272, 56, 16, 8),      # 16 blocks per strip; row 0 clipped, rows 1-2 interior
    (72, 52, 8, 16),       # 8 per strip; rows 0-1 and 4-5 clipped, rows 2-3 interior
    (80, 104, 16, 32),     # 4 per strip; rows 2-3 interior
    (80, 88, 16, 24),      # 4 per strip, 12 dx groups on 16 lanes; rows 2-3 interior
    (136, 36, 8, 8),       # 16 per strip; row 0 and row 3 clipped
]


@pytest.mark.parametrize("kind", ("seq", "flat"))
@pytest.mark.parametrize("W,H,B,R", OTHER)
def test_clip_other_geometries(ctx, W, H, B, R, kind):
    _check(ctx, _frames(W, H, B, R, kind), B, R)


def test_clip_batched_dev(ctx):
    """3 pairs of 144x56 in one launch of the device form: pair k is frames (k, k+1)."""
    W, H, B, R, n = 144, 56, 16, 16, 4
    fr = synth.luma_sequence(n, W, H, max_step=R, seed=synth.SEED0 + 56)
    nblk = (W // B) * (H // B)
    d_fr, d_ent, d_best = ctx.malloc(fr.nbytes), ctx.malloc((n - 1) * nblk * 16), ctx.malloc((n - 1) * nblk * 12)
    try:
        ctx.memcpy_h2d(d_fr, fr)
        ctx.sad_flow_dev(d_fr, n, W, H, W, W * H, 0, B, R, d_ent, d_best)
        ent = np.zeros((n - 1, nblk, 4), np.float32); best = np.zeros((n - 1, nblk, 3), np.int32)
        ctx.memcpy_d2h(ent, d_ent)
        ctx.memcpy_d2h(best, d_best)
    finally:
        for p in (d_fr, d_ent, d_best):
            ctx.free(p)
    for k in range(n - 1):
        ent_o, best_o = oracle.sad_flow(fr[k], fr[k + 1], B, R)
        np.testing.assert_array_equal(best[k], best_o)
        np.testing.assert_array_equal(ent[k].view(np.uint32), ent_o.view(np.uint32))


def test_clip_pruned_matches_exhaustive(ctx):
    """The pruned mode hands its overflow strips to the same strip_body through a strip list."""
    fr = synth.luma_sequence(2, 256, 144, max_step=16, seed=synth.SEED0 + 256 + 144)
    ent_x, best_x = ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True)
    ctx.set_sad_mode(ctx.SAD_PRUNED)
    try:
        ent_p, best_p = ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True)
    finally:
        ctx.set_sad_mode(ctx.SAD_EXHAUSTIVE)
    np.testing.assert_array_equal(best_p, best_x)
    np.testing.assert_array_equal(ent_p.view(np.uint32), ent_x.view(np.uint32))
    ent_o, best_o = oracle.sad_flow(fr[0], fr[1], 16, 16)
    np.testing.assert_array_equal(best_x, best_o)
    np.testing.assert_array_equal(ent_x.view(np.uint32), ent_o.view(np.uint32))
