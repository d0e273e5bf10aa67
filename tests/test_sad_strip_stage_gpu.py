"""-m gpu: the strip SAD kernel's window staging, on the smallest frames at which it can go wrong.

Where a window row is exactly its 16-byte granules (16x16 +-16 / +-32, 8x8 +-16 / +-32) strip_body stages the search window with
direct global -> LDS loads: the LDS address of a granule is wave-uniform base + 16 x lane, frame clipping is the lane's exec bit,
and one wait stands before the walk.  Every other instantiation stages through registers.  A granule that lands in the wrong
cell, a cell that should stay unwritten and is not, a lane left on outside the frame or a walk that starts before the window has
landed changes a winner, so everything is compared bit for bit with the CPU oracle: (dx, dy, SAD) triples and f32 records.

Widths (16x16 +-16, strips of 8 blocks): 128 = one strip whose window leaves the frame on both sides; 144 = a full strip and a
ragged one of one block; 136 = the last granule straddles W; 272 = an interior strip between two edge strips.  Heights: 48 = every
block row clipped; 80 = interior rows between a clipped top and bottom (both forms of the walk after the same staging).
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _noise(n, W, H, R, seed):
    """Seeded noise; frame k+1 is frame k moved by a vector inside the range (edges wrap), with a little new noise on top."""
    rng = np.random.default_rng(seed)
    fr = [rng.integers(0, 256, (H, W), dtype=np.uint8)]
    for _ in range(n - 1):
        dx, dy = (int(v) for v in rng.integers(-R, R + 1, 2))
        nxt = np.roll(fr[-1], (dy, dx), axis=(0, 1)).astype(np.int16) + rng.integers(-2, 3, (H, W))
        fr.append(np.clip(nxt, 0, 255).astype(np.uint8))
    return np.stack(fr)


def _flat(n, W, H):
    return np.full((n, H, W), 77, np.uint8)


_ORACLE = {}


def _expected(fr, k_prev, k_cur, B, R, key):
    """oracle.sad_flow of one pair, computed once per (content, pair, geometry)."""
    key = key + (k_prev, k_cur, B, R)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.sad_flow(fr[k_prev], fr[k_cur], B, R)
    return _ORACLE[key]


def _run_dev(ctx, fr, B, R, stride=None, pad=0, ref_mode=0):
    """The device form on frames of row pitch `stride` >= W whose padding bytes hold `pad` -> (records, triples) per pair."""
    n, H, W = fr.shape
    stride = stride or (W + 15) // 16 * 16
    buf = np.full((n, H, stride), pad, np.uint8)
    buf[:, :, :W] = fr
    nblk = (W // B) * (H // B)
    d_fr, d_ent, d_best = ctx.malloc(buf.nbytes), ctx.malloc((n - 1) * nblk * 16), ctx.malloc((n - 1) * nblk * 12)
    try:
        ctx.memcpy_h2d(d_fr, buf)
        ctx.sad_flow_dev(d_fr, n, W, H, stride, stride * H, ref_mode, B, R, d_ent, d_best)
        ent = np.zeros((n - 1, nblk, 4), np.float32)
        best = np.zeros((n - 1, nblk, 3), np.int32)
        ctx.memcpy_d2h(ent, d_ent)
        ctx.memcpy_d2h(best, d_best)
    finally:
        for p in (d_fr, d_ent, d_best):
            ctx.free(p)
    return ent, best


def _check_dev(ctx, fr, B, R, key, stride=None, pad=0, ref_mode=0):
    ent, best = _run_dev(ctx, fr, B, R, stride, pad, ref_mode)
    for k in range(len(fr) - 1):
        ent_o, best_o = _expected(fr, 0 if ref_mode else k, k + 1, B, R, key)
        np.testing.assert_array_equal(best[k], best_o)
        np.testing.assert_array_equal(ent[k].view(np.uint32), ent_o.view(np.uint32))


def _check_host(ctx, fr, B, R, key):
    ent_o, best_o = _expected(fr, 0, 1, B, R, key)
    ent_g, best_g = ctx.sad_flow(fr[0], fr[1], B, R, want_best=True)
    np.testing.assert_array_equal(best_g, best_o)
    np.testing.assert_array_equal(ent_g.view(np.uint32), ent_o.view(np.uint32))


# (W, H) at 16x16 +-16: the table of the module docstring
GEOM_16_16 = [(128, 80), (144, 80), (136, 80), (272, 80), (144, 48)]


@pytest.mark.parametrize("W,H", GEOM_16_16)
def test_stage_16_16_noise_then_flat(ctx, W, H):
    """Noise with a shifted copy, then -- same process, same workgroup slots -- a flat pair where every candidate ties: a cell
    the staging leaves unwritten still holds the noise frame's bytes there, and a wrong tie order or a leaked cell moves the
    winner away from the spec's first candidate."""
    fr = _noise(2, W, H, 16, 1000 + W + H)
    _check_host(ctx, fr, 16, 16, ("noise", W, H))
    _check_dev(ctx, fr, 16, 16, ("noise", W, H))
    _check_host(ctx, _flat(2, W, H), 16, 16, ("flat", W, H))
    _check_dev(ctx, _flat(2, W, H), 16, 16, ("flat", W, H))


@pytest.mark.parametrize("pad", (255, 0))
@pytest.mark.parametrize("W,H", [(136, 80), (144, 48), (272, 80)])
def test_stage_16_16_padded_stride(ctx, W, H, pad):
    """Row pitch beyond W (one and a half granules more than the next multiple of 16 would need), padding all ones / all zero: the
    granule that straddles W brings padding into LDS, and a masked column that leaks wins (0) or loses (255) against the noise."""
    stride = (W + 15) // 16 * 16 + 32
    fr = _noise(2, W, H, 16, 1000 + W + H)
    _check_dev(ctx, fr, 16, 16, ("noise", W, H), stride=stride, pad=pad)
    _check_dev(ctx, _flat(2, W, H), 16, 16, ("flat", W, H), stride=stride, pad=pad)


# the shared strip_body in the other instantiations: 8x8 +-32 stages directly (4 blocks per strip, 6 granules per row, 10 rows per
# step of which the last step's run past the window); 8x8 +-8, 16x16 +-24 and 16x16 +-8 must stay on register staging (8-byte granules)
OTHER = [
    # (W, H, B, R)
    (72, 88, 8, 32),       # two full strips and a ragged one; rows 4-6 interior
    (136, 36, 8, 8),       # 16 per strip; row 0 and row 3 clipped
    (80, 88, 16, 24),      # 4 per strip, 12 dx groups on 16 lanes; rows 2-3 interior
    (272, 56, 16, 8),      # 16 per strip; row 0 clipped, rows 1-2 interior
]


@pytest.mark.parametrize("W,H,B,R", OTHER)
def test_stage_other_instantiations(ctx, W, H, B, R):
    fr = _noise(2, W, H, R, 2000 + W + H + B + R)
    _check_host(ctx, fr, B, R, ("noise", W, H))
    _check_dev(ctx, fr, B, R, ("noise", W, H), stride=(W + 15) // 16 * 16 + 16, pad=255)
    _check_host(ctx, _flat(2, W, H), B, R, ("flat", W, H))


@pytest.mark.parametrize("ref_mode", (0, 1))
def test_stage_three_pairs_dev(ctx, ref_mode):
    """Three pairs in one launch: pair k is frames (k, k+1), or (0, k+1) with a shared key frame."""
    fr = _noise(4, 144, 80, 16, 3000)
    _check_dev(ctx, fr, 16, 16, ("noise4", 144, 80), ref_mode=ref_mode)


def test_stage_pruned_overflow_runs_the_strip_body(ctx):
    """Noise gives the pruned mode nothing to prune: its strips overflow and go to sad_strip_list_kernel, which walks them with
    the same strip_body -- one strip after the other in a wave, so a window is staged into LDS that the previous strip has read."""
    W, H = 272, 80
    fr = _noise(2, W, H, 16, 1000 + W + H)
    ent_o, best_o = _expected(fr, 0, 1, 16, 16, ("noise", W, H))
    ctx.set_sad_mode(ctx.SAD_PRUNED)
    try:
        ent_p, best_p = ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True)
        overflow = ctx.sad_pruned_overflow_strips()
    finally:
        ctx.set_sad_mode(ctx.SAD_EXHAUSTIVE)
    assert overflow > 0, "the frame was meant to overflow the pruned kernel's survivor lists"
    np.testing.assert_array_equal(best_p, best_o)
    np.testing.assert_array_equal(ent_p.view(np.uint32), ent_o.view(np.uint32))
