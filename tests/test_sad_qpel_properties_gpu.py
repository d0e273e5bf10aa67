"""-m gpu property sweep of hip_sad over its whole accepted domain (tests/sad_qpel_cases.py: blocks 1..64, ranges 0..64, frames
from 1x1 to 150x100, noise / binary / coarse / flat / sub-pel content, the same derandomised examples and explicit corners the
CPU sweep in tests/test_sad_qpel_cpu.py walks): at motion scale 4 against tests/indep_sad_qpel.py on the oracle's integer
winners -- both refine() and the key-free refine_by_tuples() --, at scale 1 against oracle.sad_flow.  (Dx, Dy, SAD) as integers,
records as uint32 bit patterns; an empty block grid gives zero records and no error at either scale.  ofps_hip_sad_flow repacks
every frame to a 64-byte row stride, so the sweeps reach the strip kernels (block 8 / 16, ranges 8 .. 32 of the strip table) and
the generic kernel (everything else), never the per-block kernel.  The table behind them goes through ofps_hip_sad_flow_dev with
rows that are only 4-byte aligned and with OFPS_HIP_SAD_KERNEL=block: its 16/32 and 8/32 rows take the per-block kernel
(launch_qsad) at the largest range it has, followed by the templated refinement; its other rows have no per-block kernel and
take the generic kernel on a row stride the sweeps never use."""
import numpy as np
import pytest

import oracle

import indep_sad_qpel as iq
import sad_qpel_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _same(ent_g, best_g, ent_e, best_e):
    np.testing.assert_array_equal(best_g, best_e)                                  # (Dx, Dy, SAD): integers
    np.testing.assert_array_equal(ent_g.view(np.uint32), ent_e.view(np.uint32))    # records: the same bits


def test_scale_four_sweep_matches_the_restatement_and_the_tuple_minimum(ctx):
    ctx.set_sad_motion_scale(4)
    obs = []

    @cases.sweep
    def run(case):
        w, h, b, r, _, _ = case
        fr = cases.frames(*case)
        _, best_i = oracle.sad_flow(fr[0], fr[1], b, r)
        ent_e, best_e = iq.refine(fr[0], fr[1], b, r, best_i)
        ent_t, best_t, n_valid = iq.refine_by_tuples(fr[0], fr[1], b, r, best_i)
        obs.append(cases.observe(case, best_e, n_valid))
        ent_g, best_g = ctx.sad_flow(fr[0], fr[1], b, r, want_best=True)
        assert len(ent_g) == len(best_g) == (w // b) * (h // b)
        _same(ent_g, best_g, ent_e, best_e)
        _same(ent_g, best_g, ent_t, best_t)                                        # nothing of the packed key on this side

    run()
    cases.coverage(obs)                                                            # the same conditions the CPU sweep asserts


def test_scale_one_sweep_matches_the_oracle(ctx):
    assert ctx.get_sad_motion_scale() == 1
    seen = []

    @cases.sweep
    def run(case):
        w, h, b, r, _, _ = case
        fr = cases.frames(*case)
        ent_o, best_o = oracle.sad_flow(fr[0], fr[1], b, r)
        ent_g, best_g = ctx.sad_flow(fr[0], fr[1], b, r, want_best=True)
        assert len(ent_g) == len(best_g) == (w // b) * (h // b)
        _same(ent_g, best_g, ent_o, best_o)
        seen.append((b, r, len(best_o)))

    run()
    assert sum(1 for b, _, n in seen if n and b > 32) >= 5 and sum(1 for _, r, n in seen if n and r > 32) >= 5


def _dev_pairs(ctx, fr, stride, B, R):
    """ofps_hip_sad_flow_dev, ref_mode 0, on frames laid out with the given row stride -> (entries, best) per pair"""
    n, H, W = fr.shape
    buf = np.full((n, H, stride), 0xA5, np.uint8); buf[:, :, :W] = fr             # the padding holds junk
    nblk = (W // B) * (H // B)
    d_fr, d_ent, d_best = ctx.malloc(buf.nbytes), ctx.malloc((n - 1) * nblk * 16), ctx.malloc((n - 1) * nblk * 12)
    try:
        ctx.memcpy_h2d(d_fr, buf)
        ctx.sad_flow_dev(d_fr, n, W, H, stride, stride * H, 0, B, R, d_ent, d_best)
        ent = np.zeros((n - 1, nblk, 4), np.float32); best = np.zeros((n - 1, nblk, 3), np.int32)
        ctx.memcpy_d2h(ent, d_ent); ctx.memcpy_d2h(best, d_best)
    finally:
        for p in (d_fr, d_ent, d_best):
            ctx.free(p)
    return ent, best


@pytest.mark.parametrize("path", ["rows_4_byte_aligned", "option_sad_kernel_block"])
@pytest.mark.parametrize("scale", [4, 1])
@pytest.mark.parametrize("W,H,B,R", [(100, 70, 16, 32), (150, 100, 8, 32),                                  # per-block kernel
                                     (100, 70, 16, 48), (64, 64, 64, 64), (40, 24, 4, 8), (150, 100, 8, 64)])   # generic kernel
def test_sad_flow_dev_on_unaligned_rows_and_with_the_strip_kernels_switched_off(ctx, W, H, B, R, scale, path):
    """sad_pairs_device has a per-block kernel for block 16 / 8 at ranges 8, 16 and 32 only; both `path`s keep the strip kernel
    from running, so the first two rows run launch_qsad<16, 32> and <8, 32> and the others sad_generic_kernel."""
    ctx.set_sad_motion_scale(scale)
    if path == "rows_4_byte_aligned":
        stride = (W + 3) // 4 * 4 + 4
        stride += 4 if stride % 16 == 0 else 0
        assert stride % 4 == 0 and stride % 16 != 0
    else:
        stride = (W + 63) // 64 * 64
        ctx.set_option("OFPS_HIP_SAD_KERNEL", "block")
    a, b = cases.frames(W, H, B, R, 77, "subpel"), cases.frames(W, H, B, R, 78, "binary")
    fr = np.ascontiguousarray(np.stack([a[0], a[1], b[0], b[1], a[0]]))           # sub-pel, unrelated, saturated, unrelated pairs
    ent, best = _dev_pairs(ctx, fr, stride, B, R)
    for k in range(len(fr) - 1):
        ent_o, best_o = oracle.sad_flow(fr[k], fr[k + 1], B, R)
        if scale == 4:
            ent_o, best_o = iq.refine(fr[k], fr[k + 1], B, R, best_o)
        _same(ent[k], best[k], ent_o, best_o)
