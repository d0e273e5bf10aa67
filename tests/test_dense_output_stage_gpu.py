"""The output stage both dense decoders (hip_lk, hip_flow) push every frame through -- contrast mask (mask.hip: contrast_mask_kernel), the
ordered compaction of the per-pixel records (compact_small_kernel up to 32,768 pixels; compact_count / _scan / _scatter above), the copy
into the ticket's page-locked block (dense_decoder.hip: dense_copy_records_kernel) and the read-ahead stream's per-ticket mask slots --
against the CPU oracle and against masks written out from the definitions (tests/dense_output_cases.py), bit for bit.
tests/test_dense_output_cases_cpu.py proves on the CPU that each case has the mask shape it is named for."""
from functools import lru_cache

import numpy as np
import pytest

import dense_output_cases as dc
import oracle
from oracle import np_oracle
from ofps_amd import synth

pytestmark = pytest.mark.gpu
LK = (1, 2, 1)                    # levels, radius, iters of the flow under the compaction cases: the flow is not what is tested here
FB = (5, 6, 3)                    # cv-decoder's Farneback call (cv-decoder/src/lib.rs:188-199), as in tests/test_farneback_gpu.py
FB_GEOMETRIES = ((1920, 1080), (2048, 1025))


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


def _oracle_flow(prev, cur, farneback, params):
    if farneback:
        return oracle.farneback_flow(prev, cur, params[0], 2 * params[1] + 1, params[2])
    return oracle.lk_flow(prev, cur, *params)


# ------------------------------------------------------------------------------------------------------------------ the mask kernel
@pytest.mark.parametrize("W,H", dc.MASK_GEOMETRIES)
def test_mask_over_the_geometry_list(ctx, W, H):
    """frames narrower / lower than the 7-pixel halo, one short of / at / one past the 64 x 16 tile and its 74 x 26 thresholded window"""
    for kind in dc.MASK_CONTENTS:
        g = dc.mask_content(kind, W, H)
        m = ctx.contrast_mask(g)
        assert m.shape == (H, W) and m.max(initial=0) <= 1
        np.testing.assert_array_equal(m, oracle.contrast_mask(g), err_msg=kind)
        np.testing.assert_array_equal(m, np_oracle.contrast_mask(g), err_msg=kind)
        if kind == "constant":
            assert not m.any()


@pytest.mark.parametrize("a", dc.SIGNED_AMPLITUDES)
def test_mask_of_one_impulse_at_the_tile_seams(ctx, a):
    """the threshold is `> 20`: 4 * 5 passes nothing, 4 * 6 two taps, 2 * 11 six, 21 all eight -- for every position around the tile seams, the
    expected mask from the literal taps and ellipse (neither oracle)"""
    W, H = dc.SEAM_W, dc.SEAM_H
    for y in dc.SEAM_YS:
        for x in dc.SEAM_XS:
            m = ctx.contrast_mask(dc.impulse_frame(W, H, [(y, x, a)]))
            np.testing.assert_array_equal(m, dc.impulse_mask(W, H, [(y, x, a)]), err_msg=f"impulse {a} at {(y, x)}")
    if abs(a) == 5:
        assert not m.any()


@pytest.mark.parametrize("a", (6, -6, 11, -11, 21, -21))
def test_mask_of_one_impulse_at_the_borders(ctx, a):
    """within 7 pixels of every border and corner (BORDER_REFLECT_101 folds the impulse into the window; the dilation is clipped)"""
    W, H = dc.BORDER_W, dc.BORDER_H
    for y, x in dc.border_placements():
        g = dc.impulse_frame(W, H, [(y, x, a)])
        want = oracle.contrast_mask(g)
        np.testing.assert_array_equal(want, np_oracle.contrast_mask(g))
        np.testing.assert_array_equal(ctx.contrast_mask(g), want, err_msg=f"impulse {a} at {(y, x)}")


@pytest.mark.parametrize("pad", ["255", "noise"])
@pytest.mark.parametrize("extra", [1, 3, 64])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_mask_with_a_row_stride_larger_than_the_width(ctx, entry, extra, pad):
    """rows `stride` > W bytes apart through ofps_hip_contrast_mask and ofps_hip_contrast_mask_dev: the padding bytes (all 255, or noise) are
    never read as pixels -- the reflected border columns come from the row itself -- and the mask comes back dense"""
    import torch
    for W, H in ((200, 33), (65, 17), (129, 31), (7, 5), (3, 2), (333, 77), (64, 16)):
        g = dc.mask_content("texture" if W >= 64 else "noise", W, H)
        stride = W + extra
        buf = np.full((H, stride), 255, np.uint8) if pad == "255" else synth.random_luma(1, stride, H, seed=W + extra)[0].copy()
        buf[:, :W] = g
        want = oracle.contrast_mask(g)
        if entry == "host":
            m = ctx.contrast_mask(buf[:, :W], stride=stride)
        else:
            d_in = torch.from_numpy(buf).cuda()
            d_out = torch.full((H * W + 64,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.contrast_mask_dev(d_in.data_ptr(), W, H, stride, d_out.data_ptr())
            ctx.sync()
            out = d_out.cpu().numpy()
            assert (out[H * W:] == 7).all()                                   # dense output: nothing written past W * H bytes
            m = out[:H * W].reshape(H, W)
        np.testing.assert_array_equal(m, want, err_msg=f"{W}x{H} stride {stride}")
        if W >= 64:
            assert 0 < want.mean() < 1


# ------------------------------------------------------------------------------------------- compaction + record copy, per-pixel records
@pytest.mark.parametrize("W,H,shape", dc.COMPACT_CASES)
def test_masked_records_at_every_compaction_geometry(ctx, W, H, shape):
    """lk_decode(contrast_mask, fullres_records): the surviving records, in raster order, and their count -- the single-workgroup path up to
    32,768 pixels, count / scan / scatter above (one, two and three rounds of the scan's carry loop), ragged and whole last tiles; then the
    same frames through the densifier's masked down-sampling"""
    prev, cur = dc.compaction_pair(W, H, shape)
    mask = dc.oracle_mask(W, H, shape)
    keep = mask.reshape(-1) != 0
    k = int(keep.sum())
    for farneback, params in ((False, LK),) + (((True, FB),) if (W, H) in FB_GEOMETRIES else ()):
        what = f"{W}x{H} ({shape}) {'hip_flow' if farneback else 'hip_lk'}"
        rec_o = oracle.masked_flow_to_entries(_oracle_flow(prev, cur, farneback, params), mask)
        assert len(rec_o) == k
        rec, grid = ctx.lk_decode(prev, cur, *params, contrast_mask=True, fullres_records=True, farneback=farneback)
        full, _ = ctx.lk_decode(prev, cur, *params, fullres_records=True, farneback=farneback)
        print(f"{what}: {len(rec)} records, oracle mask keeps {k} of {W * H}")
        assert grid == (W, H) and len(full) == W * H
        assert len(rec) == k, what
        _same(rec, full[keep], what + ": the context's own unmasked records filtered by the oracle mask")
        _same(rec, rec_o, what + ": oracle flow + oracle mask")
        for cap in (150, 60):
            ent, (gw, gh) = ctx.lk_decode(prev, cur, *params, max_w=cap, max_h=cap, contrast_mask=True, farneback=farneback)
            assert (gw, gh) == oracle.cv_grid(W, H, cap, cap)
            _same(ent, oracle.densify_to_entries(rec_o, gw, gh), what + f": down-sampled to {gw}x{gh}")
            if shape == "a":
                assert len(ent) == 0
            if shape in "def":
                assert 0 < len(ent) < gw * gh


# ----------------------------------------------------------------------------------------------------------------------- reduced mode
@pytest.mark.parametrize("flow", ["lk", "farneback"])
@pytest.mark.parametrize("W,H,cap", dc.REDUCED_CASES)
def test_reduced_mode_around_the_single_workgroup_limit(ctx, W, H, cap, flow):
    """ "Process Fullres" = false with a cap that leaves 32,535 (single workgroup), 32,912 and 40,000 (count / scan / scatter) reduced pixels:
    one record per unmasked pixel of the reduced frame, against the oracle chain (front-end -> flow -> mask -> records)"""
    far = flow == "farneback"
    params = FB if far else (3, 4, 3)
    y = synth.flatten_regions(synth.luma_sequence(2, W, H, max_step=3, seed=W + cap), region=max(24, W // 12), seed=cap)
    bgr = np.clip(y[..., None].astype(int) + np.array([-20, 0, 15]), 0, 255).astype(np.uint8)      # tinted, the flat regions stay flat
    for fr, fmt in ((y, oracle.FMT_LUMA), (bgr, oracle.FMT_BGR)):
        rec_o, grid_o, flow_o = oracle.cv_decode(fr[0], fr[1], fmt, process_fullres=False, max_w=cap, max_h=cap, flow=flow,
                                                 levels=params[0], radius=params[1], iters=params[2])
        rec, grid = ctx.lk_decode(fr[0], fr[1], *params, max_w=cap, max_h=cap, contrast_mask=True, farneback=far, reduced=True, fmt=fmt)
        assert grid == grid_o == ctx.cv_grid(W, H, cap, cap) and grid[0] * grid[1] == dc.REDUCED_PIXELS[(W, H, cap)]
        print(f"{W}x{H} cap {cap} {flow} fmt {fmt}: {len(rec)} of {grid[0] * grid[1]} reduced pixels")
        assert 0 < len(rec_o) < grid[0] * grid[1]
        _same(rec, rec_o, "oracle chain")
        full, _ = ctx.lk_decode(fr[0], fr[1], *params, max_w=cap, max_h=cap, farneback=far, reduced=True, fmt=fmt)
        assert len(full) == grid[0] * grid[1]
        _same(full, oracle.flow_to_entries(flow_o), "unmasked")
        mask = oracle.contrast_mask(oracle.cv_frontend(fr[1], fmt, False, cap, cap))
        _same(rec, full[mask.reshape(-1) != 0], "the unmasked records filtered by the oracle mask")


# ------------------------------------------------------------------------------------------------------------- no state between calls
def test_nothing_is_left_over_from_the_previous_call(ctx):
    """everything, then nothing, at 1080p; then the first general-path size, the last single-workgroup size, and 1080p again: each call's
    count, tile table and mask are its own (S_RESULT, S_WORK0, S_MASK and the page-locked block are reused from call to call)"""
    order = ((1920, 1080, "b"), (1920, 1080, "a"), (99, 331, "c"), (217, 151, "c"), (1920, 1080, "c"))
    for W, H, shape in order:
        prev, cur = dc.compaction_pair(W, H, shape)
        mask = dc.oracle_mask(W, H, shape)
        rec_o = oracle.masked_flow_to_entries(oracle.lk_flow(prev, cur, *LK), mask)
        rec, grid = ctx.lk_decode(prev, cur, *LK, contrast_mask=True, fullres_records=True)
        print(f"{W}x{H} ({shape}): {len(rec)} records, expected {len(rec_o)}")
        assert grid == (W, H)
        _same(rec, rec_o, f"{W}x{H} ({shape})")
    assert len(rec) == int(dc.oracle_mask(1920, 1080, "c").sum())


# ------------------------------------------------------------------------------------------------------------------------ stream forms
@lru_cache(maxsize=32)
def _stream_expected(W, H, kind_prev, kind_cur, farneback, params, fullres, cap):
    """oracle result of one pair of stream frames (the streams cycle through four frames: pairs repeat)"""
    prev, cur = dc.stream_frame(W, H, kind_prev), dc.stream_frame(W, H, kind_cur)
    rec = oracle.masked_flow_to_entries(_oracle_flow(prev, cur, farneback, params), oracle.contrast_mask(cur))
    return rec if fullres else oracle.densify_to_entries(rec, *oracle.cv_grid(W, H, cap, cap))


def _run_stream(ctx, W, H, n_frames, farneback, params, fullres, cap=150, reset=True):
    """n_frames through lk_push_frame_async with two tickets in flight, collected in order; every result against the stateless lk_decode of
    the pair and against the oracle.  -> the record counts"""
    kinds = dc.stream_kinds(n_frames)
    kw = dict(max_w=cap, max_h=cap, contrast_mask=True, fullres_records=fullres, farneback=farneback)
    pins = [ctx.pinned_frame(H, W) for _ in range(3)]
    if reset:
        ctx.lk_reset()
    tickets, got = [], []
    for k, kind in enumerate(kinds):
        np.copyto(pins[k % 3], dc.stream_frame(W, H, kind))
        tickets.append(ctx.lk_push_frame_async(pins[k % 3], *params, **kw))
        if k >= 1:
            r = ctx.lk_frame_wait(tickets[k - 1])
            got.append(None if r is None else (r[0].copy(), r[1]))
    r = ctx.lk_frame_wait(tickets[-1])
    got.append((r[0].copy(), r[1]))
    assert got[0] is None                                   # a stream's first frame has no vectors
    counts = []
    for k in range(1, n_frames):
        what = f"{W}x{H} frame {k} ({kinds[k - 1]} -> {kinds[k]})"
        want, grid = ctx.lk_decode(dc.stream_frame(W, H, kinds[k - 1]), dc.stream_frame(W, H, kinds[k]), *params, **kw)
        assert got[k][1] == grid, what
        _same(got[k][0], want, what + ": stateless lk_decode")
        _same(got[k][0], _stream_expected(W, H, kinds[k - 1], kinds[k], farneback, params, fullres, cap), what + ": oracle")
        counts.append(len(got[k][0]))
    for p in pins:
        ctx.free_pinned(p)
    return counts


@pytest.mark.parametrize("fullres", [True, False])
@pytest.mark.parametrize("decoder", ["hip_lk", "hip_flow"])
def test_stream_tickets_get_their_own_mask_and_count(ctx, decoder, fullres):
    """two tickets in flight whose frames need different masks and very different record counts (everything, nothing, 318, about half): the
    mask is made on the upload stream into the ticket's own slot of S_LK_MASKS, the count lands in the ticket's own block"""
    W, H = 480, 270
    far = decoder == "hip_flow"
    counts = _run_stream(ctx, W, H, 9, far, FB if far else (3, 4, 3), fullres)
    print(f"{decoder} fullres_records={fullres}: record counts {counts}")
    if fullres:
        assert counts[:4] == [0, 318, counts[2], W * H] and 0.25 * W * H < counts[2] < 0.75 * W * H
    else:
        assert counts[0] == 0 and 0 < counts[1] < counts[2] <= counts[3] == 150 * 84
    ctx.lk_reset()


def test_stream_at_1080p(ctx):
    """the cfg3 size: per-ticket mask slots of 2 MB, result blocks of 33 MB, two rounds of the scan"""
    counts = _run_stream(ctx, 1920, 1080, 8, False, LK, True)
    print(f"1080p record counts {counts}")
    assert counts[0] == 0 and counts[1] == 318 and counts[3] == 1920 * 1080 and 0.25 < counts[2] / (1920 * 1080) < 0.75
    counts = _run_stream(ctx, 1920, 1080, 5, False, LK, False)
    assert counts[0] == 0 and counts[3] == 150 * 84
    ctx.lk_reset()


def test_stream_restart_grows_the_result_blocks(ctx):
    """a stream at 256 x 128 (single-workgroup compaction straight into a 0.5 MB block), drained, restarts at 1920 x 1080: the tickets'
    page-locked blocks and the mask slots have to grow, and the first 1080p frame is a stream's first frame again"""
    small = _run_stream(ctx, 256, 128, 6, False, LK, True)
    assert small[:4] == [0, 318, small[2], 256 * 128]
    big = _run_stream(ctx, 1920, 1080, 6, False, LK, True, reset=False)
    assert big[:4] == [0, 318, big[2], 1920 * 1080]
    ctx.lk_reset()
