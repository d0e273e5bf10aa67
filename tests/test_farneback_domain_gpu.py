"""hip_flow (ofps_amd/csrc/farneback.hip) over its kernel and parameter domain against its CPU restatement (oracle/farneback_oracle.c): every
instantiation of the window update (fb_iter_kernel<0 .. 7>) and of the polynomial expansion (fb_polyexp_kernel<7>, <5>, <0> at poly_n 1 .. 15),
every pyramid depth 0 .. 6, the three LDS row pitches of the row filter with every rows-per-lane form, the byte paths for unaligned rows,
frames smaller than a tile, 1 .. 64 updates, initial flows, the refusals, and what one call leaves behind for the next.  The case lists
are data in tests/farneback_cases.py; tests/test_farneback_domain_cpu.py checks that every case has the property it is named for and that the
oracle agrees with the independent float64 restatement over the same grid.

Every comparison is IDENTITY OF BITS (flow and records viewed as uint32), tolerance 0: README / DESIGN claim "bit-identical to its CPU
restatement", and every stage restates the same operations in the same order.  PARITY UNPINNED with respect to the reference, as in
tests/test_farneback_gpu.py: cv-decoder calls OpenCV (cv-decoder/src/lib.rs:188-199), which is not there to compare with."""
from functools import lru_cache

import numpy as np
import pytest

import farneback_cases as FC
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, what=""):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    same = float((_u32(got) == _u32(want)).mean())
    assert same == 1.0, (what, same, float(np.abs(got - want).max()))


def _check_pair(ctx, a, b, what="", **kw):
    """flow and records of one pair against the oracle's; kw as farneback_flow takes them (poly_sigma already a float32 value)"""
    f_o = _oracle(a, b, **kw)
    f_g, e_g = ctx.farneback_flow(a, b, want_entries=True, **kw)
    _same_bits(f_g, f_o, what)
    _same_bits(e_g, oracle.flow_to_entries(f_o), what + " records")
    return f_o


def _oracle(a, b, **kw):
    return oracle.farneback_flow(a, b, **kw)


@lru_cache(maxsize=None)
def _oracle_of_clip(W, H, levels, iters, first):
    """the oracle's flow of frames (first, first + 1) of the three-frame clip of this size: shared by the layer and the initial-flow cases"""
    fr = FC.regions(W, H, n=3)
    f = oracle.farneback_flow(fr[first], fr[first + 1], levels=levels, iters=iters)
    f.setflags(write=False)
    return f


# ---- (a) window x polynomial grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("winsize", FC.WINSIZES)
def test_every_window_with_every_expansion(ctx, winsize):
    """fb_iter_kernel<winsize / 2> with fb_polyexp_kernel<0> at poly_n 1, 2, 3, 4, 6, 9, 12, 15, <5> and <7>, each also with poly_sigma = 0 (the
    0.3 n rule of make_poly) at 5, 7 and 15: 97 x 64 at levels 3 (two layers, ragged 4 x 4 update tiles and 2 x 4 expansion tiles), 2 updates"""
    fr = FC.regions(FC.GRID_W, FC.GRID_H)
    for kw in FC.grid_sets(winsize):
        _check_pair(ctx, fr[0], fr[1], str(kw), **kw)


@pytest.mark.parametrize("winsize,poly_n", FC.CORNERS)
def test_the_grids_corners_on_three_layers(ctx, winsize, poly_n):
    fr = FC.regions(FC.CORNER_W, FC.CORNER_H)
    _check_pair(ctx, fr[0], fr[1], levels=FC.CORNER_LEVELS, winsize=winsize, iters=FC.GRID_ITERS, poly_n=poly_n, poly_sigma=FC.grid_sigma(poly_n))


# ---- (b) every layer count and every row-filter variant -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.LAYER_CASES)
def test_every_layer_count_and_row_filter_variant(ctx, name):
    """0 .. 6 layers above the frame (layer 6: 159 taps in the row filter, the column chain at r = 79), `levels` below what the size allows, the
    row pitches 1 and 2 with every rows-per-lane form, one column either side of both pitch switch points, and the widest legal frame"""
    c = FC.LAYER_CASES[name]
    fr = FC.regions(c["W"], c["H"], n=3)
    f_o = _oracle_of_clip(c["W"], c["H"], c["levels"], c["iters"], 0)
    f_g, e_g = ctx.farneback_flow(fr[0], fr[1], levels=c["levels"], iters=c["iters"], want_entries=True)
    _same_bits(f_g, f_o, name)
    _same_bits(e_g, oracle.flow_to_entries(f_o), name + " records")


# ---- (c) small and ragged frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", FC.SMALL_FRAMES)
def test_frames_around_and_below_the_tile_sizes(ctx, W, H):
    """tiles are 32 x 16 (update) and 64 x 16 (expansion) with halos of up to 7 and 15: frames of one pixel, one row, one column, a tile less
    one, a tile exactly, a tile and one -- at cv-decoder's arguments and at the widest halos (winsize 15, poly_n 15)"""
    fr = FC.regions(W, H)
    for kw in ({}, FC.LARGEST):
        _check_pair(ctx, fr[0], fr[1], f"{W}x{H} {kw}", **kw)


# ---- (d) row stride and alignment through the device entry ----------------------------------------------------------------------------------
def _dev_call(ctx, a, b, stride, fill, offset, outputs, **kw):
    import torch
    H, W = a.shape
    bufs = [torch.from_numpy(FC.padded(f, stride, fill, offset, seed=s)[0]).cuda() for s, f in enumerate((a, b))]
    guard = 64
    d_flow = torch.full((H * W * 2 + guard,), 7.0, dtype=torch.float32, device="cuda") if outputs in ("flow", "both") else None
    d_ent = torch.full((H * W * 4 + guard,), 7.0, dtype=torch.float32, device="cuda") if outputs in ("records", "both") else None
    torch.cuda.synchronize()
    ctx.farneback_flow_dev(bufs[0].data_ptr() + offset, bufs[1].data_ptr() + offset, W, H, stride,
                           d_out_flow=None if d_flow is None else d_flow.data_ptr(), d_out_entries=None if d_ent is None else d_ent.data_ptr(), **kw)
    ctx.sync()
    out = []
    for d, n in ((d_flow, 2), (d_ent, 4)):
        if d is None:
            out.append(None)
            continue
        h = d.cpu().numpy()
        assert (h[H * W * n:] == 7.0).all()                                       # dense output: nothing written past it
        out.append(h[:H * W * n].reshape(H, W, 2) if n == 2 else h[:H * W * n].reshape(H * W, 4))
    return out


@pytest.mark.parametrize("fill", FC.STRIDE_FILLS)
@pytest.mark.parametrize("W,H", FC.STRIDE_SIZES)
def test_row_strides_and_unaligned_rows_through_the_device_entry(ctx, W, H, fill):
    """ofps_hip_farneback_flow_dev with rows W + 1, W + 3, W + 64 bytes apart and, at W + 64, frames that start 1, 2, 3 bytes into their
    buffer: fb_pyr_h_kernel copies rows as dwords and fb_polyexp_kernel takes its `whole` branch only when stride and pointer are 4-byte
    aligned (640 + 64 at offset 0), byte by byte otherwise.  The padding (255 or noise) is never read as a pixel: the oracle on the dense frames."""
    fr = FC.regions(W, H)
    f_o = _oracle(fr[0], fr[1])
    e_o = oracle.flow_to_entries(f_o)
    k = 0
    for pad, offset in [(p, 0) for p in FC.STRIDE_PADS] + [(64, o) for o in FC.BASE_OFFSETS]:
        outputs = FC.OUTPUTS[k % 3]; k += 1
        f_g, e_g = _dev_call(ctx, fr[0], fr[1], W + pad, fill, offset, outputs)
        if f_g is not None:
            _same_bits(f_g, f_o, f"stride W + {pad}, offset {offset}")
        if e_g is not None:
            _same_bits(e_g, e_o, f"stride W + {pad}, offset {offset}, records")


def test_every_output_combination_through_the_device_entry(ctx):
    fr = FC.regions(322, 181)
    f_o = _oracle(fr[0], fr[1])
    for outputs in FC.OUTPUTS:
        f_g, e_g = _dev_call(ctx, fr[0], fr[1], 322 + 64, "noise", 3, outputs)
        assert (f_g is None) == (outputs == "records") and (e_g is None) == (outputs == "flow")
        if f_g is not None:
            _same_bits(f_g, f_o, outputs)
        if e_g is not None:
            _same_bits(e_g, oracle.flow_to_entries(f_o), outputs)


# ---- (e) iterations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", FC.ITERS)
def test_one_to_sixty_four_updates(ctx, iters):
    """the M planes ping-pong (Mb[it & 1]); the last update of a layer writes no matrices, the others no flow"""
    fr = FC.regions(FC.ITERS_W, FC.ITERS_H)
    _check_pair(ctx, fr[0], fr[1], iters=iters)


# ---- (f) initial flow -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.INIT_CASES)
def test_initial_flow_from_the_previous_pair(ctx, name):
    """OPTFLOW_USE_INITIAL_FLOW as cv-decoder uses it (cv-decoder/src/lib.rs:161-165): fb_area_kernel brings the previous pair's flow to the
    coarsest layer at ratios 1, 2, 4, 8, 8 x 7.94 and 64"""
    c = FC.INIT_CASES[name]
    fr = FC.regions(c["W"], c["H"], n=3)
    kw = dict(levels=c["levels"], iters=c["iters"])
    first = _oracle_of_clip(c["W"], c["H"], c["levels"], c["iters"], 0)
    f_o = _oracle(fr[1], fr[2], init=first, **kw)
    if c["W"] * c["H"] <= 512 * 512:                                               # (the cold flow of the large case costs the oracle 5 s)
        assert not np.array_equal(f_o, _oracle_of_clip(c["W"], c["H"], c["levels"], c["iters"], 1))
    f_g, e_g = ctx.farneback_flow(fr[1], fr[2], init=first, want_entries=True, **kw)
    _same_bits(f_g, f_o, name)
    _same_bits(e_g, oracle.flow_to_entries(f_o), name + " records")


@pytest.mark.parametrize("kind", FC.SYNTH_INITS)
def test_synthetic_initial_flows(ctx, kind):
    """finite starting flows: sub-pixel noise, +-40 px, and one that points outside the frame at every pixel (the warp's `inside` test fails
    everywhere in the coarsest layer's first matrices)"""
    fr = FC.regions(FC.SYNTH_INIT_W, FC.SYNTH_INIT_H)
    init = FC.synthetic_init(kind)
    for kw in (dict(), dict(levels=0), dict(levels=0, iters=1)):
        f_o = _oracle(fr[0], fr[1], init=init, **kw)
        f_g, e_g = ctx.farneback_flow(fr[0], fr[1], init=init, want_entries=True, **kw)
        _same_bits(f_g, f_o, f"{kind} {kw}")
        _same_bits(e_g, oracle.flow_to_entries(f_o), f"{kind} {kw} records")


# ---- (g) refusals -----------------------------------------------------------------------------------------------------------------------------
def test_everything_without_a_kernel_is_refused_and_the_context_stays_usable(ctx):
    from ofps_amd.runtime import OfpsHipError
    fr = FC.regions(128, 96)
    want = _oracle(fr[0], fr[1])
    for kw in FC.REFUSED_PARAMS:
        with pytest.raises(OfpsHipError):
            ctx.farneback_flow(fr[0], fr[1], **kw)
        _same_bits(ctx.farneback_flow(fr[0], fr[1]), want, f"after {kw}")
    for g in FC.REFUSED_GEOMETRIES:
        z = np.zeros((2, g["H"], g["W"]), np.uint8)
        with pytest.raises(OfpsHipError):
            ctx.farneback_flow(z[0], z[1], levels=g["levels"])
        _same_bits(ctx.farneback_flow(fr[0], fr[1]), want, f"after {g}")


def test_a_stream_refuses_on_its_first_frame_and_stays_empty(ctx):
    """farneback_check_params: "a stream never accepts a frame and fails the next" -- the refusal comes with the FIRST frame (which runs no
    flow), and the refused frame is not the stream's previous frame afterwards"""
    from ofps_amd.runtime import OfpsHipError
    fr = FC.regions(FC.STREAM_W, FC.STREAM_H, n=3)
    kw = dict(contrast_mask=True, farneback=True)
    GRID = oracle.cv_grid(FC.STREAM_W, FC.STREAM_H)
    refused = [(fr[0], dict(levels=5, radius=8, iters=3)),                                              # winsize 17
               (fr[0], dict(levels=5, radius=6, iters=65)),
               (np.zeros((4096, 4096), np.uint8), dict(levels=7, radius=6, iters=3)),                  # seven layers above the frame
               (np.zeros((8, 16385), np.uint8), dict(levels=5, radius=6, iters=3))]
    want = ctx.lk_decode(fr[0], fr[1], 5, 6, 3, **kw)[0]
    _same_bits(want, oracle.densify_to_entries(oracle.masked_flow_to_entries(_oracle(fr[0], fr[1]), oracle.contrast_mask(fr[1])), *GRID), "pair")
    for frame, a in refused:
        ctx.lk_reset()
        with pytest.raises(OfpsHipError):
            ctx.lk_push_frame(frame, a["levels"], a["radius"], a["iters"], **kw)
        assert ctx.lk_push_frame(fr[0], 5, 6, 3, **kw) is None                   # the stream was empty
        ent, grid = ctx.lk_push_frame(fr[1], 5, 6, 3, **kw)
        assert grid == GRID
        _same_bits(ent, want, str(a))
    ctx.lk_reset()


# ---- (h) nothing left over between calls ------------------------------------------------------------------------------------------------------
def test_nothing_is_left_over_from_the_previous_call(ctx):
    """one context, back to back: a wide frame on the second row pitch, a 64 x 64 frame at poly_n 15, 640 x 360 at poly_n 5, the wide frame
    again -- between two frames of a 352 x 200 stream, whose next pair must be the pair call's and must not count a cache hit for planes
    that were made for another geometry and another poly_n"""
    fr = FC.regions(FC.STREAM_W, FC.STREAM_H, n=4)
    kw = dict(contrast_mask=True, farneback=True)
    GRID = oracle.cv_grid(FC.STREAM_W, FC.STREAM_H)

    def chain(a, b):
        return oracle.densify_to_entries(oracle.masked_flow_to_entries(_oracle(a, b), oracle.contrast_mask(b)), *GRID)
    ctx.lk_reset()
    h0 = ctx.flow_cache_hits()
    assert ctx.lk_push_frame(fr[0], 5, 6, 3, **kw) is None
    _same_bits(ctx.lk_push_frame(fr[1], 5, 6, 3, **kw)[0], chain(fr[0], fr[1]), "stream pair 0")
    assert ctx.flow_cache_hits() - h0 == 1
    wide = {}
    for W, H, poly_n in FC.BACK_TO_BACK:
        p = FC.regions(W, H)
        a = dict(iters=1, poly_n=poly_n, poly_sigma=FC.grid_sigma(poly_n))
        if (W, H) not in wide:
            wide[(W, H)] = _oracle(p[0], p[1], **a)
        _same_bits(ctx.farneback_flow(p[0], p[1], **a), wide[(W, H)], f"{W}x{H} poly_n {poly_n}")
    assert ctx.flow_cache_hits() - h0 == 1
    _same_bits(ctx.lk_push_frame(fr[2], 5, 6, 3, **kw)[0], chain(fr[1], fr[2]), "stream pair 1")
    assert ctx.flow_cache_hits() - h0 == 1                                        # frame 1's planes were another call's by then: expanded again
    _same_bits(ctx.lk_push_frame(fr[3], 5, 6, 3, **kw)[0], chain(fr[2], fr[3]), "stream pair 2")
    assert ctx.flow_cache_hits() - h0 == 2
    ctx.lk_reset()


# ---- (i) decoder arguments --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,radius", FC.DECODER_ARGS)
def test_decoder_arguments_reach_the_flow(ctx, levels, radius):
    """lk_decode(farneback): levels = the pyramid's, winsize = 2 * radius + 1 (dense_decoder.hip), poly_n 7, poly_sigma 1.5: the oracle chain
    flow -> masked records -> down-sampling to the capped grid, with windows 1, 5, 15 and 0, 3 (of 6 asked for) and 3 layers"""
    fr = FC.regions(FC.DECODER_W, FC.DECODER_H)
    flow = _oracle(fr[0], fr[1], levels=levels, winsize=FC.decoder_winsize(radius), iters=3, poly_n=7, poly_sigma=1.5)
    want = oracle.densify_to_entries(oracle.masked_flow_to_entries(flow, oracle.contrast_mask(fr[1])), 150, 84)
    ent, grid = ctx.lk_decode(fr[0], fr[1], levels, radius, 3, contrast_mask=True, farneback=True)
    assert grid == (150, 84)
    _same_bits(ent, want, f"levels {levels} radius {radius}")
