"""-m gpu: the quarter-pel refinement (N1q, ofps_hip_set_sad_motion_scale(ctx, 4)) through the C ABI against the NumPy restatement
tests/indep_sad_qpel.py on the CPU oracle's integer winners.  All-integer arithmetic: (Dx, Dy, SAD) equal as integers, the records
as f32 bit patterns, on every search path (strip, per-block, pruned, generic) and every single-context entry point that runs a
search: ofps_hip_sad_flow, _sad_flow_dev (both reference modes, with and without out_best, growing and shrinking geometries and
batches), push_frame / push_frame_async / push_frames_async with the detector and the estimator off and on (LSQ and RANSAC, the scale
flipped mid-stream), the Python decoder and the C++ host.  Elsewhere: the whole block / range domain and frames smaller than the
refinement's window in tests/test_sad_qpel_properties_gpu.py, the multi-device dispatcher in tests/test_multi_device_qpel.py.
Left out: the batched and the multi-device streams return no detector field, so there only the island's id and the field's side
are compared; the LK / Farneback decoders have no motion scale."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from ofps_amd import _lib, mvec, synth
from ofps_amd._lib import OfpsHipError

import indep_sad_qpel as iq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sad_qpel.npz")
TOOL = os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool")
OFPS_HIP_EINVAL = -1


@pytest.fixture()
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    c.set_sad_motion_scale(4)
    yield c
    c.close()


def _frames(W, H, R, kind, n=2):
    if kind == "seq":
        return synth.luma_sequence(n, W, H, max_step=min(R, 6), seed=synth.SEED0 + W + H)
    if kind == "pan":                                 # sub-pel global motion + sensor noise
        return synth.luma_sequence(n, W, H, max_step=3, seed=3, region=4096, noise=1)
    if kind == "random":
        return synth.random_luma(n, W, H, seed=7)
    if kind == "blocky":                              # 4x4 cells of two levels: thousands of exact SAD ties
        rng = np.random.default_rng(W * 131 + H)
        cells = (rng.integers(0, 2, (n, (H + 3) // 4, (W + 3) // 4)) * 200 + 20).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(cells, 4, axis=1), 4, axis=2)[:, :H, :W])
    if kind == "subpel":                              # frame 1 = frame 0 rendered (5, -7) quarter pels away with the spec's interpolation, + noise
        prev = synth.luma_sequence(1, W, H, max_step=0, seed=91)[0]
        q = iq.quarter_plane(prev)
        Y, X = np.mgrid[0:H, 0:W]
        cur = q[np.clip(4 * Y - 7, 0, q.shape[0] - 1), np.clip(4 * X + 5, 0, q.shape[1] - 1)].astype(np.int32)
        cur += np.random.default_rng(4).integers(-2, 3, cur.shape)
        return np.stack([prev, np.clip(cur, 0, 255).astype(np.uint8)])
    if kind == "border":                              # the scene slides out of the frame: edge blocks' winners stop at the frame border
        wide = synth.luma_sequence(1, W + 16, H + 16, max_step=0, seed=17)[0]
        return np.ascontiguousarray(np.stack([wide[8:8 + H, 8:8 + W], wide[3:3 + H, 14:14 + W]]))
    return np.full((n, H, W), 77, np.uint8)


def _expect(prev, cur, B, R):
    _, best_i = oracle.sad_flow(prev, cur, B, R, threads=8)
    ent, best = iq.refine(prev, cur, B, R, best_i)
    return ent, best, best_i


def _same(ent_g, best_g, ent_e, best_e):
    np.testing.assert_array_equal(best_g, best_e)                                  # (Dx, Dy, SAD): integers
    np.testing.assert_array_equal(ent_g.view(np.uint32), ent_e.view(np.uint32))    # records: the same bits


CASES = [
    (1920, 1080, 16, 16, "pan"),       # the flagship geometry (strip search)
    (1024, 576, 8, 32, "seq"),         # the 4K configuration's block / range on a crop
    (640, 360, 16, 8, "seq"),
    (640, 360, 16, 16, "subpel"),      # every block's winner is fractional
    (320, 200, 8, 16, "subpel"),
    (100, 70, 16, 16, "seq"),          # no multiple of the block; ofps_hip_sad_flow pads the device stride to 128
    (200, 120, 8, 8, "pan"),
    (96, 96, 12, 5, "seq"),            # generic search and generic refinement
    (64, 48, 32, 4, "seq"),            # generic, SAD beyond 16 bits
    (192, 112, 16, 10, "seq"),         # generic search, templated refinement
    (70, 50, 5, 3, "seq"),             # a block that is no multiple of 4: byte-wise current block
    (192, 96, 16, 16, "flat"),         # every candidate ties at 0: D = 4 d
    (192, 96, 16, 16, "random"),
    (256, 144, 16, 16, "blocky"),      # tie-heavy
    (256, 136, 8, 32, "blocky"),
    (320, 192, 16, 16, "border"),      # validity clipping
    (320, 192, 8, 8, "border"),
]


@pytest.mark.parametrize("W,H,B,R,kind", CASES)
def test_quarter_pel_matches_the_restatement_bit_exact(ctx, W, H, B, R, kind):
    fr = _frames(W, H, R, kind)
    ent_e, best_e, best_i = _expect(fr[0], fr[1], B, R)
    if kind == "border":
        nbx = W // B
        x0 = (np.arange(len(best_i)) % nbx) * B; y0 = (np.arange(len(best_i)) // nbx) * B
        on_border = (x0 + best_i[:, 0] == 0) | (x0 + best_i[:, 0] + B == W) | (y0 + best_i[:, 1] == 0) | (y0 + best_i[:, 1] + B == H)
        moved = (best_i[:, :2] != 0).any(axis=1)
        assert (on_border & moved).sum() >= 4                                      # displaced winners that touch the border exist
    if kind == "flat":
        np.testing.assert_array_equal(best_e[:, :2], 4 * best_i[:, :2])
    ent_g, best_g = ctx.sad_flow(fr[0], fr[1], B, R, want_best=True)
    _same(ent_g, best_g, ent_e, best_e)
    assert (best_g[:, 2] <= best_i[:, 2]).all()
    if kind == "subpel":
        assert ((best_g[:, :2] % 4) != 0).any(axis=1).mean() > 0.9
    if kind in ("pan", "seq") and W >= 200:
        assert ((best_g[:, :2] % 4) != 0).any()                                    # fractional winners occur


def test_pruned_search_mode_gets_the_same_refinement(ctx):
    fr = _frames(640, 368, 16, "pan")
    ent_e, best_e, _ = _expect(fr[0], fr[1], 16, 16)
    ctx.set_sad_mode(ctx.SAD_PRUNED)
    ent_g, best_g = ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True)
    _same(ent_g, best_g, ent_e, best_e)


def _dev_run(ctx, fr, stride, ref_mode, B, R, with_best):
    n, H, W = fr.shape
    pitch = stride * H
    buf = np.zeros((n, H, stride), np.uint8); buf[:, :, :W] = fr
    nblk = (W // B) * (H // B)
    d_fr, d_ent, d_best = ctx.malloc(buf.nbytes), ctx.malloc((n - 1) * nblk * 16), ctx.malloc((n - 1) * nblk * 12)
    try:
        ctx.memcpy_h2d(d_fr, buf)
        ctx.sad_flow_dev(d_fr, n, W, H, stride, pitch, ref_mode, B, R, d_ent, d_best if with_best else None)
        ent = np.zeros(((n - 1), nblk, 4), np.float32); best = np.zeros(((n - 1), nblk, 3), np.int32)
        ctx.memcpy_d2h(ent, d_ent)
        if with_best:
            ctx.memcpy_d2h(best, d_best)
    finally:
        for p in (d_fr, d_ent, d_best):
            ctx.free(p)
    return ent, (best if with_best else None)


@pytest.mark.parametrize("ref_mode", [0, 1])
@pytest.mark.parametrize("with_best", [True, False])
def test_sad_flow_dev_both_ref_modes_with_and_without_out_best(ctx, ref_mode, with_best):
    fr = _frames(256, 144, 16, "pan", n=4)
    ent, best = _dev_run(ctx, fr, 256, ref_mode, 16, 16, with_best)
    for k in range(3):
        ent_e, best_e, _ = _expect(fr[0 if ref_mode else k], fr[k + 1], 16, 16)
        np.testing.assert_array_equal(ent[k].view(np.uint32), ent_e.view(np.uint32))
        if with_best:
            np.testing.assert_array_equal(best[k], best_e)


@pytest.mark.parametrize("W,H,B,R", [(100, 70, 16, 16), (200, 120, 8, 16)])
def test_rows_only_four_byte_aligned_take_the_per_block_search(ctx, W, H, B, R):
    fr = _frames(W, H, R, "seq", n=3)
    stride = W + 4                                                                # 4-byte aligned, not 16
    assert stride % 16 != 0
    ent, best = _dev_run(ctx, fr, stride, 0, B, R, True)
    for k in range(2):
        ent_e, best_e, _ = _expect(fr[k], fr[k + 1], B, R)
        _same(ent[k], best[k], ent_e, best_e)


def test_push_frame_sync_async_and_batched_equal_the_stage_wise_call(ctx):
    W, H, B, R, n = 320, 192, 16, 16, 5
    fr = _frames(W, H, R, "pan", n=n)
    want = [ctx.sad_flow(fr[k], fr[k + 1], B, R) for k in range(n - 1)]
    for k in range(n - 1):
        np.testing.assert_array_equal(want[k].view(np.uint32), _expect(fr[k], fr[k + 1], B, R)[0].view(np.uint32))
    # synchronous
    ctx.reset_frames()
    for k in range(n):
        r = ctx.push_frame(fr[k], B, R, detector=False, estimator=False, want_entries=True)
        assert r["have_vectors"] == (k > 0)
        if k:
            np.testing.assert_array_equal(r["entries"].view(np.uint32), want[k - 1].view(np.uint32))
    # read-ahead: two tickets in flight
    ctx.reset_frames()
    nblk = (W // B) * (H // B)
    pinned = [ctx.pinned_frame(H, W) for _ in range(2)]
    outs = [ctx.pinned_array((nblk, 4)) for _ in range(2)]
    tickets = []
    for k in range(n):
        if len(tickets) == 2:
            t, j = tickets.pop(0)
            r = ctx.frame_wait(t)
            assert r["have_vectors"] == (j > 0)
            if j:
                np.testing.assert_array_equal(outs[j % 2].view(np.uint32), want[j - 1].view(np.uint32))
        np.copyto(pinned[k % 2], fr[k])
        tickets.append((ctx.push_frame_async(pinned[k % 2], B, R, detector=False, estimator=False, out_entries=outs[k % 2]), k))
    for t, j in tickets:
        ctx.frame_wait(t)
        np.testing.assert_array_equal(outs[j % 2].view(np.uint32), want[j - 1].view(np.uint32))
    # batched
    ctx.reset_frames()
    out = np.zeros((n, nblk, 4), np.float32)
    t = ctx.push_frames_async(np.ascontiguousarray(fr), B, R, detector=False, estimator=False, out_entries=out)
    res = ctx.frames_wait(t)
    assert [r["have_vectors"] for r in res] == [False] + [True] * (n - 1)
    for k in range(1, n):
        np.testing.assert_array_equal(out[k].view(np.uint32), want[k - 1].view(np.uint32))


# ------------------------------------------------------------------ the fused per-frame path with the detector and the estimator on
FW, FH, FB, FR, FN = 640, 360, 16, 8, 5
FASPECT, FFOV = 16 / 9, 22.275


def _fused_sequences():
    return {"seq": synth.luma_sequence(FN, FW, FH, max_step=8), "pan": _frames(FW, FH, FR, "pan", n=FN)}


def _fused_expect(fr, scales):
    """per frame k >= 1: (records, detector result, LSQ quaternion) of the stage-wise CPU chain at that frame's motion scale"""
    cam = oracle.camera(FASPECT, FFOV)
    out = [None]
    for k in range(1, len(fr)):
        ent, best_i = oracle.sad_flow(fr[k - 1], fr[k], FB, FR, threads=8)
        if scales[k] == 4:
            ent, _ = iq.refine(fr[k - 1], fr[k], FB, FR, best_i)
        out.append((ent, oracle.detect_motion(ent), oracle.solve_ypr_given(ent, cam)))
    return out


def _check_fused(k, exp, have_vectors, entries, motion, field, quat):
    """motion: None | (area, dim or None); field: the detector's field, or None where the entry point returns none"""
    if exp is None:
        assert not have_vectors and motion is None, k
        return
    ent_e, det_e, quat_e = exp
    assert have_vectors, k
    np.testing.assert_array_equal(entries.view(np.uint32), ent_e.view(np.uint32), err_msg=f"frame {k}")
    assert (motion is None) == (det_e is None), k
    if det_e is not None:
        assert motion[0] == det_e[0], k                                            # island id
        if motion[1] is not None:
            assert motion[1] == det_e[1].shape[0], k
        if field is not None:
            np.testing.assert_array_equal(field.view(np.uint32), det_e[1].view(np.uint32), err_msg=f"frame {k}")
    np.testing.assert_allclose(quat, quat_e, atol=2e-6, rtol=0, err_msg=f"frame {k}")


def _push_sync(ctx, fr, scales, **kw):
    ctx.reset_frames()
    res = []
    for k in range(len(fr)):
        ctx.set_sad_motion_scale(scales[k])
        r = ctx.push_frame(fr[k], block=FB, search_range=FR, aspect=FASPECT, fov_y_deg=FFOV, want_entries=True, want_field=True, **kw)
        mo = r["motion"]
        res.append((r["have_vectors"], r["entries"], None if mo is None else (mo[0], None), None if mo is None else mo[1], r["quat"]))
    return res


def _push_async(ctx, fr, scales, **kw):
    """two tickets in flight; detector and estimator on, so the detector is forked onto the auxiliary stream behind the search"""
    ctx.reset_frames()
    nblk = (FW // FB) * (FH // FB)
    dim = ctx.block_dim(0.05, 3)
    pinned = [ctx.pinned_frame(FH, FW) for _ in range(2)]
    ents = [ctx.pinned_array((nblk, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    res, tickets = [], []

    def collect():
        t, j = tickets.pop(0)
        r = ctx.frame_wait(t)
        mo = r["motion"]
        res.append((r["have_vectors"], ents[j % 2].copy(), mo, None if mo is None else flds[j % 2].copy(), r["quat"]))

    try:
        for k in range(len(fr)):
            if len(tickets) == 2:
                collect()
            np.copyto(pinned[k % 2], fr[k])
            ctx.set_sad_motion_scale(scales[k])
            tickets.append((ctx.push_frame_async(pinned[k % 2], block=FB, search_range=FR, aspect=FASPECT, fov_y_deg=FFOV,
                                                 out_entries=ents[k % 2], out_field=flds[k % 2], **kw), k))
        while tickets:
            collect()
    finally:
        for a in pinned + ents + flds:
            ctx.free_pinned(a)
    return res


def _push_batched(ctx, fr, scales, **kw):
    """one batch: the entry point returns the island's id and the field's side, not the field"""
    assert len(set(scales)) == 1
    ctx.reset_frames()
    ctx.set_sad_motion_scale(scales[0])
    out = np.zeros((len(fr), (FW // FB) * (FH // FB), 4), np.float32)
    t = ctx.push_frames_async(np.ascontiguousarray(fr), block=FB, search_range=FR, aspect=FASPECT, fov_y_deg=FFOV, out_entries=out, **kw)
    return [(r["have_vectors"], out[k], r["motion"], None, r["quat"]) for k, r in enumerate(ctx.frames_wait(t))]


@pytest.mark.parametrize("push", [_push_sync, _push_async, _push_batched], ids=["push_frame", "push_frame_async", "push_frames_async"])
@pytest.mark.parametrize("name", ["seq", "pan"])
def test_push_frame_at_scale_four_matches_the_stagewise_chain_with_detector_and_estimator_on(ctx, name, push):
    """tests/test_gpu_parity.py::test_push_frame_matches_stagewise_oracle at motion scale 4: the refinement is a second launch
    between the search and the fork of the detector's stream, and writes the records both stages read."""
    fr = _fused_sequences()[name]
    scales = [4] * FN
    exp = _fused_expect(fr, scales)
    if name == "pan":
        assert ((np.round(exp[1][0][:, 2] * FW * 4).astype(int) % 4) != 0).any()   # sub-pel motion is in the records
    for k, got in enumerate(push(ctx, fr, scales)):
        _check_fused(k, exp[k], *got)


def test_push_frame_async_with_ransac_at_scale_four(ctx):
    fr = _fused_sequences()["pan"]
    scales = [4] * FN
    kw = dict(use_ransac=True, num_iters=200, seed=12345)
    got_a = _push_async(ctx, fr, scales, **kw)
    got_s = _push_sync(ctx, fr, scales, **kw)
    exp = _fused_expect(fr, scales)
    cam = oracle.camera(FASPECT, FFOV)
    for k in range(1, FN):
        np.testing.assert_array_equal(got_a[k][1].view(np.uint32), exp[k][0].view(np.uint32))
        np.testing.assert_array_equal(got_s[k][1].view(np.uint32), exp[k][0].view(np.uint32))
        # the same seed on the same records: the same bits, forked or not
        np.testing.assert_array_equal(got_a[k][4].view(np.uint32), got_s[k][4].view(np.uint32), err_msg=f"frame {k}")
        # HIP and CPU RANSAC agree to 1e-4 per component (tests/test_sad_qpel_accuracy_gpu.py)
        q_o = oracle.solve_ypr_ransac(exp[k][0], cam, num_iters=200, seed=12345)
        np.testing.assert_allclose(got_a[k][4], q_o, atol=1e-4, rtol=0, err_msg=f"frame {k}")


@pytest.mark.parametrize("push", [_push_sync, _push_async], ids=["push_frame", "push_frame_async"])
def test_scale_flips_between_frames_of_one_stream_with_detector_and_estimator_on(ctx, push):
    fr = _fused_sequences()["pan"]
    scales = [4, 4, 1, 4, 1]                                                       # frames 1..4 are searched at 4, 1, 4, 1
    exp = _fused_expect(fr, scales)
    for k, got in enumerate(push(ctx, fr, scales)):
        _check_fused(k, exp[k], *got)


# ------------------------------------------------------------------ scratch regrowth, a batch after a batch
def test_geometry_grows_and_shrinks_on_one_context(ctx):
    """ofps_hip_sad_flow (its own result buffers regrow) and ofps_hip_sad_flow_dev without out_best (the integer winners live in the
    context's S_SAD_QBEST scratch, sized by the call): small, large, small, large with another block size."""
    order = [(64, 48, 16), (1920, 1080, 8), (64, 48, 16), (1920, 1080, 16)]
    frames = {(W, H): _frames(W, H, 16, "pan") for W, H, _ in order}
    expect = {g: _expect(frames[g[:2]][0], frames[g[:2]][1], g[2], 16)[0] for g in set(order)}
    for W, H, B in order:
        fr = frames[(W, H)]
        np.testing.assert_array_equal(ctx.sad_flow(fr[0], fr[1], B, 16).view(np.uint32), expect[(W, H, B)].view(np.uint32))
    for W, H, B in order:
        ent, _ = _dev_run(ctx, frames[(W, H)], (W + 63) // 64 * 64, 0, B, 16, False)
        np.testing.assert_array_equal(ent[0].view(np.uint32), expect[(W, H, B)].view(np.uint32))


def test_a_larger_batch_behind_a_smaller_one_and_scratch_alternating_with_a_caller_buffer(ctx):
    fr = _frames(256, 144, 16, "pan", n=6)
    want = [_expect(fr[k], fr[k + 1], 16, 16) for k in range(5)]
    for n, with_best in ((2, False), (6, False), (2, False), (6, True), (3, False), (6, True), (6, False)):
        ent, best = _dev_run(ctx, fr[:n], 256, 0, 16, 16, with_best)
        for k in range(n - 1):
            np.testing.assert_array_equal(ent[k].view(np.uint32), want[k][0].view(np.uint32), err_msg=f"n={n} with_best={with_best} pair {k}")
            if with_best:
                np.testing.assert_array_equal(best[k], want[k][1])


def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    for name in ("a", "b", "c"):
        W, H, B, R = (int(v) for v in g[f"{name}_geom"])
        fr = g[f"{name}_frames"]
        ent_g, best_g = ctx.sad_flow(fr[0], fr[1], B, R, want_best=True)
        _same(ent_g, best_g, g[f"{name}_entries"], g[f"{name}_best"])


def test_scale_four_one_four_on_one_context(ctx):
    fr = _frames(640, 360, 16, "pan")
    ent_q, best_q, _ = _expect(fr[0], fr[1], 16, 16)
    ent_i, best_i = oracle.sad_flow(fr[0], fr[1], 16, 16)
    assert ctx.get_sad_motion_scale() == 4
    _same(*ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True), ent_q, best_q)
    ctx.set_sad_motion_scale(1)
    assert ctx.get_sad_motion_scale() == 1
    _same(*ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True), ent_i, best_i)       # today's bytes
    ctx.set_sad_motion_scale(4)
    _same(*ctx.sad_flow(fr[0], fr[1], 16, 16, want_best=True), ent_q, best_q)


def test_default_scale_is_one_and_an_invalid_scale_is_einval():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    try:
        assert c.get_sad_motion_scale() == 1
        for bad in (0, 2, 3, 8, -4):
            assert _lib.load().ofps_hip_set_sad_motion_scale(c._h, bad) == OFPS_HIP_EINVAL
            with pytest.raises(OfpsHipError):
                c.set_sad_motion_scale(bad)
            assert c.get_sad_motion_scale() == 1
        c.set_option("OFPS_HIP_SAD_MOTION_SCALE", 4)                               # the option table sets the same field
        assert c.get_sad_motion_scale() == 4
        with pytest.raises(OfpsHipError):
            c.set_option("OFPS_HIP_SAD_MOTION_SCALE", 2)
        c.set_option("OFPS_HIP_SAD_MOTION_SCALE", None)
        assert c.get_sad_motion_scale() == 1
    finally:
        c.close()


def test_python_decoder_flips_quarter_pel_mid_stream():
    from ofps_amd.plugins import HipSadDecoder
    fr = _frames(320, 192, 16, "pan", n=5)
    dec = HipSadDecoder(list(fr))
    assert ("Quarter pel", "bool", False, None, None) in dec.props()
    flips = {0: False, 2: True, 3: False, 4: True}                                 # value while frame k is processed
    on = False
    for k in range(5):
        if k in flips:
            assert dec.set_prop("Quarter pel", flips[k])
            on = flips[k]
        field = []
        assert dec.process_frame(field) == (k > 0)
        if k:
            want = _expect(fr[k - 1], fr[k], 16, 16)[0] if on else oracle.sad_flow(fr[k - 1], fr[k], 16, 16)[0]
            np.testing.assert_array_equal(np.array(field, np.float32).view(np.uint32), want.view(np.uint32))
    dec.ctx.close()


def test_cpp_host_flips_quarter_pel_mid_stream(tmp_path):
    W, H, F = 320, 192, 5
    fr = _frames(W, H, 16, "pan", n=F)
    raw = tmp_path / "clip.y"
    raw.write_bytes(fr.tobytes())
    out = tmp_path / "clip.mvec"
    p = subprocess.run([TOOL, "extract", "hip_sad", f"{raw}?w={W}&h={H}&fps=30", str(out), str(F), "Quarter pel=true@2", "Quarter pel=false@3",
                        "Quarter pel=true@4"], check=True, capture_output=True, text=True)
    assert json.loads(p.stdout)["frames"] == F
    frames = list(mvec.read_frames(open(out, "rb")))
    assert len(frames[0]) == 0
    for k, on in ((1, False), (2, True), (3, False), (4, True)):
        want = _expect(fr[k - 1], fr[k], 16, 16)[0] if on else oracle.sad_flow(fr[k - 1], fr[k], 16, 16)[0]
        np.testing.assert_array_equal(frames[k].view(np.uint32), want.view(np.uint32))
