"""-m gpu: hip_sad's contrast gate (include/ofps_hip.h N1g) against the restatement of tests/sad_gate_cases.py.  Counts, flags, records
and winners are integers or copies: every equality is bit for bit.  The one exception is the least-squares / RANSAC quaternion of the
fused path's device-count form, held to the solver's existing parity bound (2e-6, include/ofps_hip.h: the dense decoders' fused form).
tests/test_sad_gate_cpu.py proves on the oracle that the inputs separate gate-on from gate-off."""
import numpy as np
import pytest

import sad_gate_cases as gc

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1, 0, 0, 0], np.float32)
EINVAL = -1
QUAT_BOUND = 2e-6


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(f, stride):
    buf = np.zeros((f.shape[0], stride), np.uint8)
    buf[:, :f.shape[1]] = f
    buf[:, f.shape[1]:] = 255                            # whatever lies in the padding must not be read as luma
    return buf[:, :f.shape[1]]


def _check_counts(ctx, W, H, stride, block):
    for kind in gc.CONTENTS:
        f = gc.content(kind, W, H)
        want = gc.block_counts(f, block)
        got = ctx.block_contrast(f, block) if stride == W else ctx.block_contrast(_padded(f, stride), block, stride=stride)
        w = f"{kind} {W}x{H} stride {stride} block {block}"
        assert got.shape == want.shape and got.dtype == np.uint32, w
        np.testing.assert_array_equal(got, want, err_msg=w + ": against the restatement")
        m = ctx.contrast_mask(f)
        nby, nbx = H // block, W // block
        sums = m[:nby * block, :nbx * block].reshape(nby, block, nbx, block).sum(axis=(1, 3), dtype=np.uint32)
        np.testing.assert_array_equal(got, sums, err_msg=w + ": against the sums of ofps_hip_contrast_mask's output")


# --------------------------------------------------------------------------------------------------------------- the count kernel
@pytest.mark.parametrize("block", gc.LATTICE_BLOCKS)
@pytest.mark.parametrize("size", gc.FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}s{s[2]}")
def test_block_contrast_one_writer_path(ctx, size, block):
    _check_counts(ctx, *size, block)


def test_block_contrast_atomic_path(ctx):
    W, H, stride, block = gc.GENERIC
    _check_counts(ctx, W, H, stride, block)
    _check_counts(ctx, W, H, stride, block)              # a second call starts from a zeroed buffer again


def test_block_contrast_dev(ctx):
    import torch
    W, H, stride, block = 80, 48, 96, 16
    f = gc.content("half_flat", W, H)
    buf = np.zeros((H, stride), np.uint8)
    buf[:, :W] = f
    d = torch.from_numpy(buf).cuda()
    out = torch.full(((H // block) * (W // block),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.block_contrast_dev(d.data_ptr(), W, H, stride, block, out.data_ptr())
    ctx.sync()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(H // block, W // block), gc.block_counts(f, block))


# --------------------------------------------------------------------------------------------------------------- compaction, thresholds
def _gated_sad(ctx, prev, cur, block, gate):
    ctx.set_sad_gate(gate)
    try:
        return ctx.sad_flow(prev, cur, block, gc.PAIR_RANGE, want_best=True)
    finally:
        ctx.set_sad_gate(0)


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("block", gc.LATTICE_BLOCKS)
def test_gated_sad_flow_is_the_filtered_ungated_output(ctx, block, scale):
    prev, cur = gc.half_flat_pair()
    ctx.set_sad_motion_scale(scale)
    try:
        ent0, best0 = ctx.sad_flow(prev, cur, block, gc.PAIR_RANGE, want_best=True)
        assert len(ent0) == (gc.PAIR_W // block) * (gc.PAIR_H // block)
        for mp in (1, block * block // 2, block * block):
            keep = gc.keep_flags(cur, block, mp)
            ent, best = _gated_sad(ctx, prev, cur, block, mp)
            w = f"block {block} scale {scale} min_pixels {mp}"
            assert len(ent) == len(best) == int(keep.sum()) < len(ent0), w
            np.testing.assert_array_equal(_bits(ent), _bits(gc.gate_filter(ent0, keep)), err_msg=w + ": records")
            np.testing.assert_array_equal(best, gc.gate_filter(best0, keep), err_msg=w + ": out_best")
        # all kept / none kept
        noise = gc.content("noise", gc.PAIR_W, gc.PAIR_H)
        e_all0 = ctx.sad_flow(prev, noise, block, gc.PAIR_RANGE)
        e_all, _ = _gated_sad(ctx, prev, noise, block, block * block)
        np.testing.assert_array_equal(_bits(e_all), _bits(e_all0))
        e_none, b_none = _gated_sad(ctx, prev, gc.content("constant", gc.PAIR_W, gc.PAIR_H), block, 1)
        assert e_none.shape == (0, 4) and b_none.shape == (0, 3)          # n_out == 0 is valid, no error
    finally:
        ctx.set_sad_motion_scale(1)


@pytest.mark.parametrize("scale", [1, 4])
def test_gated_dev_form_matches_the_host_form(ctx, scale):
    import torch
    prev, cur = gc.half_flat_pair()
    block, mp = 16, 128
    nblk = (gc.PAIR_W // block) * (gc.PAIR_H // block)
    ctx.set_sad_motion_scale(scale)
    try:
        ent_h, best_h = _gated_sad(ctx, prev, cur, block, mp)
        d_prev, d_cur = torch.from_numpy(prev.copy()).cuda(), torch.from_numpy(cur.copy()).cuda()
        d_ent = torch.zeros((nblk, 4), dtype=torch.float32, device="cuda")
        d_best = torch.zeros((nblk, 3), dtype=torch.int32, device="cuda")
        d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ctx.get_sad_gate() == 0                   # the device form takes its own min_pixels
        ctx.sad_flow_gated_dev(d_prev.data_ptr(), d_cur.data_ptr(), gc.PAIR_W, gc.PAIR_H, gc.PAIR_W, block, gc.PAIR_RANGE, mp, d_ent.data_ptr(),
                               d_best.data_ptr(), d_cnt.data_ptr())
        ctx.sync()
        n = int(d_cnt.cpu().numpy()[0])
        assert n == len(ent_h) == int(gc.keep_flags(cur, block, mp).sum())
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()[:n]), _bits(ent_h))
        np.testing.assert_array_equal(d_best.cpu().numpy()[:n], best_h)
        d_cnt.fill_(-1)
        torch.cuda.synchronize()
        ctx.sad_flow_gated_dev(d_prev.data_ptr(), d_cur.data_ptr(), gc.PAIR_W, gc.PAIR_H, gc.PAIR_W, block, gc.PAIR_RANGE, mp, d_ent.data_ptr(),
                               None, d_cnt.data_ptr())   # without out_best
        ctx.sync()
        assert int(d_cnt.cpu().numpy()[0]) == n
    finally:
        ctx.set_sad_motion_scale(1)


# --------------------------------------------------------------------------------------------------------------- the fused path
def _prm(use_ransac, seed, detector=True, estimator=True):
    return dict(block=gc.BLOCK, search_range=gc.RANGE, detector=detector, estimator=estimator, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1],
                use_ransac=use_ransac, seed=seed, **gc.FRAME_DETECTOR, **gc.FRAME_RANSAC)


def _sync_stream(ctx, use_ransac, frames=None, detector=True, estimator=True, gates=None):
    ctx.reset_frames()
    f = gc.frames() if frames is None else frames
    out = []
    for k in range(len(f)):
        if gates is not None:
            ctx.set_sad_gate(gates[k])
        r = ctx.push_frame(f[k], want_entries=True, want_field=True, **_prm(use_ransac, gc.SEED + k, detector, estimator))
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=r["entries"], quat=r["quat"], motion=r["motion"]))
    return out


def _async_stream(ctx, use_ransac, gates=None):
    """two tickets in flight; gates[k]: the context's gate when frame k is pushed (None: leave it alone)"""
    ctx.reset_frames()
    f = gc.frames()
    dim = ctx.block_dim(gc.FRAME_DETECTOR["min_size"], gc.FRAME_DETECTOR["subdivide"])
    pins = [ctx.pinned_frame(gc.FRAME_H, gc.FRAME_W) for _ in range(3)]
    ents = [ctx.pinned_array((gc.NBLK, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    out, tickets = [], []

    def collect(k):
        r = ctx.frame_wait(tickets[k])
        m = None if r["motion"] is None else (r["motion"][0], flds[k % 2].copy())
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=ents[k % 2][:r["n_vectors"]].copy() if r["have_vectors"] else None,
                        quat=r["quat"], motion=m))

    for k in range(gc.N_FRAMES):
        if k >= 2:
            collect(k - 2)
        if gates is not None:
            ctx.set_sad_gate(gates[k])
        np.copyto(pins[k % 3], f[k])
        tickets.append(ctx.push_frame_async(pins[k % 3], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(use_ransac, gc.SEED + k)))
    collect(gc.N_FRAMES - 2)
    collect(gc.N_FRAMES - 1)
    for p in pins + ents + flds:
        ctx.free_pinned(p)
    return out


def _same_motion(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a[0] == b[0], what
        np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what + ": field")


def _check_gated(ctx, ref, got, use_ransac, comp, what, gated_frames=None):
    """ref: the gate-0 stream, got: the gated one"""
    assert not got[0]["have"] and got[0]["motion"] is None
    np.testing.assert_array_equal(got[0]["quat"], IDENTITY)
    for k in range(1, len(got)):
        if gated_frames is not None and k not in gated_frames:
            continue
        w = f"{what} frame {k}"
        keep = gc.frame_keep(k)
        assert got[k]["have"] and got[k]["n"] == int(keep.sum()) == len(got[k]["entries"]), w
        assert ref[k]["n"] == gc.NBLK, w
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(gc.gate_filter(ref[k]["entries"], keep)), err_msg=w + ": records")
        q = ctx.almeida(got[k]["entries"], *gc.FRAME_CAM, use_ransac=use_ransac, seed=gc.SEED + k, **gc.FRAME_RANSAC)[0]
        err = float(np.abs(got[k]["quat"] - q).max())
        det_in = ctx.compensate(got[k]["entries"], *gc.FRAME_CAM, got[k]["quat"]) if comp else got[k]["entries"]
        want = ctx.detect(det_in, **gc.FRAME_DETECTOR)
        a1, a0 = gc.area_of(got[k]["motion"]), gc.area_of(ref[k]["motion"])
        print(f"{w}: kept {got[k]['n']}, quat {got[k]['quat']} (|fused - almeida| {err:.3g}), area gate 0 {a0}, gated {a1}, detect {gc.area_of(want)}")
        assert err <= QUAT_BOUND, w
        assert np.isfinite(got[k]["quat"]).all(), w
        _same_motion(got[k]["motion"], want, w)
        if not use_ransac:
            assert np.abs(got[k]["quat"] - ref[k]["quat"]).max() > 1e-4, w + ": the estimator answered as without the gate"


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
@pytest.mark.parametrize("form", ["sync", "async"])
def test_fused_gated_stream(ctx, form, use_ransac, comp):
    run = {"sync": _sync_stream, "async": _async_stream}[form]
    assert ctx.get_sad_gate() == 0
    ctx.set_detect_compensation(comp)
    try:
        ref = run(ctx, use_ransac)
        ctx.set_sad_gate(gc.GATE)
        assert ctx.get_sad_gate() == gc.GATE
        got = run(ctx, use_ransac)
    finally:
        ctx.set_sad_gate(0)
        ctx.set_detect_compensation(0)
    assert len(got) == gc.N_FRAMES
    _check_gated(ctx, ref, got, use_ransac, comp, f"{form} ransac={use_ransac} comp={comp}")
    if not comp:                                         # the raw detector: the flat side's noise vectors are gone from the island
        for k in range(1, gc.N_FRAMES):
            assert gc.area_of(got[k]["motion"]) != gc.area_of(ref[k]["motion"]), f"frame {k}: the detector answered as without the gate"


@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
def test_fused_flat_frame_and_two_kept_blocks(ctx, use_ransac):
    f = gc.frames()
    try:
        ctx.set_sad_gate(gc.GATE)
        for comp in (0, 1):
            ctx.set_detect_compensation(comp)
            got = _sync_stream(ctx, use_ransac, frames=[f[0], gc.flat_frame()])
            assert got[1]["have"] and got[1]["n"] == 0 and got[1]["entries"].shape == (0, 4) and got[1]["motion"] is None, comp
            np.testing.assert_array_equal(got[1]["quat"], IDENTITY)
        ctx.set_sad_gate(gc.TWO_BLOCK_GATE)
        for comp in (0, 1):
            ctx.set_detect_compensation(comp)
            got = _sync_stream(ctx, use_ransac, frames=[f[0], gc.two_block_frame()])
            assert got[1]["have"] and got[1]["n"] == 2, comp
            np.testing.assert_array_equal(got[1]["quat"], IDENTITY)
    finally:
        ctx.set_sad_gate(0)
        ctx.set_detect_compensation(0)


def test_gate_switch_between_tickets_in_flight(ctx):
    """frames 0, 1 pushed with the gate on, frame 2 with it off, frame 3 with it on again, two tickets in flight"""
    try:
        ref0 = _async_stream(ctx, False, gates=[0, 0, 0, 0])
        ref1 = _async_stream(ctx, False, gates=[gc.GATE] * 4)
        got = _async_stream(ctx, False, gates=[gc.GATE, gc.GATE, 0, gc.GATE])
    finally:
        ctx.set_sad_gate(0)
    for k, want in ((1, ref1), (2, ref0), (3, ref1)):
        assert got[k]["n"] == want[k]["n"]
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(want[k]["entries"]))
        np.testing.assert_array_equal(_bits(got[k]["quat"]), _bits(want[k]["quat"]))
        _same_motion(got[k]["motion"], want[k]["motion"], f"frame {k}")
    assert got[2]["n"] == gc.NBLK and got[1]["n"] == got[3]["n"] < gc.NBLK


def test_gate_0_after_gate_n_equals_a_fresh_context_and_one_stage_off(ctx):
    from ofps_amd.runtime import HipContext
    fresh = HipContext(0)
    try:
        ref = _sync_stream(fresh, False)                                   # a context that never saw the gate
    finally:
        fresh.close()
    try:
        ctx.set_sad_gate(gc.GATE)
        gated = _sync_stream(ctx, False)
        det_only = _sync_stream(ctx, False, estimator=False)
        est_only = _sync_stream(ctx, False, detector=False)
    finally:
        ctx.set_sad_gate(0)
    again = _sync_stream(ctx, False)
    for k in range(1, gc.N_FRAMES):
        assert again[k]["n"] == gc.NBLK
        np.testing.assert_array_equal(_bits(again[k]["entries"]), _bits(ref[k]["entries"]))
        np.testing.assert_array_equal(_bits(again[k]["quat"]), _bits(ref[k]["quat"]))
        _same_motion(again[k]["motion"], ref[k]["motion"], f"gate 0 again, frame {k}")
        for got in (det_only, est_only):
            assert got[k]["n"] == gated[k]["n"]
            np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(gated[k]["entries"]))
        np.testing.assert_array_equal(det_only[k]["quat"], IDENTITY)
        _same_motion(det_only[k]["motion"], gated[k]["motion"], f"detector only, frame {k}")
        assert est_only[k]["motion"] is None
        np.testing.assert_array_equal(_bits(est_only[k]["quat"]), _bits(gated[k]["quat"]))


# --------------------------------------------------------------------------------------------------------------- errors, options, scope
def test_bad_gate_values_and_the_option(ctx):
    from ofps_amd import _lib
    from ofps_amd.runtime import OfpsHipError
    prev, cur = gc.half_flat_pair()
    assert ctx.get_sad_gate() == 0
    assert _lib.load().ofps_hip_set_sad_gate(ctx._h, -1) == EINVAL and ctx.get_sad_gate() == 0
    try:
        ctx.set_sad_gate(65)                             # fits block 16, not block 8: refused at the call
        assert len(ctx.sad_flow(prev, cur, 16, gc.PAIR_RANGE)) <= (gc.PAIR_W // 16) * (gc.PAIR_H // 16)
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow(prev, cur, 8, gc.PAIR_RANGE)
        assert ei.value.code == EINVAL
        ctx.reset_frames()
        ctx.push_frame(gc.frames()[0], **_prm(False, 0))
        ctx.set_sad_gate(257)
        with pytest.raises(OfpsHipError) as ei:
            ctx.push_frame(gc.frames()[1], **_prm(False, 0))
        assert ei.value.code == EINVAL
    finally:
        ctx.set_sad_gate(0)
        ctx.reset_frames()
    ctx.set_option("OFPS_HIP_SAD_GATE", 7)               # the option table sets the same field
    assert ctx.get_sad_gate() == 7
    with pytest.raises(OfpsHipError) as ei:
        ctx.set_option("OFPS_HIP_SAD_GATE", -3)
    assert ei.value.code == EINVAL and ctx.get_sad_gate() == 7
    ctx.set_option("OFPS_HIP_SAD_GATE", None)
    assert ctx.get_sad_gate() == 0


def test_batched_and_multi_forms_ignore_the_gate(ctx, monkeypatch):
    import torch
    from ofps_amd.runtime import MultiDevice
    f = gc.frames()
    try:
        ctx.set_sad_gate(gc.GATE)
        ctx.reset_frames()
        buf = ctx.pinned_array((3, gc.FRAME_H, gc.FRAME_W), np.uint8)
        ents = ctx.pinned_array((3, gc.NBLK, 4))
        np.copyto(buf, f[:3])
        res = ctx.frames_wait(ctx.push_frames_async(buf, out_entries=ents, **_prm(False, gc.SEED)))
        assert [r["n_vectors"] for r in res] == [0, gc.NBLK, gc.NBLK]
        np.testing.assert_array_equal(_bits(ents[1]), _bits(gc.frame_vectors(1)[0]))
        ctx.free_pinned(buf); ctx.free_pinned(ents)
        d = torch.from_numpy(f[:2].copy()).cuda()
        d_ent = torch.zeros((gc.NBLK, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.sad_flow_dev(d.data_ptr(), 2, gc.FRAME_W, gc.FRAME_H, gc.FRAME_W, gc.FRAME_W * gc.FRAME_H, 0, gc.BLOCK, gc.RANGE, d_ent.data_ptr())
        ctx.sync()
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()), _bits(gc.frame_vectors(1)[0]))
    finally:
        ctx.set_sad_gate(0)
        ctx.reset_frames()
    monkeypatch.setenv("OFPS_HIP_SAD_GATE", str(gc.GATE))                  # the workers read the environment at their own init
    m = MultiDevice([0, 0])
    try:
        out = m.sad_flow(f[:3], gc.BLOCK, gc.RANGE)
        assert out.shape == (2, gc.NBLK, 4)
        for k in (1, 2):
            np.testing.assert_array_equal(_bits(out[k - 1]), _bits(gc.frame_vectors(k)[0]))
    finally:
        m.close()


def test_plugin_property(ctx):
    from ofps_amd.plugins import HipSadDecoder
    f = gc.frames()
    dec = HipSadDecoder(iter(f[:3]))
    try:
        assert ("Contrast gate", "usize", 0, 0, 256) in dec.props()
        assert dec.set_prop("Search range", gc.RANGE)      # the decoder's default is 16; the cases' oracle vectors are range 8
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True and len(field) == gc.NBLK
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(gc.frame_vectors(1)[0]))
        assert dec.set_prop("Contrast gate", gc.GATE)
        field = []
        assert dec.process_frame(field) is True
        keep = gc.frame_keep(2)
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(gc.gate_filter(gc.frame_vectors(2)[0], keep)))
    finally:
        dec.ctx.close()
