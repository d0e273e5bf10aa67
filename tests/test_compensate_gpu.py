"""-m gpu: the compensation stage (ofps_hip_compensate[_dev]) against the oracle chain of tests/compensate_cases.py, bit for bit, and the
compensated detector of the fused per-frame entry points (ofps_hip_set_detect_compensation(ctx, 1)): hip_sad in its sync, async and
batched forms, the dense decoders' tail.  In mode 1 a ticket's vectors and quaternion are mode 0's bit for bit, its detector result is
ofps_hip_detect(ofps_hip_compensate(out_entries, quat)) bit for bit -- and its area is NOT mode 0's: the assertion that fails without the
feature.  tests/test_compensate_cpu.py proves on the oracle that the inputs separate the two."""
import numpy as np
import pytest

import compensate_cases as cc
import dense_fused_cases as fc
import oracle

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1, 0, 0, 0], np.float32)
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the stage on its own
@pytest.mark.parametrize("n", cc.RECORD_COUNTS)
def test_compensate_record_counts_bit_for_bit(ctx, n):
    """pos: the input's bits; motion: the oracle chain's bits with the same quaternion bits -- at every count, 70,000 included (no fast
    regime above the estimator's 65,536 switch)"""
    kinds = ("planted", "random") if n == len(cc.planted_field()) else ("random",)
    for kind in kinds:
        e, q, want = cc.expected_case(kind, n, seed=n % 97)
        got = ctx.compensate(e, *cc.CAM, q)
        assert got.shape == (n, 4)
        np.testing.assert_array_equal(_bits(got[:, :2]), _bits(e[:, :2]), err_msg=f"{kind} n={n}: pos")
        diff = np.abs(_bits(got[:, 2:]).astype(np.int64) - _bits(want[:, 2:]).astype(np.int64))
        print(f"{kind} n={n}: motion words that differ from the oracle: {int((diff != 0).sum())}, worst {int(diff.max()) if n else 0} ulp")
        np.testing.assert_array_equal(_bits(got[:, 2:]), _bits(want[:, 2:]), err_msg=f"{kind} n={n}: motion")
    if n:                                                # the result does not depend on the record count: the first record alone
        one = ctx.compensate(e[:1], *cc.CAM, q)
        np.testing.assert_array_equal(_bits(one), _bits(got[:1]))


def test_compensate_dev_batch_in_place_and_behind_the_estimator(ctx):
    import torch
    n = len(cc.planted_field())
    items = [cc.expected_case("planted", n, 1), cc.expected_case("random", n, 2), cc.expected_case("random", n, 3)]
    ent = np.stack([it[0] for it in items])
    d_ent = torch.from_numpy(ent.copy()).cuda()
    d_q = torch.from_numpy(np.stack([it[1] for it in items])).cuda()          # three different quaternions, in device memory
    d_out = torch.zeros_like(d_ent)
    torch.cuda.synchronize()
    ctx.compensate_dev(d_ent.data_ptr(), n, 3, *cc.CAM, d_q.data_ptr(), d_out.data_ptr())
    ctx.sync()
    out = d_out.cpu().numpy()
    for b, it in enumerate(items):
        np.testing.assert_array_equal(_bits(out[b]), _bits(it[2]), err_msg=f"item {b}")
    np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()), _bits(ent))      # out of place: the input is untouched
    d_in_place = d_ent.clone()
    torch.cuda.synchronize()
    ctx.compensate_dev(d_in_place.data_ptr(), n, 3, *cc.CAM, d_q.data_ptr(), d_in_place.data_ptr())
    ctx.sync()
    np.testing.assert_array_equal(_bits(d_in_place.cpu().numpy()), _bits(out))
    # the estimator's quaternions consumed where it left them: almeida_dev -> compensate_dev, nothing in between
    for use_ransac in (False, True):
        d_fit = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
        d_res = torch.zeros_like(d_ent)
        torch.cuda.synchronize()
        ctx.almeida_dev(d_ent.data_ptr(), n, 3, *cc.CAM, use_ransac, cc.RANSAC["num_iters"], cc.RANSAC["inlier_deg"], cc.RANSAC["num_samples"],
                        cc.SEED, d_fit.data_ptr())
        ctx.compensate_dev(d_ent.data_ptr(), n, 3, *cc.CAM, d_fit.data_ptr(), d_res.data_ptr())
        ctx.sync()
        fit, res = d_fit.cpu().numpy(), d_res.cpu().numpy()
        assert fc.off_identity(fit[0]) > 1e-3                                  # the planted rotation, not an untouched buffer
        for b in range(3):
            np.testing.assert_array_equal(_bits(res[b]), _bits(ctx.compensate(ent[b], *cc.CAM, fit[b])), err_msg=f"ransac={use_ransac} item {b}")
    # batch >= 1, n == 0
    ctx.compensate_dev(0, 0, 2, *cc.CAM, d_q.data_ptr(), 0)
    ctx.sync()
    assert ctx.compensate(np.zeros((0, 4), np.float32), *cc.CAM, IDENTITY).shape == (0, 4)


def test_planted_field_on_the_device(ctx):
    """the chain a user runs by hand: estimate, compensate, detect -- the raw field is one island, the compensated one the planted island"""
    e = cc.planted_field()
    for use_ransac in (True, False):
        q, _ = ctx.almeida(e, *cc.CAM, use_ransac=use_ransac, seed=cc.SEED, **cc.RANSAC)
        raw = ctx.detect(e, **cc.DETECTOR)
        comp = ctx.detect(ctx.compensate(e, *cc.CAM, q), **cc.DETECTOR)
        print(f"ransac={use_ransac}: quat {q}, raw area {cc.area_of(raw)}, compensated area {cc.area_of(comp)}")
        assert raw is not None and raw[0] >= 0.9 * cc.CELLS
        assert comp is not None and 1 <= comp[0] <= 0.25 * cc.CELLS


# ------------------------------------------------------------------------------------------------------------------- fused hip_sad forms
def _prm(use_ransac, seed, detector=True, estimator=True):
    return dict(block=cc.BLOCK, search_range=cc.RANGE, detector=detector, estimator=estimator, aspect=cc.FRAME_CAM[0], fov_y_deg=cc.FRAME_CAM[1],
                use_ransac=use_ransac, seed=seed, **cc.FRAME_DETECTOR, **cc.FRAME_RANSAC)


def _sync_stream(ctx, use_ransac, detector=True, estimator=True):
    ctx.reset_frames()
    f = cc.frames()
    out = []
    for k in range(cc.STREAM_FRAMES):
        r = ctx.push_frame(f[k], want_entries=True, want_field=True, **_prm(use_ransac, cc.SEED + k, detector, estimator))
        out.append(dict(have=r["have_vectors"], entries=r["entries"], quat=r["quat"], motion=r["motion"]))
    return out


def _async_stream(ctx, use_ransac, modes=None):
    """two tickets in flight; modes[k]: the context's mode when frame k is pushed (None: leave it alone)"""
    ctx.reset_frames()
    f = cc.frames()
    dim = ctx.block_dim(cc.FRAME_DETECTOR["min_size"], cc.FRAME_DETECTOR["subdivide"])
    pins = [ctx.pinned_frame(cc.FRAME_H, cc.FRAME_W) for _ in range(3)]
    ents = [ctx.pinned_array((240, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    out, tickets = [], []

    def collect(k):
        r = ctx.frame_wait(tickets[k])
        m = None if r["motion"] is None else (r["motion"][0], flds[k % 2].copy())
        out.append(dict(have=r["have_vectors"], entries=ents[k % 2].copy() if r["have_vectors"] else None, quat=r["quat"], motion=m))

    for k in range(cc.STREAM_FRAMES):
        if k >= 2:
            collect(k - 2)
        if modes is not None:
            ctx.set_detect_compensation(modes[k])
        np.copyto(pins[k % 3], f[k])
        tickets.append(ctx.push_frame_async(pins[k % 3], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(use_ransac, cc.SEED + k)))
    collect(cc.STREAM_FRAMES - 2)
    collect(cc.STREAM_FRAMES - 1)
    for p in pins + ents + flds:
        ctx.free_pinned(p)
    return out


def _batched_stream(ctx, use_ransac):
    """n = 3 frames per ticket, two tickets in flight -> one dict per frame (the batched form hands back no field: area and dim only)"""
    ctx.reset_frames()
    f = cc.frames()
    bufs = [ctx.pinned_array((3, cc.FRAME_H, cc.FRAME_W), np.uint8) for _ in range(2)]
    ents = [ctx.pinned_array((3, 240, 4)) for _ in range(2)]
    tickets = []
    for t in range(2):
        np.copyto(bufs[t], f[3 * t:3 * t + 3])
        tickets.append(ctx.push_frames_async(bufs[t], out_entries=ents[t], **_prm(use_ransac, cc.SEED + 3 * t)))
    out = []
    for t in range(2):
        for j, r in enumerate(ctx.frames_wait(tickets[t])):
            out.append(dict(have=r["have_vectors"], entries=ents[t][j].copy() if r["have_vectors"] else None, quat=r["quat"], motion=r["motion"]))
    for p in bufs + ents:
        ctx.free_pinned(p)
    return out


def _same_motion(a, b, what, with_field=True):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a[0] == b[0], what
        if with_field:
            np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what + ": field")


def _check_compensated(ctx, ref, got, what, batched=False):
    """ref: the mode-0 stream, got: the mode-1 stream"""
    assert not got[0]["have"] and got[0]["motion"] is None
    np.testing.assert_array_equal(got[0]["quat"], IDENTITY)
    for k in range(1, len(got)):
        w = f"{what} frame {k}"
        assert got[k]["have"] and ref[k]["have"], w
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(ref[k]["entries"]), err_msg=w + ": vectors")
        np.testing.assert_array_equal(_bits(got[k]["quat"]), _bits(ref[k]["quat"]), err_msg=w + ": quaternion")
        want = ctx.detect(ctx.compensate(got[k]["entries"], *cc.FRAME_CAM, got[k]["quat"]), **cc.FRAME_DETECTOR)
        a1, a0 = cc.area_of(got[k]["motion"]), cc.area_of(ref[k]["motion"])
        print(f"{w}: quat {got[k]['quat']}, area mode 0 {a0}, mode 1 {a1}, detect(compensate) {cc.area_of(want)}")
        if batched:
            dim = ctx.block_dim(cc.FRAME_DETECTOR["min_size"], cc.FRAME_DETECTOR["subdivide"])
            assert got[k]["motion"] == (None if want is None else (want[0], dim)), w
        else:
            _same_motion(got[k]["motion"], want, w)
        assert a1 != a0, w + ": the compensated detector answered like the raw one"
        assert a0 >= 0.9 * cc.FRAME_CELLS and 1 <= a1 <= 0.25 * cc.FRAME_CELLS, w         # what the oracle shows on these frames (CPU test)


@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
@pytest.mark.parametrize("form", ["sync", "async", "batched"])
def test_fused_hip_sad_compensated_detector(ctx, form, use_ransac):
    run = {"sync": _sync_stream, "async": _async_stream, "batched": _batched_stream}[form]
    assert ctx.get_detect_compensation() == 0
    ref = run(ctx, use_ransac)
    ctx.set_detect_compensation(1)
    try:
        assert ctx.get_detect_compensation() == 1
        got = run(ctx, use_ransac)
    finally:
        ctx.set_detect_compensation(0)
    assert len(got) == (6 if form == "batched" else cc.STREAM_FRAMES)
    _check_compensated(ctx, ref, got, f"{form} ransac={use_ransac}", batched=form == "batched")


def test_one_stage_off_and_mode_0_after_mode_1(ctx):
    from ofps_amd.runtime import HipContext
    fresh = HipContext(0)
    try:
        ref = _sync_stream(fresh, False)                                   # a context that never saw mode 1
        ref_det_only = _sync_stream(fresh, False, estimator=False)
        ref_est_only = _sync_stream(fresh, False, detector=False)
    finally:
        fresh.close()
    ctx.set_detect_compensation(1)
    try:
        det_only = _sync_stream(ctx, False, estimator=False)               # estimator not run: the raw detector, no error
        est_only = _sync_stream(ctx, False, detector=False)
    finally:
        ctx.set_detect_compensation(0)
    again = _sync_stream(ctx, False)                                       # mode 0 after mode 1: a fresh context's bytes
    for k in range(1, cc.STREAM_FRAMES):
        for got, want, w in ((det_only, ref_det_only, "detector only"), (est_only, ref_est_only, "estimator only"), (again, ref, "mode 0 again")):
            np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(want[k]["entries"]), err_msg=w)
            np.testing.assert_array_equal(_bits(got[k]["quat"]), _bits(want[k]["quat"]), err_msg=w)
            _same_motion(got[k]["motion"], want[k]["motion"], f"{w} frame {k}")
        np.testing.assert_array_equal(det_only[k]["quat"], IDENTITY)
        assert det_only[k]["motion"] is not None and det_only[k]["motion"][0] == ref[k]["motion"][0]       # the raw island
        assert est_only[k]["motion"] is None
        np.testing.assert_array_equal(_bits(est_only[k]["quat"]), _bits(ref[k]["quat"]))


def test_mode_switch_between_tickets(ctx):
    """frames 0, 1 pushed in mode 1, frame 2 in mode 0, frame 3 in mode 1 again, two tickets in flight: each ticket follows the mode at its push"""
    ref0 = _async_stream(ctx, False)
    try:
        ref1 = _async_stream(ctx, False, modes=[1, 1, 1, 1])
        got = _async_stream(ctx, False, modes=[1, 1, 0, 1])
    finally:
        ctx.set_detect_compensation(0)
    for k, want in ((1, ref1), (2, ref0), (3, ref1)):
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(ref0[k]["entries"]))
        np.testing.assert_array_equal(_bits(got[k]["quat"]), _bits(ref0[k]["quat"]))
        _same_motion(got[k]["motion"], want[k]["motion"], f"frame {k}")
    assert cc.area_of(got[2]["motion"]) != cc.area_of(ref1[2]["motion"])


def test_bad_mode_values_and_the_option(ctx):
    from ofps_amd import _lib
    from ofps_amd.runtime import OfpsHipError
    assert ctx.get_detect_compensation() == 0
    for bad in (2, -1):
        assert _lib.load().ofps_hip_set_detect_compensation(ctx._h, bad) == EINVAL
        assert ctx.get_detect_compensation() == 0
    ctx.set_option("OFPS_HIP_DETECT_COMPENSATE", 1)                         # the option table sets the same field
    assert ctx.get_detect_compensation() == 1
    with pytest.raises(OfpsHipError) as ei:
        ctx.set_option("OFPS_HIP_DETECT_COMPENSATE", 2)
    assert ei.value.code == EINVAL and ctx.get_detect_compensation() == 1
    ctx.set_option("OFPS_HIP_DETECT_COMPENSATE", None)
    assert ctx.get_detect_compensation() == 0


# ------------------------------------------------------------------------------------------------------------------- the dense decoders' tail
def _dense_kw(cap, farneback):
    p = fc.FB if farneback else fc.LK
    return dict(levels=p[0], radius=p[1], iters=p[2], max_w=cap[0], max_h=cap[1], contrast_mask=True, reduced=True, farneback=farneback,
                fmt=oracle.FMT_BGR)


def _dense_tail(use_ransac, detector=True, estimator=True):
    return dict(detector=detector, estimator=estimator, aspect=fc.CAM[0], fov_y_deg=fc.CAM[1], use_ransac=use_ransac, num_iters=fc.RANSAC_ITERS,
                inlier_deg=fc.INLIER_DEG, num_samples=300, seed=fc.SEED, **fc.DETECTOR)


def _dense_stream(ctx, kinds, kw, tail):
    ctx.lk_reset()
    out = [ctx.lk_push_frame_fused(fc.bgr_of(fc.frame(k)), **kw, **tail) for k in kinds]
    ctx.lk_reset()
    return out


# (150, 150): the reduced mode's smallest capacity, 12,600 records; (300, 300): 50,400.  Both lie above 8,192 records, where the estimator in
# front of the compensation launch is the cluster solver with the count on the device.
@pytest.mark.parametrize("cap", [(150, 150), (300, 300)])
@pytest.mark.parametrize("decoder", ["hip_lk", "hip_flow"])
def test_fused_dense_compensated_detector(ctx, decoder, cap):
    kw = _dense_kw(cap, decoder == "hip_flow")
    for use_ransac in (False, True):
        tail = _dense_tail(use_ransac)
        ref = _dense_stream(ctx, fc.MOVE, kw, tail)
        ctx.set_detect_compensation(1)
        try:
            got = _dense_stream(ctx, fc.MOVE, kw, tail)
        finally:
            ctx.set_detect_compensation(0)
        assert not got[0]["have_vectors"]
        for k in (1, 2):
            w = f"{decoder} cap {cap} ransac={use_ransac} frame {k}"
            assert got[k]["have_vectors"] and got[k]["n_vectors"] == ref[k]["n_vectors"] > 0, w
            np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(ref[k]["entries"]), err_msg=w + ": records")
            np.testing.assert_array_equal(_bits(got[k]["quat"]), _bits(ref[k]["quat"]), err_msg=w + ": quaternion")
            want = ctx.detect(ctx.compensate(got[k]["entries"], *fc.CAM, got[k]["quat"]), **fc.DETECTOR)
            a1, a0 = cc.area_of(got[k]["motion"]), cc.area_of(ref[k]["motion"])
            print(f"{w}: n {got[k]['n_vectors']}, quat {got[k]['quat']}, area mode 0 {a0}, mode 1 {a1}, detect(compensate) {cc.area_of(want)}")
            _same_motion(got[k]["motion"], want, w)
            assert a1 != a0, w + ": the compensated detector answered like the raw one"


def test_fused_dense_flat_frame_and_one_stage_off(ctx):
    kw = _dense_kw((150, 150), False)
    ctx.set_detect_compensation(1)
    try:
        got = _dense_stream(ctx, ("move0", "flat"), kw, _dense_tail(False))            # *d_n == 0: no motion, identity
        det_only = _dense_stream(ctx, fc.MOVE[:2], kw, _dense_tail(False, estimator=False))
    finally:
        ctx.set_detect_compensation(0)
    assert got[1]["have_vectors"] and got[1]["n_vectors"] == 0 and got[1]["motion"] is None
    np.testing.assert_array_equal(got[1]["quat"], IDENTITY)
    ref = _dense_stream(ctx, fc.MOVE[:2], kw, _dense_tail(False, estimator=False))
    np.testing.assert_array_equal(_bits(det_only[1]["entries"]), _bits(ref[1]["entries"]))
    np.testing.assert_array_equal(det_only[1]["quat"], IDENTITY)
    _same_motion(det_only[1]["motion"], ref[1]["motion"], "dense, estimator not run: the raw detector")
