"""The dense decoders' fused form -- ofps_hip_lk_push_frame_fused[_async] / ofps_hip_lk_frame_fused_wait: frame -> records -> island +
quaternion in one ticket, the records and their data-dependent COUNT staying on the device -- against the stage-wise chain on the CPU oracle
(tests/dense_fused_cases.py) and against this build's own stage-wise calls on the records the fused call returned.  Bounds are the
project's: records and detector bit for bit, quaternion 2e-6 (least squares) / 1e-4 (RANSAC).  tests/test_dense_fused_cpu.py proves on the
CPU that the frames give the counts the cases are named for."""
import numpy as np
import pytest

import dense_fused_cases as fc
import oracle

pytestmark = pytest.mark.gpu
LSQ_ATOL, RANSAC_ATOL = 2e-6, 1e-4
IDENTITY = np.array([1, 0, 0, 0], np.float32)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tail(use_ransac=False, num_samples=1000, detector=True, estimator=True, detector_params=None):
    return dict(detector=detector, estimator=estimator, aspect=fc.CAM[0], fov_y_deg=fc.CAM[1], use_ransac=use_ransac,
                num_iters=fc.RANSAC_ITERS, inlier_deg=fc.INLIER_DEG, num_samples=num_samples, seed=fc.SEED, **(detector_params or fc.DETECTOR))


def _detector_of(tail):
    return {k: tail[k] for k in ("min_size", "subdivide", "target_motion")}


def _stream(ctx, frames, kw, tails, reset=True):
    """frames through lk_push_frame_fused_async, two tickets in flight, collected in order -> the result dicts (tails[k]: frame k's tail)"""
    pins = [ctx.pinned_array(frames[0].shape, np.uint8) for _ in range(3)]
    if reset:
        ctx.lk_reset()
    tickets, got = [], []
    for k, f in enumerate(frames):
        np.copyto(pins[k % 3], f)
        tickets.append(ctx.lk_push_frame_fused_async(pins[k % 3], **kw, **tails[k]))
        if k >= 1:
            got.append(ctx.lk_frame_fused_wait(tickets[k - 1]))
    got.append(ctx.lk_frame_fused_wait(tickets[-1]))
    for p in pins:
        ctx.free_pinned(p)
    return got


def _check(ctx, res, rec_o, grid_o, tail, what, stagewise=True):
    """one fused result against the oracle chain on the oracle's records, and against the build's own detect / almeida on the returned records"""
    assert res["have_vectors"] and res["grid"] == grid_o, what
    print(f"{what}: n = {res['n_vectors']} of {grid_o[0] * grid_o[1]} (oracle {len(rec_o)}), quat {res['quat']}")
    assert res["n_vectors"] == len(rec_o) == len(res["entries"]), what
    np.testing.assert_array_equal(_bits(res["entries"]), _bits(rec_o), err_msg=what + ": records")
    assert np.isfinite(res["quat"]).all(), what
    det_o, q_o = fc.expected(rec_o, tail["use_ransac"], tail["num_samples"], tail["seed"], _detector_of(tail), tail["inlier_deg"])
    print(f"   oracle island {None if det_o is None else det_o[0]}")
    if tail["detector"]:
        assert (res["motion"] is None) == (det_o is None), what
        if det_o is not None:
            assert res["motion"][0] == det_o[0], what
            np.testing.assert_array_equal(_bits(res["motion"][1]), _bits(det_o[1]), err_msg=what + ": island field")
    else:
        assert res["motion"] is None
    if tail["estimator"]:
        print(f"   oracle quat {q_o}, |diff| max {np.abs(res['quat'] - q_o).max():.3g}")
        np.testing.assert_allclose(res["quat"], q_o, atol=RANSAC_ATOL if tail["use_ransac"] else LSQ_ATOL, rtol=0, err_msg=what)
    else:
        np.testing.assert_array_equal(res["quat"], IDENTITY)
    if stagewise:
        ent = res["entries"].copy()
        if tail["detector"]:
            det = ctx.detect(ent, **_detector_of(tail))
            assert (det is None) == (res["motion"] is None), what
            if det is not None:
                assert det[0] == res["motion"][0]
                np.testing.assert_array_equal(_bits(det[1]), _bits(res["motion"][1]), err_msg=what + ": ctx.detect on the returned records")
        if tail["estimator"] and not tail["use_ransac"]:
            q, _ = ctx.almeida(ent, *fc.CAM, use_ransac=False)
            np.testing.assert_allclose(res["quat"], q, atol=LSQ_ATOL, rtol=0, err_msg=what + ": ctx.almeida on the returned records")


def _kw(cap, reduced, farneback=False, params=fc.LK, use_previous=False, fmt=0):
    return dict(levels=params[0], radius=params[1], iters=params[2], max_w=cap[0], max_h=cap[1], contrast_mask=True, reduced=reduced,
                farneback=farneback, use_previous=use_previous, fmt=fmt)


# ------------------------------------------------------------------------------------------- every solver class, the count on the device
@pytest.mark.parametrize("cap,reduced", fc.CASES)
def test_every_solver_class_with_a_device_side_count(ctx, cap, reduced):
    """texture, half-flat, impulse pair, noise, flat: consecutive tickets with 0 < n < n_max, a few dozen (or no) records, n == n_max and
    n == 0 under ONE capacity; then the three "move" frames, whose pairs carry a real flow (an island, a rotation 1e-3 from the identity:
    pinned on the CPU) over most of the frame and over its right half -- least squares, RANSAC with fewer samples than records and with more
    samples than the capacity (above 8,192 samples the refit takes the cluster solver with the inlier count on the device), detector on"""
    kinds = ("texture", "halfflat", "impulse", "noise", "flat") + fc.MOVE
    frames = [fc.frame(k) for k in kinds]
    grid = (fc.REDUCED_CAPS if reduced else fc.DOWNSAMPLED_CAPS)[cap]
    for use_ransac, ns in ((False, 1000),) + tuple((True, s) for s in fc.samples_for(grid[0] * grid[1])):
        tail = _tail(use_ransac, ns)
        got = _stream(ctx, frames, _kw(cap, reduced), [tail] * len(frames))
        assert not got[0]["have_vectors"] and got[0]["n_vectors"] == 0 and got[0]["motion"] is None
        np.testing.assert_array_equal(got[0]["quat"], IDENTITY)
        counts = []
        for k in range(1, len(kinds)):
            rec_o, grid_o = fc.records(kinds[k - 1], kinds[k], cap, reduced)
            _check(ctx, got[k], rec_o, grid_o, tail, f"cap {cap} reduced={reduced} ransac={use_ransac}/{ns} {kinds[k - 1]} -> {kinds[k]}")
            counts.append(got[k]["n_vectors"])
        cells = grid_o[0] * grid_o[1]
        assert 0 < counts[0] < cells and counts[2] == cells and counts[3] == 0 and 0 < counts[6] < counts[5], counts
        for k in (6, 7):                                   # the motion pairs: nothing here is compared with an empty field or the identity
            assert got[k]["motion"] is not None and got[k]["motion"][0] >= 100 and fc.off_identity(got[k]["quat"]) > 1e-3, (k, got[k]["quat"])
        # n == 0: identity, no motion -- never NaN, a hang or an error
        np.testing.assert_array_equal(got[4]["quat"], IDENTITY)
        assert got[4]["motion"] is None
    ctx.lk_reset()


def test_fewer_than_three_records(ctx):
    """one weight-4 impulse whose 10 x 10 box of mask falls into one cell of a 12 x 6 grid, or straddles two: the oracle's answer"""
    for n in (1, 2):
        kinds = (f"few{n}_prev", f"few{n}")
        for use_ransac in (False, True):
            tail = _tail(use_ransac, 1000)
            got = _stream(ctx, [fc.frame(k) for k in kinds], _kw(fc.FEW_CAP, False), [tail] * 2)
            rec_o, grid_o = fc.records(*kinds, fc.FEW_CAP, False)
            assert len(rec_o) == n
            _check(ctx, got[1], rec_o, grid_o, tail, f"{n} record(s) ransac={use_ransac}")
    ctx.lk_reset()


def test_launch_per_step_solver_with_a_device_side_count(ctx):
    """OFPS_HIP_ALMEIDA_PATH=step sends every size to the launch-per-step kernels (the path of capacities the cluster cannot hold): least
    squares, and RANSAC with more than 8,192 samples, whose refit is then the stepped solver with the inlier count on the device and
    min_n = 3 (the flat frame: no inlier, identity from the epilogue launch)"""
    ctx.set_option("OFPS_HIP_ALMEIDA_PATH", "step")
    try:
        for cap, reduced in (((150, 150), False), ((480, 270), True)):
            kinds = fc.MOVE + ("flat", "noise")
            for tail in (_tail(), _tail(True, cap[0] * cap[1] + 1000)):
                got = _stream(ctx, [fc.frame(k) for k in kinds], _kw(cap, reduced), [tail] * len(kinds))
                for k in range(1, len(kinds)):
                    rec_o, grid_o = fc.records(kinds[k - 1], kinds[k], cap, reduced)
                    _check(ctx, got[k], rec_o, grid_o, tail, f"stepped, cap {cap} ransac={tail['use_ransac']} {kinds[k - 1]} -> {kinds[k]}",
                           stagewise=False)
                assert fc.off_identity(got[1]["quat"]) > 1e-3 and fc.off_identity(got[2]["quat"]) > 1e-3
                np.testing.assert_array_equal(got[3]["quat"], IDENTITY)
    finally:
        ctx.set_option("OFPS_HIP_ALMEIDA_PATH", None)
        ctx.lk_reset()


@pytest.mark.parametrize("cap,reduced", [((100, 100), False), ((300, 300), True)])
def test_detector_two_pass_sort_with_a_device_side_count(ctx, cap, reduced):
    """a 23 x 23 detector field (529 cells: two digits of the densifier's radix sort) on 5,600 and 50,400 records of capacity"""
    kinds = fc.MOVE + ("halfflat",)
    tail = _tail(detector_params=fc.DETECTOR_FINE)
    got = _stream(ctx, [fc.frame(k) for k in kinds], _kw(cap, reduced), [tail] * len(kinds))
    for k in range(1, len(kinds)):
        rec_o, grid_o = fc.records(kinds[k - 1], kinds[k], cap, reduced)
        _check(ctx, got[k], rec_o, grid_o, tail, f"23 x 23 field, cap {cap} {kinds[k - 1]} -> {kinds[k]}")
    assert got[1]["motion"] is not None and got[1]["motion"][1].shape == (23, 23, 2) and got[1]["motion"][0] >= 400
    ctx.lk_reset()


# ------------------------------------------------------------------------------------------------------------------------------ streams
def _cycle(n):
    return [fc.STREAM_CYCLE[k % len(fc.STREAM_CYCLE)] for k in range(n)]


def test_stream_hip_lk_two_tickets_in_flight(ctx):
    """flat / noise / impulse / half-flat / texture, detector AND estimator on, the tail alternating between least squares and RANSAC:
    consecutive tickets have very different counts -- each ticket's island, quaternion and records are its own frame's"""
    kinds = _cycle(10)
    tails = [_tail(bool(k & 1), 300) for k in range(len(kinds))]
    for cap, reduced in ((fc.DEFAULT_CAP, False), ((300, 300), True)):
        got = _stream(ctx, [fc.frame(k) for k in kinds], _kw(cap, reduced), tails)
        for k in range(1, len(kinds)):
            rec_o, grid_o = fc.records(kinds[k - 1], kinds[k], cap, reduced)
            _check(ctx, got[k], rec_o, grid_o, tails[k], f"hip_lk stream cap {cap} frame {k} ({kinds[k - 1]} -> {kinds[k]})")
    ctx.lk_reset()


def test_stream_hip_flow_with_use_previous(ctx):
    """hip_flow with OFPS_HIP_FLOW_USE_PREVIOUS: the oracle's flow chained through `init`, the fused tail on each pair's records"""
    kinds = _cycle(9)
    frames = [fc.frame(k) for k in kinds]
    grid = oracle.cv_grid(fc.W, fc.H, *fc.DEFAULT_CAP)
    tails = [_tail(bool(k & 1), 300) for k in range(len(kinds))]
    got = _stream(ctx, frames, _kw(fc.DEFAULT_CAP, False, farneback=True, params=fc.FB, use_previous=True), tails)
    flow = None
    for k in range(1, len(kinds)):
        flow = oracle.farneback_flow(frames[k - 1], frames[k], init=flow)
        rec_o = oracle.densify_to_entries(oracle.masked_flow_to_entries(flow, oracle.contrast_mask(frames[k])), *grid)
        _check(ctx, got[k], rec_o, tuple(grid), tails[k], f"hip_flow stream frame {k} ({kinds[k - 1]} -> {kinds[k]})")
    ctx.lk_reset()


# ------------------------------------------------------------------------------------------------------------------ stream equivalences
def test_sync_equals_async_and_mixes_with_the_plain_calls(ctx):
    """sync == async + wait; fused and plain pushes interleaved on one stream; either wait collects either ticket"""
    kinds = _cycle(9)
    frames = [fc.frame(k) for k in kinds]
    kw, tail = _kw(fc.DEFAULT_CAP, False), _tail()
    plain_kw = {k: v for k, v in kw.items() if k != "levels" and k != "radius" and k != "iters"}
    ref = _stream(ctx, frames, kw, [tail] * len(frames))
    ctx.lk_reset()
    first = ctx.lk_push_frame_fused(frames[0], **kw, **tail)
    assert not first["have_vectors"] and first["motion"] is None and first["entries"] is None
    np.testing.assert_array_equal(first["quat"], IDENTITY)
    for k in range(1, len(frames)):
        what = f"frame {k}"
        if k % 3 == 0:                                          # a plain push in the middle of the stream
            ent, grid = ctx.lk_push_frame(frames[k], *fc.LK, **plain_kw)
            np.testing.assert_array_equal(_bits(ent), _bits(ref[k]["entries"]), err_msg=what)
            assert grid == ref[k]["grid"]
            continue
        r = ctx.lk_push_frame_fused(frames[k], **kw, **tail)
        np.testing.assert_array_equal(_bits(r["entries"]), _bits(ref[k]["entries"]), err_msg=what)
        assert (r["motion"] is None) == (ref[k]["motion"] is None) and r["n_vectors"] == ref[k]["n_vectors"]
        if r["motion"] is not None:
            assert r["motion"][0] == ref[k]["motion"][0]
            np.testing.assert_array_equal(_bits(r["motion"][1]), _bits(ref[k]["motion"][1]), err_msg=what)
        np.testing.assert_array_equal(_bits(r["quat"]), _bits(ref[k]["quat"]), err_msg=what)     # the same launches: the same bits
    # a plain wait on a fused ticket, a fused wait on a plain ticket
    ctx.lk_reset()
    pins = [ctx.pinned_array(frames[0].shape, np.uint8) for _ in range(3)]
    for k in range(3):
        np.copyto(pins[k], frames[k])
    t0 = ctx.lk_push_frame_fused_async(pins[0], **kw, **tail)
    assert ctx.lk_frame_wait(t0) is None
    t1 = ctx.lk_push_frame_fused_async(pins[1], **kw, **tail)
    t2 = ctx.lk_push_frame_async(pins[2], *fc.LK, **plain_kw)
    ent, grid = ctx.lk_frame_wait(t1)
    np.testing.assert_array_equal(_bits(ent), _bits(ref[1]["entries"]))
    r = ctx.lk_frame_fused_wait(t2)
    np.testing.assert_array_equal(_bits(r["entries"]), _bits(ref[2]["entries"]))
    assert r["have_vectors"] and r["motion"] is None and r["n_vectors"] == ref[2]["n_vectors"]
    np.testing.assert_array_equal(r["quat"], IDENTITY)
    for p in pins:
        ctx.free_pinned(p)
    ctx.lk_reset()


def test_third_push_reset_and_rewind_with_a_fused_ticket_pending(ctx):
    from ofps_amd._lib import OfpsHipError
    kinds = ("flat",) + fc.MOVE
    frames = [fc.frame(k) for k in kinds]
    kw, tail = _kw(fc.DEFAULT_CAP, False), _tail()
    pins = [ctx.pinned_array(frames[0].shape, np.uint8) for _ in range(3)]
    for k in range(3):
        np.copyto(pins[k], frames[k])
    for drop in (ctx.lk_reset, ctx.lk_rewind):
        ctx.lk_reset()
        t0 = ctx.lk_push_frame_fused_async(pins[0], **kw, **tail)
        t1 = ctx.lk_push_frame_fused_async(pins[1], **kw, **tail)
        with pytest.raises(OfpsHipError) as ei:
            ctx.lk_push_frame_fused_async(pins[2], **kw, **tail)
        assert ei.value.code == -1                               # OFPS_HIP_EINVAL: at most two frames in flight
        r0 = ctx.lk_frame_fused_wait(t0)
        assert not r0["have_vectors"]
        drop()                                                   # t1 is pending: drained and forgotten
        with pytest.raises(OfpsHipError):
            ctx.lk_frame_fused_wait(t1)
        first = ctx.lk_push_frame_fused(frames[1], **kw, **tail)
        assert not first["have_vectors"]                         # a new stream's first frame
        r = ctx.lk_push_frame_fused(frames[2], **kw, **tail)
        rec_o, grid_o = fc.records(kinds[1], kinds[2], fc.DEFAULT_CAP, False)
        _check(ctx, r, rec_o, grid_o, tail, f"after {drop.__name__}")
    with pytest.raises(OfpsHipError) as ei:                      # the full-resolution record form has no fused tail
        ctx.lk_push_frame_fused(frames[0], **kw, **tail, fullres_records=True)
    assert ei.value.code == -3
    for p in pins:
        ctx.free_pinned(p)
    ctx.lk_reset()


def test_existing_device_entry_points_are_unchanged_by_a_fused_call(ctx):
    """ofps_hip_almeida_dev / ofps_hip_detect_dev with a host n: the same bits before and after fused calls on the same context"""
    import torch
    rec, _ = fc.records("move0", "move1", fc.DEFAULT_CAP, False)
    d_ent = torch.from_numpy(rec.copy()).cuda()
    dim = ctx.block_dim(fc.DETECTOR["min_size"], fc.DETECTOR["subdivide"])

    def stagewise():
        out = []
        for use_ransac in (False, True):
            d_q = torch.zeros(4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.almeida_dev(d_ent.data_ptr(), len(rec), 1, *fc.CAM, use_ransac, fc.RANSAC_ITERS, fc.INLIER_DEG, 300, fc.SEED, d_q.data_ptr())
            ctx.sync()
            out.append(d_q.cpu().numpy())
        d_res = torch.zeros(4, dtype=torch.int32, device="cuda")
        d_fld = torch.zeros(dim * dim * 2, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.detect_dev(d_ent.data_ptr(), len(rec), 1, fc.DETECTOR["min_size"], fc.DETECTOR["subdivide"], fc.DETECTOR["target_motion"],
                       d_res.data_ptr(), d_fld.data_ptr())
        ctx.sync()
        return out + [d_res.cpu().numpy().astype(np.float32), d_fld.cpu().numpy()]

    before = stagewise()
    for use_ransac in (False, True):
        _stream(ctx, [fc.frame(k) for k in fc.MOVE + ("noise",)], _kw(fc.DEFAULT_CAP, False), [_tail(use_ransac, 20000)] * 4)
    after = stagewise()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    np.testing.assert_allclose(before[0], fc.expected(rec)[1], atol=LSQ_ATOL, rtol=0)
    ctx.lk_reset()


# ---------------------------------------------------------------------------------------------------------------------------- full size
@pytest.mark.parametrize("decoder", ["hip_flow_reduced_bgr", "hip_lk_default_grid"])
def test_full_size_stream(ctx, decoder):
    """1080p: a BGR hip_flow stream in the reduced mode and a hip_lk stream on the default 150 x 84 grid, 4 frames each, against the oracle"""
    W, H = 1920, 1080
    kinds = fc.MOVE + ("impulse",)
    tail = _tail()
    if decoder == "hip_flow_reduced_bgr":
        frames = [fc.bgr_of(fc.frame(k, W, H)) for k in kinds]
        kw = _kw(fc.DEFAULT_CAP, True, farneback=True, params=fc.FB, fmt=oracle.FMT_BGR)
        want = [fc.records(kinds[k - 1], kinds[k], fc.DEFAULT_CAP, True, True, fc.FB, W, H, oracle.FMT_BGR) for k in range(1, 4)]
    else:
        frames = [fc.frame(k, W, H) for k in kinds]
        kw = _kw(fc.DEFAULT_CAP, False)
        want = [fc.records(kinds[k - 1], kinds[k], fc.DEFAULT_CAP, False, False, fc.LK, W, H) for k in range(1, 4)]
    got = _stream(ctx, frames, kw, [tail] * 4)
    for k in range(1, 4):
        _check(ctx, got[k], want[k - 1][0], want[k - 1][1], tail, f"1080p {decoder} frame {k}")
    ctx.lk_reset()


# ------------------------------------------------------------------------------------------------------------- the cluster's recovery
def test_cluster_recovery_in_the_device_count_form():
    """one fused 150 x 84 least-squares frame with the test-hooks library's withheld granule armed: the bounded wait expires, one workgroup
    solves the problem alone from the device-side count, the oracle's quaternion comes back"""
    from ofps_amd.runtime import HipContext
    hooks = HipContext(0, test_hooks=True)
    try:
        kinds = ("move0", "move1")
        tail = _tail(detector=False)
        ref = _stream(hooks, [fc.frame(k) for k in kinds], _kw(fc.DEFAULT_CAP, False), [tail] * 2)
        r0 = hooks.almeida_recoveries()
        hooks.set_option("OFPS_HIP_ALMEIDA_TEST_FAULT", "2")
        got = _stream(hooks, [fc.frame(k) for k in kinds], _kw(fc.DEFAULT_CAP, False), [tail] * 2)
        hooks.set_option("OFPS_HIP_ALMEIDA_TEST_FAULT", None)
        assert hooks.almeida_recoveries() == r0 + 1
        rec_o, grid_o = fc.records(*kinds, fc.DEFAULT_CAP, False)
        _check(hooks, got[1], rec_o, grid_o, tail, "withheld granule", stagewise=False)
        np.testing.assert_allclose(got[1]["quat"], ref[1]["quat"], atol=LSQ_ATOL, rtol=0)
        assert fc.off_identity(got[1]["quat"]) > 1e-3
    finally:
        hooks.set_option("OFPS_HIP_ALMEIDA_TEST_FAULT", None)
        hooks.close()
