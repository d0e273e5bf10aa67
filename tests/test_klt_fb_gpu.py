"""-m gpu: hip_klt's forward-backward check (include/ofps_hip.h N3f) through the C ABI, bit for bit against the restatement
tests/indep_klt_fb.py: the stage ofps_hip_klt_track_q[_dev]; ofps_hip_klt_track / _flow, host and _dev, at the limits 1, 16, 64 and 4096 on the
cases of tests/klt_cases.py with guard words behind every output; mean removal and the check together on the relit pairs; the batch form in
chain and key mode against one-pair calls and the restatement; the fused sparse form of the dense decoders' stream against
ofps_hip_klt_flow + ofps_hip_detect + ofps_hip_almeida; the batched stream and two multi-device workers against the single-context stream;
the option and the environment variable; the plugin and the C++ host by name; the setting switched off against a context that never saw
the setter; the refusals.  Every comparison is bit for bit but the quaternion's (2e-6, the bound of the existing fused tests).
Expectations are computed once per process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import indep_klt as ik
import indep_klt_fb as ifb
import klt_batch_cases as bc
import klt_cases as kc
import klt_fb_cases as fc
import klt_zm_cases as zc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6
GUARD = 64
GUARD_WORD = 0x5A17C0DE
CAM = (16 / 9, 39.6 * 9 / 16)
SEED = 77
R160 = (16, 2, 1, 1, 160, 4, 7, 10)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    assert c.get_klt_fb() == 0 and c.get_klt_mean_removal() == 0
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(ctx, params, fb_limit=None, mean_removal=None):
    cell, r, min_score, min_eig, R, L, w, K = params
    ctx.set_klt(cell, r, min_score, min_eig, R)
    if fb_limit is not None:
        ctx.set_klt_fb(fb_limit)
    if mean_removal is not None:
        ctx.set_klt_mean_removal(1 if mean_removal else 0)
    return L, w, K


def _reset(ctx):
    ctx.set_klt(); ctx.set_klt_fb(0); ctx.set_klt_mean_removal(0)


class _DevBuf:
    """device memory of `words` 32-bit words with GUARD more behind them"""

    def __init__(self, ctx, words, fill=None):
        self.ctx, self.words = ctx, int(words)
        self.ptr = ctx.malloc(4 * (self.words + GUARD))
        host = np.full(self.words + GUARD, GUARD_WORD, np.uint32)
        if fill is not None:
            host[:self.words] = np.ascontiguousarray(fill).view(np.uint32).ravel()
        ctx.memcpy_h2d(self.ptr, host)

    def read(self, dtype):
        host = np.zeros(self.words + GUARD, np.uint32)
        self.ctx.memcpy_d2h(host, self.ptr)
        assert (host[self.words:] == GUARD_WORD).all(), "guard words behind a device output were overwritten"
        return host[:self.words].view(dtype)

    def free(self):
        self.ctx.free(self.ptr)


def _dev_frame(ctx, img, pad):
    view, stride = kc.padded(img, pad)
    buf = np.ascontiguousarray(view.base if view.base is not None else view)
    ptr = ctx.malloc(buf.size)
    ctx.memcpy_h2d(ptr, buf)
    return ptr, stride


def _dev_forms(ctx, prev, cur, pad, L, w, K, points, points_q=None):
    """the _dev forms that track, on frames with `pad` bytes of row padding -> (quads of `points`, records, count, slots, quads of points_q)"""
    H, W = prev.shape
    ns = ctx.klt_slot_count(W, H)
    dp, stride = _dev_frame(ctx, prev, pad)
    dc, _ = _dev_frame(ctx, cur, pad)
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
    ptq = np.ascontiguousarray(points_q if points_q is not None else np.zeros((0, 2)), np.int32).reshape(-1, 2)
    b_pts, b_quad = _DevBuf(ctx, max(2 * len(pts), 1), pts if len(pts) else None), _DevBuf(ctx, max(4 * len(pts), 1))
    b_ptq, b_quadq = _DevBuf(ctx, max(2 * len(ptq), 1), ptq if len(ptq) else None), _DevBuf(ctx, max(4 * len(ptq), 1))
    b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns)
    try:
        ctx.klt_track_dev(dp, dc, W, H, stride, b_pts.ptr, len(pts), L, w, K, b_quad.ptr)
        ctx.klt_track_q_dev(dp, dc, W, H, stride, b_ptq.ptr, len(ptq), L, w, K, b_quadq.ptr)
        ctx.klt_flow_dev(dp, dc, W, H, stride, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        count = int(b_cnt.read(np.uint32)[0])
        return (b_quad.read(np.int32)[:4 * len(pts)].reshape(-1, 4), b_rec.read(np.float32).reshape(-1, 4)[:count], count,
                b_slots.read(np.int32).reshape(-1, 6), b_quadq.read(np.int32)[:4 * len(ptq)].reshape(-1, 4))
    finally:
        for b in (b_pts, b_quad, b_ptq, b_quadq, b_rec, b_cnt, b_slots):
            b.free()
        ctx.free(dp); ctx.free(dc)


def _check_stage_forms(ctx, name, params, fb_limit, pad=0, mean_removal=False):
    """host and _dev forms of _flow and _track on one case, parameter set and limit against the restatement"""
    prev, cur = fc.case(name)
    exp = fc.expect(name, params, fb_limit, mean_removal)
    L, w, K = _set(ctx, params, fb_limit, mean_removal)
    what = f"{name} {params} limit {fb_limit} pad {pad} mean removal {mean_removal}"
    stride = None
    pv, cv = prev, cur
    if pad:
        (pv, stride), (cv, _) = kc.padded(prev, pad), kc.padded(cur, pad)
    ent, slots = ctx.klt_flow(pv, cv, L, w, K, want_slots=True, stride=stride)
    np.testing.assert_array_equal(slots, exp["slots"], err_msg=what + ": slots")
    assert len(ent) == exp["count"], what
    np.testing.assert_array_equal(_bits(ent), _bits(exp["records"]), err_msg=what + ": record bits")
    pts, quads = fc.quads(exp)
    np.testing.assert_array_equal(ctx.klt_track(pv, cv, pts, L, w, K, stride=stride), quads, err_msg=what + ": quadruples")
    dq, drec, dcount, dslots, _ = _dev_forms(ctx, prev, cur, pad, L, w, K, pts)
    np.testing.assert_array_equal(dq, quads, err_msg=what + ": track_dev")
    np.testing.assert_array_equal(dslots, exp["slots"], err_msg=what + ": flow_dev slots")
    assert dcount == exp["count"], what
    np.testing.assert_array_equal(_bits(drec), _bits(exp["records"]), err_msg=what + ": flow_dev record bits")
    return slots


# ------------------------------------------------------------------------------------------------ the stage form
@pytest.mark.parametrize("mean_removal", [False, True], ids=["plain", "zm"])
def test_track_q_on_subpixel_points_corners_and_points_outside(ctx, mean_removal):
    prev, cur = fc.case("warp97")
    H, W = prev.shape
    xm, ym = 256 * (W - 1), 256 * (H - 1)
    rng = np.random.default_rng(9)
    inside = np.concatenate([[[0, 0], [xm, 0], [0, ym], [xm, ym], [xm - 1, ym - 1], [1, 1], [128 * W, 128 * H], [256 * 40 + 255, 256 * 30 + 129]],
                             np.column_stack([rng.integers(0, xm + 1, 40), rng.integers(0, ym + 1, 40)])]).astype(np.int32)
    outside = np.array([[-1, 5], [xm + 1, 5], [5, -1], [5, ym + 1], [256 * W, 256 * H], [-(2 ** 31), 2 ** 31 - 1], [2 ** 31 - 1, -(2 ** 31)]],
                       np.int64).astype(np.int32)
    left = np.tile(np.array([0, 0, 0, ik.ST_LEFT], np.int32), (len(outside), 1))
    try:
        ctx.set_klt_fb(64)                                     # the stage never applies the check
        seen = set()
        for params in (fc.SET0, (16, 2, 1, 1, 64, 1, 1, 1), (16, 2, 1, 400, 160, 3, 7, 30), kc.DEFAULT_SET):
            L, w, K = _set(ctx, params, mean_removal=mean_removal)
            want = ifb.track_points_q(prev, cur, inside, L, w, K, params[3], params[4], mean_removal)
            seen |= set(want[:, 3])
            np.testing.assert_array_equal(ctx.klt_track_q(prev, cur, inside, L, w, K), want, err_msg=str(params))
            for pad in (0, 13):
                got = _dev_forms(ctx, prev, cur, pad, L, w, K, np.zeros((0, 2)), np.concatenate([inside, outside]))[4]
                np.testing.assert_array_equal(got[:len(inside)], want, err_msg=f"{params} pad {pad}")
                np.testing.assert_array_equal(got[len(inside):], left, err_msg=f"{params} pad {pad}")
            # whole pixels: what ofps_hip_klt_track answers there with the check off
            whole = inside[:8] & ~255
            ctx.set_klt_fb(0)
            np.testing.assert_array_equal(ctx.klt_track_q(prev, cur, whole, L, w, K), ctx.klt_track(prev, cur, whole >> 8, L, w, K))
            ctx.set_klt_fb(64)
        assert seen >= {ik.ST_KEPT, ik.ST_LEFT, ik.ST_RESIDUAL}, seen
        for k in range(len(outside)):
            with pytest.raises(OfpsHipError) as e:
                ctx.klt_track_q(prev, cur, outside[k:k + 1], 2, 4, 10)
            assert e.value.code == EINVAL, outside[k]
        assert len(ctx.klt_track_q(prev, cur, np.zeros((0, 2), np.int32), 2, 4, 10)) == 0
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ stage forms against the restatement
@pytest.mark.parametrize("fb_limit", fc.LIMITS)
@pytest.mark.parametrize("name", fc.SMALL_NAMES)
def test_stage_forms_match_the_restatement(ctx, name, fb_limit):
    """the seven small cases x PARAM_SETS: w = 1, 4, 7, L = 1 .. 4, K = 1, 10, 30"""
    try:
        for params in kc.PARAM_SETS:
            _check_stage_forms(ctx, name, params, fb_limit)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("fb_limit", fc.LIMITS)
@pytest.mark.parametrize("params", [kc.DEFAULT_SET, R160], ids=["R0", "R160"])
def test_decoder_defaults_on_the_320_pair(ctx, params, fb_limit):
    assert [kc.DEFAULT_SET, R160] == kc.param_sets("warp320")
    try:
        slots = _check_stage_forms(ctx, "warp320", params, fb_limit)
        if params == kc.DEFAULT_SET:                           # one backward pass leaves the frame: no limit keeps that slot
            assert (slots[:, 5] == ifb.ST_NO_RETURN).sum() >= 1
    finally:
        _reset(ctx)


def test_every_reason_for_not_returning_comes_back_as_status_5(ctx):
    try:
        slots = _check_stage_forms(ctx, "luma", kc.PARAM_SETS[1], 64)      # backward passes that are flat or lost by their residual
        assert (slots[:, 5] == ifb.ST_NO_RETURN).sum() == 174 - 15
        slots = _check_stage_forms(ctx, "repaint", fc.SET0, 64)            # the distance alone
        assert (slots[:, 5] == ifb.ST_NO_RETURN).sum() == 13 and not (slots[fc.in_repaint(slots), 5] == ik.ST_KEPT).any()
    finally:
        _reset(ctx)


@pytest.mark.parametrize("fb_limit", [16, 64])
@pytest.mark.parametrize("offset", zc.RELIT_OFFSETS)
def test_mean_removal_and_the_check_on_the_relit_pairs(ctx, offset, fb_limit):
    try:
        for params in (zc.SET0, zc.SET0_R64):
            _check_stage_forms(ctx, f"warp96{offset:+d}", params, fb_limit, mean_removal=True)
        base = _check_stage_forms(ctx, "inv", zc.SET0_R64, fb_limit, mean_removal=True)
        np.testing.assert_array_equal(_check_stage_forms(ctx, f"inv{offset:+d}", zc.SET0_R64, fb_limit, mean_removal=True), base)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("mean_removal", [False, True], ids=["plain", "zm"])
@pytest.mark.parametrize("pad", [12, 13])
def test_padded_rows(ctx, pad, mean_removal):
    try:
        _check_stage_forms(ctx, "warp97+20" if mean_removal else "warp97", zc.SET0_R64, 64, pad, mean_removal)
        _check_stage_forms(ctx, "repaint", fc.SET0, 16, pad, mean_removal)
    finally:
        _reset(ctx)


def test_host_forms_leave_the_words_behind_their_outputs_alone(ctx):
    prev, cur = fc.case("repaint")
    H, W = prev.shape
    _reset(ctx)
    ctx.set_klt_fb(64)
    try:
        ns = ctx.klt_slot_count(W, H)
        lib, h = ctx._lib, ctx._h
        u8, i32, f32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)
        ent = np.full(4 * ns + GUARD, GUARD_WORD, np.uint32)
        slots = np.full(6 * ns + GUARD, GUARD_WORD, np.uint32)
        pts = np.array([[10, 10], [60, 40], [127, 95]], np.int32)
        quads = np.full(4 * len(pts) + GUARD, GUARD_WORD, np.uint32)
        quads_q = np.full(4 * len(pts) + GUARD, GUARD_WORD, np.uint32)
        pts_q = (256 * pts + np.array([[3, 250], [128, 1], [0, 0]])).astype(np.int32)
        n = C.c_uint32(0)
        p, c = np.ascontiguousarray(prev), np.ascontiguousarray(cur)
        assert lib.ofps_hip_klt_flow(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, 2, 4, 10, ent.ctypes.data_as(f32), C.byref(n),
                                     slots.ctypes.data_as(i32)) == 0
        assert lib.ofps_hip_klt_track(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, pts.ctypes.data_as(i32), len(pts), 2, 4, 10,
                                      quads.ctypes.data_as(i32)) == 0
        assert lib.ofps_hip_klt_track_q(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, pts_q.ctypes.data_as(i32), len(pts), 2, 4, 10,
                                        quads_q.ctypes.data_as(i32)) == 0
        for a, words in ((ent, 4 * ns), (slots, 6 * ns), (quads, 4 * len(pts)), (quads_q, 4 * len(pts))):
            assert (a[words:] == GUARD_WORD).all()
        exp = fc.expect("repaint", fc.SET0, 64)
        assert n.value == exp["count"]
        np.testing.assert_array_equal(slots[:6 * ns].view(np.int32).reshape(-1, 6), exp["slots"])
        np.testing.assert_array_equal(quads[:4 * len(pts)].view(np.int32).reshape(-1, 4), ifb.track(prev, cur, pts, 2, 4, 10, fb_limit=64))
        np.testing.assert_array_equal(quads_q[:4 * len(pts)].view(np.int32).reshape(-1, 4), ifb.track_points_q(prev, cur, pts_q, 2, 4, 10))
    finally:
        _reset(ctx)


def test_features_do_not_change(ctx):
    prev, _ = fc.case("repaint")
    _reset(ctx)
    ctx.set_klt_fb(64)
    try:
        np.testing.assert_array_equal(ctx.klt_features(prev), fc.expect("repaint", fc.SET0, 0)["features"])
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ batch form
def _upload(ctx, fr):
    ptr = ctx.malloc(fr.size)
    ctx.memcpy_h2d(ptr, np.ascontiguousarray(fr))
    return ptr, fr.shape[2], fr.shape[1] * fr.shape[2]


def _batch_dev(ctx, fr, ref_mode, L, w, K):
    n, H, W = fr.shape
    pairs, ns = n - 1, ctx.klt_slot_count(W, H)
    d, stride, pitch = _upload(ctx, fr)
    b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * pairs * ns), _DevBuf(ctx, pairs), _DevBuf(ctx, 6 * pairs * ns)
    try:
        ctx.klt_flow_batch_dev(d, n, W, H, stride, pitch, ref_mode, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        return b_rec.read(np.float32).reshape(pairs, ns, 4), b_cnt.read(np.uint32).copy(), b_slots.read(np.int32).reshape(pairs, ns, 6)
    finally:
        for b in (b_rec, b_cnt, b_slots):
            b.free()
        ctx.free(d)


def _check_items(got, want, what):
    rec, counts, slots = got
    assert len(counts) == len(want), what
    for k, (wrec, wcount, wslots) in enumerate(want):
        assert int(counts[k]) == wcount, f"{what}: item {k} count {int(counts[k])} != {wcount}"
        np.testing.assert_array_equal(_bits(rec[k][:wcount]), _bits(wrec), err_msg=f"{what}: item {k} record bits")
        np.testing.assert_array_equal(slots[k], wslots, err_msg=f"{what}: item {k} slots")


@pytest.mark.parametrize("mean_removal", [False, True], ids=["plain", "zm"])
@pytest.mark.parametrize("ref_mode", [0, 1], ids=["chain", "key"])
def test_batch_form_against_one_pair_calls_and_the_restatement(ctx, ref_mode, mean_removal):
    fr = fc.sequence(flicker=mean_removal)
    params = zc.SET0_R64 if ref_mode else fc.SET0
    fb_limit = 16 if ref_mode else 64
    L, w, K = _set(ctx, params, fb_limit, mean_removal)
    try:
        restated = [(e["records"], int(e["count"]), e["slots"]) for e in fc.sequence_expect(params, ref_mode, fb_limit, mean_removal, mean_removal)]
        assert any((e[2][:, 5] == ifb.ST_NO_RETURN).any() for e in restated)
        pairs = []
        for k in range(len(fr) - 1):
            a, b = bc.pair_of(k, ref_mode)
            ent, slots = ctx.klt_flow(fr[a], fr[b], L, w, K, want_slots=True)
            pairs.append((ent, len(ent), slots))
        for want, what in ((restated, "restatement"), (pairs, "one-pair calls")):
            _check_items(_batch_dev(ctx, fr, ref_mode, L, w, K), want, f"dev, {what}")
            _check_items(ctx.klt_flow_batch(fr, L, w, K, ref_mode=ref_mode, want_slots=True), want, f"host, {what}")
        one = fr[:2]                                           # a batch of one pair keeps the one-pair compaction
        _check_items(ctx.klt_flow_batch(one, L, w, K, ref_mode=ref_mode, want_slots=True), restated[:1], "one pair")
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ fused sparse form
@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
def test_fused_sparse_form(ctx, use_ransac):
    fr = fc.sequence()
    L, w, K = _set(ctx, fc.SET0, 64)
    tail = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1],
                use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200)
    try:
        ctx.lk_reset()
        first = ctx.lk_push_frame_fused(np.ascontiguousarray(fr[0]), L, w, K, sparse=True, seed=SEED, **tail)
        assert not first["have_vectors"]
        restated = fc.sequence_expect(fc.SET0, 0, 64)
        for k in range(1, len(fr)):
            r = ctx.lk_push_frame_fused(np.ascontiguousarray(fr[k]), L, w, K, sparse=True, seed=SEED + k, **tail)
            want = ctx.klt_flow(fr[k - 1], fr[k], L, w, K)
            assert r["have_vectors"] and r["n_vectors"] == len(want) == restated[k - 1]["count"], k
            np.testing.assert_array_equal(_bits(r["entries"]), _bits(want), err_msg=f"frame {k}")
            np.testing.assert_array_equal(_bits(want), _bits(restated[k - 1]["records"]), err_msg=f"frame {k}")
            det = ctx.detect(want, 0.05, 3, 0.003)
            assert (det is None) == (r["motion"] is None), k
            if det is not None:
                assert det[0] == r["motion"][0], k
                np.testing.assert_array_equal(_bits(det[1]), _bits(r["motion"][1]), err_msg=f"frame {k}")
            q, _ = ctx.almeida(want, *CAM, use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200, seed=SEED + k)
            print("frame", k, "quaternion difference", float(np.abs(q - r["quat"]).max()))
            assert np.abs(q - r["quat"]).max() <= QUAT_BOUND, k
    finally:
        ctx.lk_reset(); _reset(ctx)


# ------------------------------------------------------------------------------------------------ batched stream and workers
def _single_stream(ctx, frames, L, w, K, **tail):
    ctx.lk_reset()
    out = [ctx.lk_push_frame_fused(np.ascontiguousarray(f), L, w, K, sparse=True, seed=SEED + j, **tail) for j, f in enumerate(frames)]
    ctx.lk_reset()
    return out


def _batched_stream(ctx, frames, sizes, L, w, K, **tail):
    n, H, W = frames.shape
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
    try:
        ctx.reset_frames()
        ns = ctx.batch_record_capacity(W, H)
        out, start = [], 0
        for size in sizes:
            batch = np.ascontiguousarray(frames[start:start + size])
            ent = np.zeros((size, ns, 4), np.float32)
            for j, r in enumerate(ctx.frames_wait(ctx.push_frames_async(batch, seed=SEED + start, out_entries=ent, **tail))):
                r["entries"] = ent[j][:r["n_vectors"]].copy()
                out.append(r)
            start += size
        return out
    finally:
        ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)


def test_batched_stream_and_workers_equal_the_single_context_stream(ctx):
    fr = fc.sequence()
    L, w, K = _set(ctx, fc.SET0, 64)
    try:
        single = _single_stream(ctx, fr, L, w, K)
        batched = _batched_stream(ctx, fr, (3, 3), L, w, K)
    finally:
        _reset(ctx)
    restated = fc.sequence_expect(fc.SET0, 0, 64)
    assert not single[0]["have_vectors"] and not batched[0]["have_vectors"]
    for k in range(1, 6):
        s, b = single[k], batched[k]
        assert s["have_vectors"] and b["have_vectors"] and s["n_vectors"] == b["n_vectors"] == restated[k - 1]["count"], k
        np.testing.assert_array_equal(_bits(b["entries"]), _bits(s["entries"][:s["n_vectors"]]), err_msg=f"frame {k}")
        np.testing.assert_array_equal(_bits(b["entries"]), _bits(restated[k - 1]["records"]), err_msg=f"frame {k}")
        assert (s["motion"] is None) == (b["motion"] is None), k
        if s["motion"] is not None:
            assert s["motion"][0] == b["motion"][0], k
        assert np.abs(s["quat"] - b["quat"]).max() <= QUAT_BOUND, k
    # two workers on device 0, their contexts' settings from the environment alone
    cell, r, min_score, min_eig, R, _, _, _ = fc.SET0
    env = dict(os.environ, OFPS_HIP_BATCH_DECODER="1", OFPS_HIP_KLT_FB="64", OFPS_HIP_KLT_CELL=str(cell), OFPS_HIP_KLT_SCORE_RADIUS=str(r),
               OFPS_HIP_KLT_MIN_SCORE=str(min_score), OFPS_HIP_KLT_MIN_EIG=str(min_eig), OFPS_HIP_KLT_MAX_RESIDUAL=str(R), OFPS_HIP_KLT_LEVELS=str(L),
               OFPS_HIP_KLT_RADIUS=str(w), OFPS_HIP_KLT_ITERS=str(K), KLT_CHILD_SEED=str(SEED))
    env.pop("OFPS_HIP_KLT_MEAN_REMOVAL", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_klt_fb_child.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    got = child["frames"]
    assert child["capacity"] == 48 and [g["have_vectors"] for g in got] == [False] + [True] * 5
    for k in range(1, 6):
        assert got[k]["n_vectors"] == batched[k]["n_vectors"], k
        assert got[k]["entries"] == _bits(batched[k]["entries"]).reshape(-1).tolist(), k
        assert got[k]["quat"] == _bits(batched[k]["quat"]).tolist(), k
        assert got[k]["motion"] == (list(batched[k]["motion"]) if batched[k]["motion"] is not None else None), k


def test_the_option_and_the_environment_variable_set_what_the_getter_reads(ctx):
    try:
        assert ctx.get_klt_fb() == 0
        ctx.set_option("OFPS_HIP_KLT_FB", 64)
        assert ctx.get_klt_fb() == 64
        np.testing.assert_array_equal(ctx.klt_flow(*fc.case("repaint"), 2, 4, 10, want_slots=True)[1], fc.expect("repaint", fc.SET0, 64)["slots"])
        ctx.set_option("OFPS_HIP_KLT_FB", 4096)
        assert ctx.get_klt_fb() == 4096
        ctx.set_option("OFPS_HIP_KLT_FB", 0)
        assert ctx.get_klt_fb() == 0
        ctx.set_klt_fb(16)
        ctx.set_option("OFPS_HIP_KLT_FB", None)
        assert ctx.get_klt_fb() == 0                           # the default
    finally:
        _reset(ctx)
    code = ("import sys; sys.path.insert(0, %r); from ofps_amd.runtime import HipContext; c = HipContext(0); "
            "print(c.get_klt_fb()); c.close()" % ROOT)
    for value, want in (("64", 64), ("far", 0)):               # a malformed variable is reported once and ignored
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OFPS_HIP_KLT_FB=value), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert int(p.stdout.strip().splitlines()[-1]) == want, value
        assert ("OFPS_HIP_KLT_FB" in p.stderr) == (value == "far")


# ------------------------------------------------------------------------------------------------ plugin and C++ host
def test_plugin_property_reaches_the_context():
    from ofps_amd.plugins import HipKltDecoder
    fr = fc.sequence()
    dec = HipKltDecoder(iter([fr[0], fr[1], fr[2], fr[3]]))
    try:
        assert ("Consistency check", "usize", 0, 0, 4096) in dec.props()
        for name, value in (("Levels", 2), ("Window radius", 4), ("Iterations", 10)):
            assert dec.set_prop(name, value)
        assert dec.set_prop("Consistency check", 64)
        assert ("Consistency check", "usize", 64, 0, 4096) in dec.props()
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt_fb() == 64
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(fc.sequence_expect(fc.SET0, 0, 64)[0]["records"]))
        assert dec.set_prop("Consistency check", 16)           # switched in mid-stream
        field = []
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt_fb() == 16
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(fc.sequence_expect(fc.SET0, 0, 16)[1]["records"]))
        assert dec.set_prop("Consistency check", 0)            # and off: the next pair is the unchecked tracker's
        field = []
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt_fb() == 0
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(fc.sequence_expect(fc.SET0, 0, 0)[2]["records"]))
    finally:
        dec.ctx.close()


def test_cpp_host_property_by_name(tmp_path):
    from ofps_amd import mvec
    tool = os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool")
    fr = fc.sequence()
    raw = tmp_path / "clip.y"
    raw.write_bytes(b"".join(np.ascontiguousarray(f).tobytes() for f in fr[:4]))
    out = tmp_path / "clip_klt.mvec"
    arg = f"{raw}?w=128&h=96&fps=30"
    # on for frames 1 and 2, off before frame 3 is read
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "4", "Levels=2", "Window radius=4", "Consistency check=64", "Consistency check=0@3"],
                       check=True, capture_output=True, text=True, timeout=120)
    frames = list(mvec.read_frames(open(out, "rb")))
    assert json.loads(p.stdout)["frames"] == 4 == len(frames) and len(frames[0]) == 0
    on, off = fc.sequence_expect(fc.SET0, 0, 64), fc.sequence_expect(fc.SET0, 0, 0)
    for k, want in ((1, on[0]), (2, on[1]), (3, off[2])):
        np.testing.assert_array_equal(_bits(frames[k]), _bits(want["records"]), err_msg=f"frame {k}")
    assert on[2]["records"].tobytes() != off[2]["records"].tobytes()
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "2", "Consistency check=64", "Consistency checks=1"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "Consistency checks" in p.stderr
    # a saved configuration carries it like every other property
    cfg = {"decoder": [{"selected_plugin": "hip_klt", "arg": arg, "extra": False}, True],
           "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": None}, True],
           "settings": {"worker": {"decoder_properties": {"Consistency check": {"Usize": {"val": 64, "min": 0, "max": 4096}},
                                                          "Levels": {"Usize": {"val": 2, "min": 1, "max": 6}}},
                                   "realtime_processing": False, "detector_properties": {}},
                        "overlay_mf": False, "max_frame_gap": 3, "min_frames": 1, "draw_perf_stats": {"summary_window": False, "graph_window": False}}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    got = json.loads(subprocess.run([tool, "parse-config", str(path)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert got["decoder_properties"]["Consistency check"] == ["Usize", 64, 0, 4096]
    det = json.loads(subprocess.run([tool, "detect", "--config", str(path)], check=True, capture_output=True, text=True, timeout=120)
                     .stdout.strip().splitlines()[-1])
    assert det["frames"] == 4
    # the stream benchmark's flag
    r = json.loads(subprocess.run([tool, "stream-bench", "128", "96", "12", "batch", "3", "--klt", "--klt-fb", "64"], check=True, capture_output=True,
                                  text=True, timeout=120).stdout.strip().splitlines()[-1])
    assert r["decoder"] == "hip_klt" and r["fb_limit"] == 64 and 0 <= r["last_n_vectors"] <= 48


# ------------------------------------------------------------------------------------------------ feature off
def _off_answers(c):
    """klt_flow, the batch form and a push_frames_async ticket on the sequence, as bytes"""
    fr = fc.sequence()
    L, w, K = _set(c, zc.SET0_R64)
    ent, slots = c.klt_flow(fr[0], fr[1], L, w, K, want_slots=True)
    rec, counts, bslots = c.klt_flow_batch(fr, L, w, K, want_slots=True)
    kept = b"".join(rec[k][:int(counts[k])].tobytes() for k in range(len(counts)))
    stream = _batched_stream(c, fr, (3, 3), L, w, K)
    c.set_klt()
    return (ent.tobytes(), slots.tobytes(), kept, counts.tobytes(), bslots.tobytes(),
            [(r["have_vectors"], r["n_vectors"], r["motion"], r["quat"].tobytes(), r["entries"].tobytes()) for r in stream])


def test_switched_off_equals_a_context_that_never_saw_the_setter(ctx):
    from ofps_amd.runtime import HipContext
    _reset(ctx)
    ctx.set_klt_fb(64)
    try:
        on = _off_answers(ctx)                                 # calls with the setting on
        ctx.set_klt_fb(0)
        fresh = HipContext(0)
        try:
            assert fresh.get_klt_fb() == 0
            off, want = _off_answers(ctx), _off_answers(fresh)
            assert off == want
            assert on[1] != off[1] and on[4] != off[4] and on[5] != off[5]      # and the setting did something
            plain = fc.sequence_expect(zc.SET0_R64, 0, 0)
            np.testing.assert_array_equal(np.frombuffer(off[1], np.int32).reshape(-1, 6), plain[0]["slots"])
            np.testing.assert_array_equal(np.frombuffer(on[1], np.int32).reshape(-1, 6), fc.sequence_expect(zc.SET0_R64, 0, 64)[0]["slots"])
        finally:
            fresh.close()
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    _reset(ctx)
    ctx.set_klt_fb(64)

    try:
        for bad in (-1, 4097, 2 ** 31 - 1, -(2 ** 31)):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_klt_fb(bad)
            assert e.value.code == EINVAL, bad
            assert ctx.get_klt_fb() == 64, bad                 # the setting stays as it was
            np.testing.assert_array_equal(ctx.klt_flow(*fc.case("repaint"), 2, 4, 10, want_slots=True)[1], fc.expect("repaint", fc.SET0, 64)["slots"])
        for bad in ("far", "-1", "4097", "64x", "1e2", " 64"):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_option("OFPS_HIP_KLT_FB", bad)
            assert e.value.code == EINVAL, bad
            assert ctx.get_klt_fb() == 64, bad
            np.testing.assert_array_equal(ctx.klt_flow(*fc.case("repaint"), 2, 4, 10, want_slots=True)[1], fc.expect("repaint", fc.SET0, 64)["slots"])
        ctx.set_klt_fb(4096); ctx.set_klt_fb(1); ctx.set_klt_fb(64)
        assert ctx._lib.ofps_hip_set_klt_fb(None, 1) == EINVAL and ctx._lib.ofps_hip_get_klt_fb(None) == EINVAL
    finally:
        _reset(ctx)
