"""hip_klt's motion prediction (include/ofps_hip.h N3p) on the GPU, bit for bit against the restatement tests/indep_klt_pred.py: the predictor's
stage form, tracks from caller-given guesses, the flow of a pair started from the previous pair's slots, the sparse stream and fused forms
with the setting on, the forms that ignore it, both hosts' property, and the refusals."""
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
import indep_klt_pred as ip
import klt_cases as kc
import klt_pred_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6
GUARD = 64
GUARD_WORD = 0x5A17C0DE
CAM = (16 / 9, 39.6 * 9 / 16)
SEED = 77
VARIANTS = [(False, 0), (True, 0), (False, 1), (False, 64), (True, 1), (True, 64)]      # (mean removal, F)
VARIANT_IDS = ["plain", "zm", "F1", "F64", "zm-F1", "zm-F64"]
PER_KIND = 10                                                # points per kind of guess in one call


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    assert c.get_klt_prediction() == 0 and c.get_klt_fb() == 0 and c.get_klt_mean_removal() == 0
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(ctx, params, fb_limit=0, mean_removal=False):
    cell, r, min_score, min_eig, R, L, w, K = params
    ctx.set_klt(cell, r, min_score, min_eig, R)
    ctx.set_klt_fb(fb_limit)
    ctx.set_klt_mean_removal(1 if mean_removal else 0)
    return L, w, K


def _reset(ctx):
    ctx.set_klt(); ctx.set_klt_fb(0); ctx.set_klt_mean_removal(0); ctx.set_klt_prediction(0)


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


# ------------------------------------------------------------------------------------------------ the predictor
def _predict_both_forms(ctx, slots, W, H, cell):
    want = ip.predict(slots, W, H, cell)
    np.testing.assert_array_equal(ctx.klt_predict(slots, W, H, cell), want)
    ns = len(want)
    b_in, b_out = _DevBuf(ctx, 6 * ns, slots), _DevBuf(ctx, 2 * ns)
    try:
        ctx.klt_predict_dev(b_in.ptr, W, H, cell, b_out.ptr)
        ctx.sync()
        np.testing.assert_array_equal(b_out.read(np.int32).reshape(-1, 2), want)
        np.testing.assert_array_equal(b_in.read(np.int32).reshape(-1, 6), slots)
    finally:
        b_in.free(); b_out.free()
    return want


@pytest.mark.parametrize("table", pc.predictor_tables(), ids=lambda t: t[0])
def test_predict_on_the_hand_made_tables(ctx, table):
    name, W, H, cell, slots = table
    _predict_both_forms(ctx, slots, W, H, cell)


def test_predict_host_form_leaves_the_words_behind_its_output_alone(ctx):
    name, W, H, cell, slots = pc.predictor_tables()[6]
    ns = len(slots)
    out = np.full(2 * ns + GUARD, GUARD_WORD, np.uint32)
    i32 = C.POINTER(C.c_int32)
    assert ctx._lib.ofps_hip_klt_predict(ctx._h, np.ascontiguousarray(slots).ctypes.data_as(i32), W, H, cell, out.ctypes.data_as(i32)) == 0
    assert (out[2 * ns:] == GUARD_WORD).all()
    np.testing.assert_array_equal(out[:2 * ns].view(np.int32).reshape(-1, 2), ip.predict(slots, W, H, cell))


@pytest.mark.parametrize("cell", [8, 16, 32])
def test_predict_on_the_slots_of_a_real_pair(ctx, cell):
    fr = pc.ramp_frames("ramp3")
    params = (cell,) + pc.RAMP_SET[1:]
    L, w, K = _set(ctx, params)
    try:
        _, slots = ctx.klt_flow(fr[2], fr[3], L, w, K, want_slots=True)
        assert (slots[:, 5] == ik.ST_KEPT).any()
        g = _predict_both_forms(ctx, slots, pc.RAMP_W, pc.RAMP_H, cell)
        assert g.any()
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ tracks from guesses
def _mixed(name, params):
    """-> (points, guesses, host mask): every kind of guess on up to PER_KIND features each, and three points outside the frame; the host form
    takes the rows of the mask (it refuses a far guess and a point outside)"""
    cell, r, min_score = params[:3]
    prev, _ = pc.case(name)
    H, W = prev.shape
    feat = pc.points(name, cell, r, min_score)
    pts = feat[np.linspace(0, len(feat) - 1, min(PER_KIND, len(feat))).astype(int)]
    P, G, host = [], [], []
    for kind in pc.GUESS_KINDS:
        g = pc.guesses(name, kind, pts)
        P.append(pts); G.append(g)
        host.append((np.abs(g.astype(np.int64)) <= ip.MAX_GUESS).all(axis=1))
    outside = np.array([[W, 3], [-1, 5], [7, H]], np.int32)
    P.append(outside); G.append(np.array([[0, 0], [256, -256], [-77, 5]], np.int32)); host.append(np.zeros(3, bool))
    return np.concatenate(P).astype(np.int32), np.concatenate(G).astype(np.int32), np.concatenate(host)


def _track_from_both_forms(ctx, name, params, mean_removal, fb_limit, pad=0):
    prev, cur = pc.case(name)
    H, W = prev.shape
    cell, r, min_score, min_eig, R, L, w, K = params
    pts, gs, host = _mixed(name, params)
    want = ip.track_from(prev, cur, pts, gs, L, w, K, min_eig, R, mean_removal, fb_limit)
    _set(ctx, params, fb_limit, mean_removal)
    what = f"{name} {params} mean removal {mean_removal} limit {fb_limit} pad {pad}"
    try:
        stride, pv, cv = None, prev, cur
        if pad:
            (pv, stride), (cv, _) = kc.padded(prev, pad), kc.padded(cur, pad)
        np.testing.assert_array_equal(ctx.klt_track_from(pv, cv, pts[host], gs[host], L, w, K, stride=stride), want[host], err_msg=what + ": host form")
        with pytest.raises(OfpsHipError) as e:                 # a guess beyond +-2^23: refused by the host form ...
            ctx.klt_track_from(pv, cv, pts[:len(pts) - 3], gs[:len(pts) - 3], L, w, K, stride=stride)
        assert e.value.code == EINVAL
        dp, dstride = _dev_frame(ctx, prev, pad)
        dc, _ = _dev_frame(ctx, cur, pad)
        b_pts, b_gs, b_quad = _DevBuf(ctx, 2 * len(pts), pts), _DevBuf(ctx, 2 * len(pts), gs), _DevBuf(ctx, 4 * len(pts))
        try:
            ctx.klt_track_from_dev(dp, dc, W, H, dstride, b_pts.ptr, b_gs.ptr, len(pts), L, w, K, b_quad.ptr)
            ctx.sync()
            np.testing.assert_array_equal(b_quad.read(np.int32).reshape(-1, 4), want, err_msg=what + ": _dev form")      # ... and (0, 0) here
            b_pts.read(np.int32); b_gs.read(np.int32)
        finally:
            for b in (b_pts, b_gs, b_quad):
                b.free()
            ctx.free(dp); ctx.free(dc)
    finally:
        _reset(ctx)
    return pts, gs, want


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name", pc.SMALL_NAMES)
def test_track_from_matches_the_restatement(ctx, name, variant):
    seen = set()
    for params in kc.PARAM_SETS:
        pts, gs, want = _track_from_both_forms(ctx, name, params, *variant)
        seen |= set(want[:, 3])
        n = (len(pts) - 3) // 4
        np.testing.assert_array_equal(want[2 * n:3 * n], want[:n])         # a guess that leaves the frame is the zero guess
        assert (want[-3:, 3] == ik.ST_LEFT).all() and not want[-3:, :3].any()
    assert ik.ST_LEFT in seen and (ik.ST_KEPT in seen or variant[1] == 1)      # (an exact round trip, F = 1, may keep none of a case's points)


@pytest.mark.parametrize("variant", [(False, 0), (True, 64)], ids=["plain", "zm-F64"])
@pytest.mark.parametrize("pad", [12, 13])
def test_track_from_on_padded_rows(ctx, pad, variant):
    _track_from_both_forms(ctx, "warp97", kc.PARAM_SETS[0], *variant, pad=pad)


def test_track_from_host_form_leaves_the_words_behind_its_output_alone_and_does_not_read_the_setting(ctx):
    prev, cur = pc.case("warp96")
    pts, gs, want = pc.track_expect("warp96", kc.PARAM_SETS[0], "truth", True, 64)
    _set(ctx, kc.PARAM_SETS[0], 64, True)
    try:
        u8, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        for on in (0, 1):
            ctx.set_klt_prediction(on)
            quads = np.full(4 * len(pts) + GUARD, GUARD_WORD, np.uint32)
            p, c = np.ascontiguousarray(prev), np.ascontiguousarray(cur)
            assert ctx._lib.ofps_hip_klt_track_from(ctx._h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), 96, 64, 96, np.ascontiguousarray(pts).ctypes.data_as(i32),
                                                    np.ascontiguousarray(gs).ctypes.data_as(i32), len(pts), 2, 4, 10, quads.ctypes.data_as(i32)) == 0
            assert (quads[4 * len(pts):] == GUARD_WORD).all()
            np.testing.assert_array_equal(quads[:4 * len(pts)].view(np.int32).reshape(-1, 4), want)
        assert len(ctx.klt_track_from(prev, cur, np.zeros((0, 2)), np.zeros((0, 2)), 2, 4, 10)) == 0
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ the flow of a chain of pairs
def _flow_from_dev(ctx, prev, cur, L, w, K, b_prev_slots, b_slots):
    H, W = prev.shape
    ns = ctx.klt_slot_count(W, H)
    dp, stride = _dev_frame(ctx, prev, 0)
    dc, _ = _dev_frame(ctx, cur, 0)
    b_rec, b_cnt = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1)
    try:
        ctx.klt_flow_from_dev(dp, dc, W, H, stride, L, w, K, b_prev_slots.ptr if b_prev_slots else None, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        count = int(b_cnt.read(np.uint32)[0])
        return b_rec.read(np.float32).reshape(-1, 4)[:count], b_slots.read(np.int32).reshape(-1, 6).copy()
    finally:
        b_rec.free(); b_cnt.free()
        ctx.free(dp); ctx.free(dc)


@pytest.mark.parametrize("fb_limit", [0, 64])
@pytest.mark.parametrize("params", [pc.RAMP_SET, pc.DEFAULT_SET], ids=["L2w4", "defaults"])
@pytest.mark.parametrize("name", ["ramp3", "ramp4"])
def test_flow_from_chained_over_the_ramps(ctx, name, params, fb_limit):
    fr = pc.ramp_frames(name)
    want = pc.ramp_expect(name, params, True, fb_limit)
    plain = pc.ramp_expect(name, params, False, fb_limit)
    L, w, K = _set(ctx, params, fb_limit)
    ns = ctx.klt_slot_count(pc.RAMP_W, pc.RAMP_H)
    bufs = [_DevBuf(ctx, 6 * ns), _DevBuf(ctx, 6 * ns)]
    try:
        prev_slots = None
        for k in range(len(fr) - 1):
            ent, slots = ctx.klt_flow_from(fr[k], fr[k + 1], L, w, K, prev_slots)
            np.testing.assert_array_equal(slots, want[k]["slots"], err_msg=f"pair {k}: slots")
            assert len(ent) == want[k]["count"]
            np.testing.assert_array_equal(_bits(ent), _bits(want[k]["records"]), err_msg=f"pair {k}: record bits")
            drec, dslots = _flow_from_dev(ctx, fr[k], fr[k + 1], L, w, K, bufs[(k + 1) & 1] if k else None, bufs[k & 1])
            np.testing.assert_array_equal(dslots, want[k]["slots"], err_msg=f"pair {k}: _dev slots")
            np.testing.assert_array_equal(_bits(drec), _bits(want[k]["records"]), err_msg=f"pair {k}: _dev record bits")
            # prev_slots = NULL is ofps_hip_klt_flow
            e0, s0 = ctx.klt_flow_from(fr[k], fr[k + 1], L, w, K, None)
            e1, s1 = ctx.klt_flow(fr[k], fr[k + 1], L, w, K, want_slots=True)
            assert e0.tobytes() == e1.tobytes() and s0.tobytes() == s1.tobytes()
            np.testing.assert_array_equal(s1, plain[k]["slots"], err_msg=f"pair {k}: unpredicted slots")
            prev_slots = slots
        assert any(want[k]["slots"].tobytes() != plain[k]["slots"].tobytes() for k in range(1, len(fr) - 1))
    finally:
        for b in bufs:
            b.free()
        _reset(ctx)


def test_flow_from_with_mean_removal_and_without_slots_out(ctx):
    fr = pc.ramp_frames("ramp3")
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True, 64, True)
    L, w, K = _set(ctx, pc.RAMP_SET, 64, True)
    try:
        prev_slots = None
        for k in range(4):
            ent, slots = ctx.klt_flow_from(fr[k], fr[k + 1], L, w, K, prev_slots)
            np.testing.assert_array_equal(slots, want[k]["slots"], err_msg=f"pair {k}")
            only = ctx.klt_flow_from(fr[k], fr[k + 1], L, w, K, prev_slots, want_slots=False)
            assert only.tobytes() == ent.tobytes() == want[k]["records"].tobytes()
            prev_slots = slots
    finally:
        _reset(ctx)


def test_flow_from_host_form_leaves_the_words_behind_its_outputs_alone_and_dev_form_refuses_overlapping_slots(ctx):
    fr = pc.ramp_frames("ramp3")
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True, 64)
    L, w, K = _set(ctx, pc.RAMP_SET, 64)
    try:
        ns = ctx.klt_slot_count(pc.RAMP_W, pc.RAMP_H)
        u8, i32, f32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)
        prev_slots = None
        for k in range(3):
            ent = np.full(4 * ns + GUARD, GUARD_WORD, np.uint32)
            slots = np.full(6 * ns + GUARD, GUARD_WORD, np.uint32)
            n = np.full(1 + GUARD, GUARD_WORD, np.uint32)
            p, c = np.ascontiguousarray(fr[k]), np.ascontiguousarray(fr[k + 1])
            assert ctx._lib.ofps_hip_klt_flow_from(ctx._h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), pc.RAMP_W, pc.RAMP_H, pc.RAMP_W, L, w, K,
                                                   prev_slots.ctypes.data_as(i32) if prev_slots is not None else None, ent.ctypes.data_as(f32),
                                                   n.ctypes.data_as(C.POINTER(C.c_uint32)), slots.ctypes.data_as(i32)) == 0
            for a, words in ((ent, 4 * ns), (slots, 6 * ns), (n, 1)):
                assert (a[words:] == GUARD_WORD).all(), k
            assert int(n[0]) == want[k]["count"]
            np.testing.assert_array_equal(slots[:6 * ns].view(np.int32).reshape(-1, 6), want[k]["slots"], err_msg=f"pair {k}")
            np.testing.assert_array_equal(ent[:4 * int(n[0])], _bits(want[k]["records"]).ravel(), err_msg=f"pair {k}")
            prev_slots = np.ascontiguousarray(slots[:6 * ns].view(np.int32))
        # the host form copies prev_slots first, so one array may be both
        both = prev_slots.copy()
        ent, got = np.zeros((ns, 4), np.float32), None
        n = C.c_uint32(0)
        p, c = np.ascontiguousarray(fr[3]), np.ascontiguousarray(fr[4])
        assert ctx._lib.ofps_hip_klt_flow_from(ctx._h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), pc.RAMP_W, pc.RAMP_H, pc.RAMP_W, L, w, K,
                                               both.ctypes.data_as(i32), ent.ctypes.data_as(f32), C.byref(n), both.ctypes.data_as(i32)) == 0
        np.testing.assert_array_equal(both.reshape(-1, 6), want[3]["slots"])
        # the _dev form refuses arrays that share a byte, before anything is enqueued
        buf = _DevBuf(ctx, 12 * ns, np.concatenate([prev_slots, prev_slots]))
        b_rec, b_cnt = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1)
        dp, stride = _dev_frame(ctx, fr[3], 0)
        dc, _ = _dev_frame(ctx, fr[4], 0)
        try:
            for off_prev, off_out in ((0, 0), (0, 4), (24 * ns - 4, 0)):
                with pytest.raises(OfpsHipError) as e:
                    ctx.klt_flow_from_dev(dp, dc, pc.RAMP_W, pc.RAMP_H, stride, L, w, K, buf.ptr + off_prev, b_rec.ptr, b_cnt.ptr, buf.ptr + off_out)
                assert e.value.code == EINVAL
            ctx.klt_flow_from_dev(dp, dc, pc.RAMP_W, pc.RAMP_H, stride, L, w, K, buf.ptr, b_rec.ptr, b_cnt.ptr, buf.ptr + 24 * ns)      # side by side
            ctx.sync()
            np.testing.assert_array_equal(buf.read(np.int32)[6 * ns:].reshape(-1, 6), want[3]["slots"])
            assert int(b_cnt.read(np.uint32)[0]) == want[3]["count"]
        finally:
            for b in (buf, b_rec, b_cnt):
                b.free()
            ctx.free(dp); ctx.free(dc)
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ the stream forms
def _stream_sync(ctx, frames, L, w, K, **kw):
    return [ctx.lk_push_frame(np.ascontiguousarray(f), L, w, K, sparse=True, **kw) for f in frames]


def _check_stream(got, want, what):
    assert got[0] is None, what
    for k, w in enumerate(want):
        ent = got[k + 1][0]
        assert len(ent) == w["count"], f"{what}: pair {k} count {len(ent)} != {w['count']}"
        np.testing.assert_array_equal(_bits(ent), _bits(w["records"]), err_msg=f"{what}: pair {k} record bits")


@pytest.mark.parametrize("fb_limit", [0, 64])
def test_stream_with_the_setting_on_synchronous_and_two_tickets_in_flight(ctx, fb_limit):
    fr = pc.ramp_frames("ramp3")
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True, fb_limit)
    plain = pc.ramp_expect("ramp3", pc.RAMP_SET, False, fb_limit)
    L, w, K = _set(ctx, pc.RAMP_SET, fb_limit)
    try:
        ctx.lk_reset()
        _check_stream(_stream_sync(ctx, fr, L, w, K), plain, "setting off")
        ctx.set_klt_prediction(1)
        ctx.lk_reset()
        _check_stream(_stream_sync(ctx, fr, L, w, K), want, "synchronous")
        # two tickets in flight: frame k + 1 is pushed before frame k's ticket is collected
        ctx.lk_reset()
        keep = [np.ascontiguousarray(f) for f in fr]
        got, tickets = [], [ctx.lk_push_frame_async(keep[0], L, w, K, sparse=True)]
        for k in range(1, len(keep)):
            tickets.append(ctx.lk_push_frame_async(keep[k], L, w, K, sparse=True))
            got.append(ctx.lk_frame_wait(tickets[k - 1]))
        got.append(ctx.lk_frame_wait(tickets[-1]))
        _check_stream(got, want, "two tickets in flight")
        # ofps_hip_lk_reset in mid-sequence forgets the slots: the next pair is the unpredicted one
        ctx.lk_reset()
        got = _stream_sync(ctx, fr[:4], L, w, K)
        ctx.lk_reset()
        got2 = _stream_sync(ctx, fr[3:6], L, w, K)
        _check_stream(got, want[:3], "before the reset")
        np.testing.assert_array_equal(_bits(got2[1][0]), _bits(plain[3]["records"]))
        assert plain[3]["records"].tobytes() != want[3]["records"].tobytes()
        # ... and the pair behind it is predicted from that one
        cell, r, ms, e, R = pc.RAMP_SET[:5]
        after = ip.flow_from(fr[4], fr[5], L, w, K, plain[3]["slots"], cell, r, ms, e, R, False, fb_limit)
        np.testing.assert_array_equal(_bits(got2[2][0]), _bits(after["records"]))
    finally:
        ctx.lk_reset(); _reset(ctx)


def test_the_setting_switched_in_mid_stream(ctx):
    fr = pc.ramp_frames("ramp3")
    cell, r, ms, e, R, L, w, K = pc.RAMP_SET
    on = [1, 1, 0, 1, 1, 0]                                  # the setting at the push that completes pair k
    want, prev_slots = [], None
    for k in range(6):
        o = ip.flow_from(fr[k], fr[k + 1], L, w, K, prev_slots if on[k] else None, cell, r, ms, e, R)
        want.append(o)
        prev_slots = o["slots"] if on[k] else None           # a pair pushed with the setting off writes no slots
    _set(ctx, pc.RAMP_SET)
    try:
        ctx.lk_reset()
        got = [ctx.lk_push_frame(np.ascontiguousarray(fr[0]), L, w, K, sparse=True)]
        for k in range(6):
            ctx.set_klt_prediction(on[k])
            got.append(ctx.lk_push_frame(np.ascontiguousarray(fr[k + 1]), L, w, K, sparse=True))
        _check_stream(got, want, "switched")
        plain = pc.ramp_expect("ramp3", pc.RAMP_SET, False)
        assert want[3]["records"].tobytes() == plain[3]["records"].tobytes()          # the successor of an unpredicted pair starts from zero
        assert want[4]["records"].tobytes() != plain[4]["records"].tobytes()
        # the chain of ofps_hip_klt_flow_from calls says the same
        ent, slots = ctx.klt_flow_from(fr[3], fr[4], L, w, K, None)
        ent4, _ = ctx.klt_flow_from(fr[4], fr[5], L, w, K, slots)
        assert ent4.tobytes() == got[5][0].tobytes()
    finally:
        ctx.lk_reset(); _reset(ctx)


def _bgr(f, k):
    """a colour frame whose grey value is not one of its channels"""
    f = f.astype(np.int32)
    return np.ascontiguousarray(np.stack([np.clip(f + 9, 0, 255), f, np.clip(f - 14, 0, 255)], 2).astype(np.uint8))


@pytest.mark.parametrize("mode", ["luma-reduced", "bgr-reduced", "bgr-full"])
def test_stream_reduced_and_bgr_against_the_chain_on_the_frames_the_tracker_reads(ctx, mode):
    from ofps_amd.runtime import HipContext
    fr = pc.ramp_frames("ramp4")[:6]
    fmt = HipContext.FMT_BGR if mode.startswith("bgr") else HipContext.FMT_LUMA
    reduced = mode.endswith("reduced")
    frames = [_bgr(f, k) if fmt != HipContext.FMT_LUMA else np.ascontiguousarray(f) for k, f in enumerate(fr)]
    kw = dict(reduced=reduced, fmt=fmt, max_w=120, max_h=120)
    cell, r, ms, e, R, L, w, K = pc.RAMP_SET
    _set(ctx, pc.RAMP_SET, 64)
    try:
        gray = [ctx.cv_frontend(f, fmt, reduced, 120, 120) for f in frames]
        assert gray[0].shape == ((72, 120) if reduced else (96, 160))
        want = ip.flow_chain(gray, L, w, K, True, cell=cell, r=r, min_score=ms, min_eig=e, max_residual=R, fb_limit=64)
        ctx.set_klt_prediction(1)
        ctx.lk_reset()
        got = _stream_sync(ctx, frames, L, w, K, **kw)
        _check_stream(got, want, mode)
        prev_slots = None
        for k in range(5):                                     # the chain of ofps_hip_klt_flow_from calls
            ent, prev_slots = ctx.klt_flow_from(gray[k], gray[k + 1], L, w, K, prev_slots)
            assert ent.tobytes() == got[k + 1][0].tobytes(), k
        assert sum(o["count"] for o in want) > 100
        # a change of mode forgets the slots: the same frames full-size and luma start from zero again
        if reduced:
            other = _stream_sync(ctx, [np.ascontiguousarray(f) for f in fr[3:5]], L, w, K)
            ent, _ = ctx.klt_flow(fr[3], fr[4], L, w, K, want_slots=True)
            assert other[0] is None and other[1][0].tobytes() == ent.tobytes()
    finally:
        ctx.lk_reset(); _reset(ctx)


@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
def test_fused_form_with_the_setting_on(ctx, use_ransac):
    fr = pc.ramp_frames("ramp3")
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True, 64)
    L, w, K = _set(ctx, pc.RAMP_SET, 64)
    tail = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1],
                use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200)
    try:
        ctx.set_klt_prediction(1)
        ctx.lk_reset()
        keep = [np.ascontiguousarray(f) for f in fr]
        if use_ransac:                                         # the read-ahead form, two tickets in flight
            res, tickets = [], [ctx.lk_push_frame_fused_async(keep[0], L, w, K, sparse=True, seed=SEED, **tail)]
            for k in range(1, len(keep)):
                tickets.append(ctx.lk_push_frame_fused_async(keep[k], L, w, K, sparse=True, seed=SEED + k, **tail))
                res.append(ctx.lk_frame_fused_wait(tickets[k - 1]))
            res.append(ctx.lk_frame_fused_wait(tickets[-1]))
        else:
            res = [ctx.lk_push_frame_fused(keep[k], L, w, K, sparse=True, seed=SEED + k, **tail) for k in range(len(keep))]
        assert not res[0]["have_vectors"]
        prev_slots = None
        for k in range(1, len(fr)):
            r = res[k]
            ent, prev_slots = ctx.klt_flow_from(fr[k - 1], fr[k], L, w, K, prev_slots)
            assert r["have_vectors"] and r["n_vectors"] == len(ent) == want[k - 1]["count"], k
            np.testing.assert_array_equal(_bits(r["entries"][:r["n_vectors"]]), _bits(ent), err_msg=f"frame {k}")
            np.testing.assert_array_equal(_bits(ent), _bits(want[k - 1]["records"]), err_msg=f"frame {k}")
            det = ctx.detect(ent, 0.05, 3, 0.003)
            assert (det is None) == (r["motion"] is None), k
            if det is not None:
                assert det[0] == r["motion"][0], k
                np.testing.assert_array_equal(_bits(det[1]), _bits(r["motion"][1]), err_msg=f"frame {k}")
            q, _ = ctx.almeida(ent, *CAM, use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200, seed=SEED + k)
            print("frame", k, "quaternion difference", float(np.abs(q - r["quat"]).max()))
            assert np.abs(q - r["quat"]).max() <= QUAT_BOUND, k
    finally:
        ctx.lk_reset(); _reset(ctx)


def test_the_option_and_the_environment_variable_set_what_the_getter_reads(ctx):
    fr = pc.ramp_frames("ramp3")
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True)
    L, w, K = _set(ctx, pc.RAMP_SET)
    try:
        assert ctx.get_klt_prediction() == 0
        ctx.set_option("OFPS_HIP_KLT_PREDICTION", 1)
        assert ctx.get_klt_prediction() == 1
        ctx.lk_reset()
        _check_stream(_stream_sync(ctx, fr[:4], L, w, K), want[:3], "option")
        ctx.set_option("OFPS_HIP_KLT_PREDICTION", 0)
        assert ctx.get_klt_prediction() == 0
        ctx.set_klt_prediction(1)
        ctx.set_option("OFPS_HIP_KLT_PREDICTION", None)
        assert ctx.get_klt_prediction() == 0                   # the default
    finally:
        ctx.lk_reset(); _reset(ctx)
    code = ("import sys; sys.path.insert(0, %r); from ofps_amd.runtime import HipContext; c = HipContext(0); "
            "print(c.get_klt_prediction()); c.close()" % ROOT)
    for value, expect in (("1", 1), ("yes", 0)):              # a malformed variable is reported once and ignored
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OFPS_HIP_KLT_PREDICTION=value), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert int(p.stdout.strip().splitlines()[-1]) == expect, value
        assert ("OFPS_HIP_KLT_PREDICTION" in p.stderr) == (value == "yes")


# ------------------------------------------------------------------------------------------------ feature off, and the forms that ignore it
TAIL = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1], use_ransac=False)


def _batched_stream(c, frames, sizes, L, w, K):
    n, H, W = frames.shape
    c.set_batch_decoder(c.BATCH_DECODER_KLT, L, w, K)
    try:
        c.reset_frames()
        ns = c.batch_record_capacity(W, H)
        out, start = [], 0
        for size in sizes:
            batch = np.ascontiguousarray(frames[start:start + size])
            ent = np.zeros((size, ns, 4), np.float32)
            for j, r in enumerate(c.frames_wait(c.push_frames_async(batch, seed=SEED + start, out_entries=ent))):
                out.append((r["have_vectors"], r["n_vectors"], r["motion"], r["quat"].tobytes(), ent[j][:r["n_vectors"]].tobytes()))
            start += size
        return out
    finally:
        c.set_batch_decoder(c.BATCH_DECODER_SAD)


def _one_pair_answers(c):
    """klt_flow, a sparse stream and a fused stream over three frames, as bytes"""
    fr = pc.ramp_frames("ramp3")
    L, w, K = _set(c, pc.RAMP_SET)
    ent, slots = c.klt_flow(fr[3], fr[4], L, w, K, want_slots=True)
    c.lk_reset()
    stream = [c.lk_push_frame(np.ascontiguousarray(f), L, w, K, sparse=True) for f in fr[2:5]]
    c.lk_reset()
    fused = [c.lk_push_frame_fused(np.ascontiguousarray(f), L, w, K, sparse=True, seed=SEED + j, **TAIL) for j, f in enumerate(fr[2:5])]
    c.lk_reset()
    return (ent.tobytes(), slots.tobytes(), [s[0].tobytes() for s in stream[1:]],
            [(r["n_vectors"], r["motion"] is None, r["quat"].tobytes(), r["entries"][:r["n_vectors"]].tobytes()) for r in fused[1:]])


def _batch_answers(c):
    fr = np.stack(pc.ramp_frames("ramp3"))
    L, w, K = _set(c, pc.RAMP_SET)
    out = []
    for ref_mode in (0, 1):
        rec, counts, bslots = c.klt_flow_batch(fr, L, w, K, ref_mode=ref_mode, want_slots=True)
        out.append((b"".join(rec[k][:int(counts[k])].tobytes() for k in range(len(counts))), counts.tobytes(), bslots.tobytes()))
    out.append(_batched_stream(c, fr, (4, 3), L, w, K))
    return out


def test_switched_off_equals_a_context_that_never_saw_the_setter(ctx):
    from ofps_amd.runtime import HipContext
    _reset(ctx)
    ctx.set_klt_prediction(1)
    try:
        on = _one_pair_answers(ctx)                             # calls with the setting on
        ctx.set_klt_prediction(0)
        fresh = HipContext(0)
        try:
            assert fresh.get_klt_prediction() == 0
            off, want = _one_pair_answers(ctx), _one_pair_answers(fresh)
            assert off == want
            assert on[0] == off[0] and on[1] == off[1]          # ofps_hip_klt_flow does not read the setting
            assert on[2][0] == off[2][0] and on[2][1] != off[2][1] and on[3][1] != off[3][1]     # the streams' second pair does
            np.testing.assert_array_equal(np.frombuffer(off[1], np.int32).reshape(-1, 6), pc.ramp_expect("ramp3", pc.RAMP_SET, False)[3]["slots"])
        finally:
            fresh.close()
    finally:
        ctx.lk_reset(); _reset(ctx)


def test_the_batch_form_and_the_batched_stream_ignore_the_setting(ctx):
    _reset(ctx)
    try:
        off = _batch_answers(ctx)
        ctx.set_klt_prediction(1)
        on = _batch_answers(ctx)
        assert on == off
        plain = pc.ramp_expect("ramp3", pc.RAMP_SET, False)
        np.testing.assert_array_equal(np.frombuffer(on[0][2], np.int32).reshape(len(plain), -1, 6), np.stack([p["slots"] for p in plain]))
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ plugin and C++ host
def test_plugin_extension_property_reaches_the_context():
    from ofps_amd.plugins import HipKltDecoder
    fr = pc.ramp_frames("ramp3")
    dec = HipKltDecoder(iter(fr[:5]))
    try:
        assert dec.props()[-1][0] == "Consistency check" and dec.ext_props() == [("Prediction", "bool", False, None, None)]
        for name, value in (("Levels", 2), ("Window radius", 4), ("Iterations", 10)):
            assert dec.set_prop(name, value)
        assert dec.set_prop("Prediction", True) and not dec.set_prop("Predictions", True)
        assert dec.ext_props() == [("Prediction", "bool", True, None, None)]
        on, off = pc.ramp_expect("ramp3", pc.RAMP_SET, True), pc.ramp_expect("ramp3", pc.RAMP_SET, False)
        field = []
        assert dec.process_frame(field) is False
        for k in range(3):
            field = []
            assert dec.process_frame(field) is True
            assert dec.ctx.get_klt_prediction() == 1
            np.testing.assert_array_equal(_bits(np.array(field)), _bits(on[k]["records"]), err_msg=f"pair {k}")
        assert dec.set_prop("Prediction", False)               # switched off in mid-stream
        field = []
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt_prediction() == 0
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(off[3]["records"]))
        assert on[3]["records"].tobytes() != off[3]["records"].tobytes()
    finally:
        dec.ctx.close()


def test_cpp_host_property_by_name(tmp_path):
    from ofps_amd import mvec
    tool = os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool")
    fr = pc.ramp_frames("ramp3")
    raw = tmp_path / "clip.y"
    raw.write_bytes(b"".join(np.ascontiguousarray(f).tobytes() for f in fr[:6]))
    out = tmp_path / "clip_klt.mvec"
    arg = f"{raw}?w={pc.RAMP_W}&h={pc.RAMP_H}&fps=30"
    # on for the pairs that end with frames 1 to 4, off before frame 5 is read
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "6", "Levels=2", "Window radius=4", "Prediction=true", "Prediction=false@5"],
                       check=True, capture_output=True, text=True, timeout=120)
    frames = list(mvec.read_frames(open(out, "rb")))
    assert json.loads(p.stdout)["frames"] == 6 == len(frames) and len(frames[0]) == 0
    on, off = pc.ramp_expect("ramp3", pc.RAMP_SET, True), pc.ramp_expect("ramp3", pc.RAMP_SET, False)
    for k, want in ((1, on[0]), (2, on[1]), (3, on[2]), (4, on[3]), (5, off[4])):
        np.testing.assert_array_equal(_bits(frames[k]), _bits(want["records"]), err_msg=f"frame {k}")
    assert on[3]["records"].tobytes() != off[3]["records"].tobytes() and on[4]["records"].tobytes() != off[4]["records"].tobytes()
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "2", "Prediction=true", "Predictions=true"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "Predictions" in p.stderr
    # a saved configuration carries it like every other property
    cfg = {"decoder": [{"selected_plugin": "hip_klt", "arg": arg, "extra": False}, True],
           "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": None}, True],
           "settings": {"worker": {"decoder_properties": {"Prediction": {"Bool": True}, "Levels": {"Usize": {"val": 2, "min": 1, "max": 6}}},
                                   "realtime_processing": False, "detector_properties": {}},
                        "overlay_mf": False, "max_frame_gap": 3, "min_frames": 1, "draw_perf_stats": {"summary_window": False, "graph_window": False}}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    got = json.loads(subprocess.run([tool, "parse-config", str(path)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert got["decoder_properties"]["Prediction"] == ["Bool", True]
    det = json.loads(subprocess.run([tool, "detect", "--config", str(path)], check=True, capture_output=True, text=True, timeout=120)
                     .stdout.strip().splitlines()[-1])
    assert det["frames"] == 6 and det["decoder_properties"]["Prediction"] is True and det["decoder_properties"]["Levels"] == 2
    cfg["settings"]["worker"]["decoder_properties"]["Prediction"] = {"Bool": False}
    path.write_text(json.dumps(cfg))
    det0 = json.loads(subprocess.run([tool, "detect", "--config", str(path)], check=True, capture_output=True, text=True, timeout=120)
                      .stdout.strip().splitlines()[-1])
    assert det0["frames"] == 6 and det0["decoder_properties"]["Prediction"] is False
    # the stream benchmark's flag: the batched form reports the setting and ignores it
    runs = [json.loads(subprocess.run([tool, "stream-bench", "128", "96", "12", "batch", "3", "--klt"] + extra, check=True, capture_output=True,
                                      text=True, timeout=120).stdout.strip().splitlines()[-1]) for extra in ([], ["--klt-predict"])]
    assert [r["prediction"] for r in runs] == [0, 1] and runs[0]["decoder"] == "hip_klt"
    assert runs[0]["last_n_vectors"] == runs[1]["last_n_vectors"]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    fr = pc.ramp_frames("ramp3")
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True)
    L, w, K = _set(ctx, pc.RAMP_SET)
    ctx.set_klt_prediction(1)

    def valid_call():
        assert ctx.get_klt_prediction() == 1                   # the setting stays as it was
        ctx.lk_reset()
        _check_stream(_stream_sync(ctx, fr[:3], L, w, K), want[:2], "after a refusal")

    try:
        for bad in (-1, 2, 2 ** 31 - 1, -(2 ** 31)):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_klt_prediction(bad)
            assert e.value.code == EINVAL, bad
            valid_call()
        for bad in ("yes", "-1", "2", "1x", " 1"):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_option("OFPS_HIP_KLT_PREDICTION", bad)
            assert e.value.code == EINVAL, bad
            valid_call()
        assert ctx._lib.ofps_hip_set_klt_prediction(None, 1) == EINVAL and ctx._lib.ofps_hip_get_klt_prediction(None) == EINVAL
        slots = np.zeros((60, 6), np.int32)
        for W, H, cell in ((160, 96, 12), (0, 96, 16), (160, 40000, 16)):
            with pytest.raises(OfpsHipError) as e:
                ctx.klt_predict_dev(1, W, H, cell, 1)
            assert e.value.code == EINVAL
        np.testing.assert_array_equal(ctx.klt_predict(slots, 160, 96, 16), 0)
    finally:
        ctx.lk_reset(); _reset(ctx)
