"""-m gpu: hip_klt (include/ofps_hip.h N3) through the C ABI, bit for bit against the restatement tests/indep_klt.py: the stage forms
(ofps_hip_klt_features / _track / _flow, host and _dev) on every case and parameter set of tests/klt_cases.py, with guard words behind
every output and both row paddings; lattices at and above the one-workgroup compaction's limit against the raw slots compacted on the
host; the dense decoders' stream and fused forms with OFPS_HIP_FLOW_SPARSE; the refusals; the dense decoders without the flag against a
context that never saw a klt call; the plugin.  Expectations are computed once per process and shared read-only."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from ofps_amd import synth
from ofps_amd._lib import OfpsHipError

import indep_klt as ik
import klt_cases as kc

pytestmark = pytest.mark.gpu

EINVAL = -1
QUAT_BOUND = 2e-6                                         # the project's solver bound: a fused ticket's quaternion against ofps_hip_almeida
GUARD = 64                                                # guard words behind every output
GUARD_WORD = 0x5A17C0DE
CASES = {name: (prev, cur) for name, prev, cur in kc.content_cases()}
CAM = (16 / 9, 39.6 * 9 / 16)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@lru_cache(maxsize=None)
def _expect(name, params):
    cell, r, min_score, min_eig, R, L, w, K = params
    prev, cur = CASES[name]
    return ik.flow(prev, cur, L, w, K, cell, r, min_score, min_eig, R)


def _set(ctx, params):
    cell, r, min_score, min_eig, R, L, w, K = params
    ctx.set_klt(cell, r, min_score, min_eig, R)
    return L, w, K


def _quads_of(exp):
    s = exp["slots"]
    have = s[:, 5] != ik.ST_NONE
    return s[have][:, :2], np.column_stack([s[have, 3], s[have, 4], exp["residuals"][have], s[have, 5]]).astype(np.int32)


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


def _dev_forms(ctx, prev, cur, pad, L, w, K, points):
    """the three _dev forms on frames with `pad` bytes of row padding -> (triples, quads of `points`, records, count, slots)"""
    H, W = prev.shape
    ns = ctx.klt_slot_count(W, H)
    dp, stride = _dev_frame(ctx, prev, pad)
    dc, _ = _dev_frame(ctx, cur, pad)
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
    b_tri, b_pts, b_quad = _DevBuf(ctx, 3 * ns), _DevBuf(ctx, max(2 * len(pts), 1), pts if len(pts) else None), _DevBuf(ctx, max(4 * len(pts), 1))
    b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns)
    try:
        ctx.klt_features_dev(dp, W, H, stride, b_tri.ptr)
        ctx.klt_track_dev(dp, dc, W, H, stride, b_pts.ptr, len(pts), L, w, K, b_quad.ptr)
        ctx.klt_flow_dev(dp, dc, W, H, stride, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        count = int(b_cnt.read(np.uint32)[0])
        return (b_tri.read(np.int32).reshape(-1, 3), b_quad.read(np.int32)[:4 * len(pts)].reshape(-1, 4),
                b_rec.read(np.float32).reshape(-1, 4)[:count], count, b_slots.read(np.int32).reshape(-1, 6))
    finally:
        for b in (b_tri, b_pts, b_quad, b_rec, b_cnt, b_slots):
            b.free()
        ctx.free(dp); ctx.free(dc)


# ------------------------------------------------------------------------------------------------ stage forms against the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_forms_match_the_restatement(ctx, name):
    prev, cur = CASES[name]
    for params in kc.param_sets(name):
        exp = _expect(name, params)
        L, w, K = _set(ctx, params)
        what = f"{name} {params}"
        np.testing.assert_array_equal(ctx.klt_features(prev), exp["features"], err_msg=what + ": features")
        ent, slots = ctx.klt_flow(prev, cur, L, w, K, want_slots=True)
        np.testing.assert_array_equal(slots, exp["slots"], err_msg=what + ": slots")
        assert len(ent) == exp["count"], what
        np.testing.assert_array_equal(_bits(ent), _bits(exp["records"]), err_msg=what + ": record bits")
        pts, quads = _quads_of(exp)
        np.testing.assert_array_equal(ctx.klt_track(prev, cur, pts, L, w, K), quads, err_msg=what + ": quadruples")
        tri, dq, drec, dcount, dslots = _dev_forms(ctx, prev, cur, 0, L, w, K, pts)
        np.testing.assert_array_equal(tri, exp["features"], err_msg=what + ": features_dev")
        np.testing.assert_array_equal(dq, quads, err_msg=what + ": track_dev")
        np.testing.assert_array_equal(dslots, exp["slots"], err_msg=what + ": flow_dev slots")
        assert dcount == exp["count"], what
        np.testing.assert_array_equal(_bits(drec), _bits(exp["records"]), err_msg=what + ": flow_dev record bits")
    ctx.set_klt()


def test_the_cases_reach_every_status(ctx):
    seen = set()
    for name in CASES:
        for params in kc.param_sets(name):
            seen |= set(np.unique(_expect(name, params)["slots"][:, 5]).tolist())
    assert seen == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ robustness of the stage forms
@pytest.mark.parametrize("pad", [12, 13])
def test_padded_rows(ctx, pad):
    params = kc.PARAM_SETS[0]
    exp = _expect("warp97", params)
    prev, cur = CASES["warp97"]
    L, w, K = _set(ctx, params)
    pv, stride = kc.padded(prev, pad)
    cv, _ = kc.padded(cur, pad)
    np.testing.assert_array_equal(ctx.klt_features(pv, stride=stride), exp["features"])
    ent, slots = ctx.klt_flow(pv, cv, L, w, K, want_slots=True, stride=stride)
    np.testing.assert_array_equal(slots, exp["slots"])
    np.testing.assert_array_equal(_bits(ent), _bits(exp["records"]))
    pts, quads = _quads_of(exp)
    np.testing.assert_array_equal(ctx.klt_track(pv, cv, pts, L, w, K, stride=stride), quads)
    tri, dq, drec, dcount, dslots = _dev_forms(ctx, prev, cur, pad, L, w, K, pts)
    np.testing.assert_array_equal(tri, exp["features"])
    np.testing.assert_array_equal(dq, quads)
    np.testing.assert_array_equal(dslots, exp["slots"])
    np.testing.assert_array_equal(_bits(drec), _bits(exp["records"]))


def test_host_forms_leave_the_words_behind_their_outputs_alone(ctx):
    prev, cur = CASES["warp97"]
    H, W = prev.shape
    ctx.set_klt()
    ns = ctx.klt_slot_count(W, H)
    lib, h = ctx._lib, ctx._h
    u8, i32, f32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    tri = np.full(3 * ns + GUARD, GUARD_WORD, np.uint32)
    ent = np.full(4 * ns + GUARD, GUARD_WORD, np.uint32)
    slots = np.full(6 * ns + GUARD, GUARD_WORD, np.uint32)
    pts = np.array([[10, 10], [40, 30], [96, 64]], np.int32)
    quads = np.full(4 * len(pts) + GUARD, GUARD_WORD, np.uint32)
    n = C.c_uint32(0)
    p, c = np.ascontiguousarray(prev), np.ascontiguousarray(cur)
    assert lib.ofps_hip_klt_features(h, p.ctypes.data_as(u8), W, H, W, tri.ctypes.data_as(i32)) == 0
    assert lib.ofps_hip_klt_flow(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, 2, 4, 10, ent.ctypes.data_as(f32), C.byref(n),
                                 slots.ctypes.data_as(i32)) == 0
    assert lib.ofps_hip_klt_track(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, pts.ctypes.data_as(i32), len(pts), 2, 4, 10,
                                  quads.ctypes.data_as(i32)) == 0
    for a, words in ((tri, 3 * ns), (ent, 4 * ns), (slots, 6 * ns), (quads, 4 * len(pts))):
        assert (a[words:] == GUARD_WORD).all()
    assert n.value == _expect("warp97", kc.PARAM_SETS[0])["count"]


def test_track_on_caller_given_points(ctx):
    prev, cur = CASES["warp97"]
    H, W = prev.shape
    ctx.set_klt(16, 2, 1, 1, 64)
    rng = np.random.default_rng(5)
    pts = np.concatenate([[[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W // 2, H // 2]],
                          np.column_stack([rng.integers(0, W, 27), rng.integers(0, H, 27)])]).astype(np.int32)
    for L, w, K in ((1, 1, 1), (2, 4, 10), (3, 7, 30)):
        want = ik.track(prev, cur, pts, L, w, K, 1, 64)
        np.testing.assert_array_equal(ctx.klt_track(prev, cur, pts, L, w, K), want, err_msg=f"L={L} w={w} K={K}")
    # the _dev form answers status 3 for a point outside the frame and reads nothing out of bounds; the host form refuses it
    outside = np.array([[-1, 5], [W, 5], [5, -1], [5, H], [-(2 ** 31), 2 ** 31 - 1], [2 ** 31 - 1, -(2 ** 31)]], np.int64).astype(np.int32)
    allpts = np.concatenate([pts, outside])
    _, dq, _, _, _ = _dev_forms(ctx, prev, cur, 0, 2, 4, 10, allpts)
    np.testing.assert_array_equal(dq[:len(pts)], ik.track(prev, cur, pts, 2, 4, 10, 1, 64))
    np.testing.assert_array_equal(dq[len(pts):], np.tile(np.array([0, 0, 0, ik.ST_LEFT], np.int32), (len(outside), 1)))
    with pytest.raises(OfpsHipError) as e:
        ctx.klt_track(prev, cur, outside[:1], 2, 4, 10)
    assert e.value.code == EINVAL
    assert ctx.klt_track(prev, cur, np.zeros((0, 2), np.int32), 2, 4, 10).shape == (0, 4)
    ctx.set_klt()


# ------------------------------------------------------------------------------------------------ large lattices
def _host_compaction(slots, W, H):
    kept = slots[slots[:, 5] == ik.ST_KEPT]
    return np.array([ik.record(int(s[0]), int(s[1]), int(s[3]), int(s[4]), W, H) for s in kept], np.float32).reshape(-1, 4)


# 1280 x 720 at cell 8: 14,400 slots, the one-workgroup compaction's many rounds; 1920 x 1096 at cell 8: 32,880 slots, above kCompactSmallMax
# = 32,768: the grid-wide compaction
@pytest.mark.parametrize("W,H", [(1280, 720), (1920, 1096)])
def test_large_lattice_records_are_the_raw_slots_compacted(ctx, W, H):
    tex = synth.random_luma(1, W + 8, H + 8, seed=synth.SEED0 + 9)[0]
    prev = np.ascontiguousarray(tex[4:4 + H, 4:4 + W])
    cur = np.ascontiguousarray(tex[2:2 + H, 5:5 + W])         # content moves by (-1, +2)
    prev[100:300, 200:500] = 128; cur[100:300, 200:500] = 128            # a flat patch: cells without a feature
    cur[400:500, 600:900] = tex[0:100, 0:300]                 # a repainted patch: residual losses
    ctx.set_klt(8, 1, 1, 1, 160)
    ns = ctx.klt_slot_count(W, H)
    assert ns == (W // 8) * (H // 8) and (ns > 32768) == (W == 1920)
    ent, slots = ctx.klt_flow(prev, cur, 2, 2, 5, want_slots=True)
    want = _host_compaction(slots, W, H)
    assert 0 < len(want) < ns and len(ent) == len(want)       # some slots are dropped: the compaction has something to do
    np.testing.assert_array_equal(_bits(ent), _bits(want))
    np.testing.assert_array_equal(slots[:, :3], ctx.klt_features(prev))
    ctx.set_klt()


# ------------------------------------------------------------------------------------------------ stream forms with the flag
SW, SH = 160, 96


@lru_cache(maxsize=None)
def _stream_frames():
    a, b = kc.warp_pair(SW, SH, (1.3, -0.6))
    c, _ = kc.warp_pair(SW, SH, (2.1, 0.7))
    return a, b, np.ascontiguousarray(b[:, ::-1]), c


def test_stream_forms_equal_the_stage_form(ctx):
    fr = _stream_frames()
    ctx.set_klt(16, 2, 1, 1, 160)
    ctx.lk_reset()
    kw = dict(levels=3, radius=4, iters=10, sparse=True)
    assert ctx.lk_push_frame(fr[0], **kw) is None             # a stream's first frame: have_vectors = 0
    for k in (1, 2, 3):
        ent, grid = ctx.lk_push_frame(fr[k], **kw)
        want = ctx.klt_flow(fr[k - 1], fr[k], 3, 4, 10)
        assert grid == (10, 6)
        np.testing.assert_array_equal(_bits(ent), _bits(want))
    # max_w / max_h are not looked at on full-size frames
    ent, grid = ctx.lk_decode(fr[0], fr[1], 3, 4, 10, max_w=0, max_h=0, sparse=True)
    np.testing.assert_array_equal(_bits(ent), _bits(ctx.klt_flow(fr[0], fr[1], 3, 4, 10)))
    # ofps_hip_lk_reset: the next frame starts a stream
    ctx.lk_reset()
    assert ctx.lk_push_frame(fr[1], **kw) is None
    ent, _ = ctx.lk_push_frame(fr[2], **kw)
    np.testing.assert_array_equal(_bits(ent), _bits(ctx.klt_flow(fr[1], fr[2], 3, 4, 10)))
    ctx.lk_reset(); ctx.set_klt()


def test_two_tickets_in_flight(ctx):
    fr = _stream_frames()
    ctx.set_klt(8, 2, 1, 1, 0)
    ctx.lk_reset()
    pinned = [ctx.pinned_frame(SH, SW) for _ in range(3)]
    kw = dict(levels=2, radius=4, iters=10, sparse=True)
    want = [None] + [ctx.klt_flow(fr[k - 1], fr[k], 2, 4, 10) for k in (1, 2, 3)]
    tickets = []
    got = []
    for k in range(4):
        np.copyto(pinned[k % 3], fr[k])
        tickets.append(ctx.lk_push_frame_async(pinned[k % 3], **kw))
        if len(tickets) == 2:
            got.append(ctx.lk_frame_wait(tickets.pop(0)))
    got.append(ctx.lk_frame_wait(tickets.pop(0)))
    assert got[0] is None
    for k in (1, 2, 3):
        ent, grid = got[k]
        assert grid == (20, 12)
        np.testing.assert_array_equal(_bits(ent), _bits(want[k]), err_msg=f"frame {k}")
    ctx.lk_reset(); ctx.set_klt()


def test_bgr_input_and_the_reduced_mode(ctx):
    fr = _stream_frames()
    rng = np.random.default_rng(3)
    bgr = [np.clip(f[..., None].astype(int) + rng.integers(-20, 21, (1, 1, 3)), 0, 255).astype(np.uint8) for f in fr[:2]]
    ctx.set_klt()
    gray = [ctx.cv_frontend(b, fmt=ctx.FMT_BGR) for b in bgr]
    ent, grid = ctx.lk_decode(bgr[0], bgr[1], 2, 4, 10, fmt=ctx.FMT_BGR, sparse=True)
    np.testing.assert_array_equal(_bits(ent), _bits(ctx.klt_flow(gray[0], gray[1], 2, 4, 10)))
    assert grid == (10, 6) and len(ent) > 0
    # OFPS_HIP_LK_REDUCED: every frame resized to the capped grid first, the tracker runs there
    big = kc.warp_pair(320, 192, (5.3, -4.6))
    small = [ctx.cv_frontend(f, reduced=True, max_w=100, max_h=100) for f in big]
    gw, gh = ctx.cv_grid(320, 192, 100, 100)
    assert small[0].shape == (gh, gw) and (gh >> 1) >= 8
    ctx.set_klt(8)
    ctx.lk_reset()
    assert ctx.lk_push_frame(big[0], 2, 4, 10, max_w=100, max_h=100, reduced=True, sparse=True) is None
    ent, grid = ctx.lk_push_frame(big[1], 2, 4, 10, max_w=100, max_h=100, reduced=True, sparse=True)
    assert grid == (-(-gw // 8), -(-gh // 8)) and len(ent) > 0
    np.testing.assert_array_equal(_bits(ent), _bits(ctx.klt_flow(small[0], small[1], 2, 4, 10)))
    ctx.lk_reset(); ctx.set_klt()


# ------------------------------------------------------------------------------------------------ fused form
@pytest.mark.parametrize("use_ransac", [False, True])
def test_fused_form(ctx, use_ransac):
    prev, cur = kc.warp_pair(320, 192, (5.3, -4.6))
    ctx.set_klt(16, 2, 1, 1, 160)
    ctx.lk_reset()
    tail = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1],
                use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200, seed=7)
    kw = dict(levels=4, radius=7, iters=10, sparse=True)
    first = ctx.lk_push_frame_fused(prev, **kw, **tail)
    assert not first["have_vectors"] and first["motion"] is None and first["quat"].tolist() == [1, 0, 0, 0]
    r = ctx.lk_push_frame_fused(cur, **kw, **tail)
    want = ctx.klt_flow(prev, cur, 4, 7, 10)
    assert r["have_vectors"] and r["n_vectors"] == len(want) and r["grid"] == (20, 12) and len(want) > 100
    np.testing.assert_array_equal(_bits(r["entries"]), _bits(want))
    np.testing.assert_array_equal(_bits(want), _bits(_expect("warp320", (16, 2, 1, 1, 160, 4, 7, 10))["records"]))     # and the restatement's
    det = ctx.detect(want, 0.05, 3, 0.003)
    assert (det is None) == (r["motion"] is None)
    if det is not None:
        assert det[0] == r["motion"][0]
        np.testing.assert_array_equal(_bits(det[1]), _bits(r["motion"][1]))
    q, _ = ctx.almeida(want, *CAM, use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200, seed=7)
    print("quaternion difference", np.abs(q - r["quat"]).max())
    assert np.abs(q - r["quat"]).max() <= QUAT_BOUND
    ctx.lk_reset(); ctx.set_klt()


def test_fused_form_with_detect_compensation(ctx):
    prev, cur = kc.warp_pair(320, 192, (5.3, -4.6))
    ctx.set_klt()
    ctx.lk_reset()
    ctx.set_detect_compensation(1)
    try:
        tail = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.0005, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1])
        kw = dict(levels=4, radius=7, iters=10, sparse=True)
        ctx.lk_push_frame_fused(prev, **kw, **tail)
        r = ctx.lk_push_frame_fused(cur, **kw, **tail)
    finally:
        ctx.set_detect_compensation(0)
    want = ctx.klt_flow(prev, cur, 4, 7, 10)
    np.testing.assert_array_equal(_bits(r["entries"]), _bits(want))       # the records handed back stay the raw ones
    det = ctx.detect(ctx.compensate(want, *CAM, r["quat"]), 0.05, 3, 0.0005)
    assert (det is None) == (r["motion"] is None)
    if det is not None:
        assert det[0] == r["motion"][0]
        np.testing.assert_array_equal(_bits(det[1]), _bits(r["motion"][1]))
    ctx.lk_reset()


def test_fused_form_on_a_flat_frame(ctx):
    prev, cur = kc.flat_pair(160, 96)
    ctx.set_klt()
    ctx.lk_reset()
    kw = dict(levels=2, radius=4, iters=10, sparse=True, aspect=CAM[0], fov_y_deg=CAM[1])
    ctx.lk_push_frame_fused(prev, **kw)
    for ransac in (False, True):
        r = ctx.lk_push_frame_fused(cur, use_ransac=ransac, **kw)
        assert r["have_vectors"] and r["n_vectors"] == 0 and r["motion"] is None and r["quat"].tolist() == [1, 0, 0, 0]
    ctx.lk_reset()


def test_fused_tickets_in_flight(ctx):
    """ofps_hip_lk_push_frame_fused_async with the flag: a ticket's tail reads its count on the device while the next ticket is pushed"""
    fr = _stream_frames()
    ctx.set_klt(8, 2, 1, 1, 0)
    ctx.lk_reset()
    pinned = [ctx.pinned_frame(SH, SW) for _ in range(3)]
    tail = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1])
    kw = dict(levels=2, radius=4, iters=10, sparse=True)
    tickets, got = [], []
    for k in range(4):
        np.copyto(pinned[k % 3], fr[k])
        tickets.append(ctx.lk_push_frame_fused_async(pinned[k % 3], **kw, **tail))
        if len(tickets) == 2:
            got.append(ctx.lk_frame_fused_wait(tickets.pop(0)))
    got.append(ctx.lk_frame_fused_wait(tickets.pop(0)))
    assert not got[0]["have_vectors"] and got[0]["quat"].tolist() == [1, 0, 0, 0]
    for k in (1, 2, 3):
        want = ctx.klt_flow(fr[k - 1], fr[k], 2, 4, 10)
        r = got[k]
        assert r["have_vectors"] and r["n_vectors"] == len(want) > 0 and r["grid"] == (20, 12), k
        np.testing.assert_array_equal(_bits(r["entries"]), _bits(want), err_msg=f"frame {k}")
        det = ctx.detect(want, 0.05, 3, 0.003)
        assert (det is None) == (r["motion"] is None), k
        if det is not None:
            assert det[0] == r["motion"][0]
            np.testing.assert_array_equal(_bits(det[1]), _bits(r["motion"][1]), err_msg=f"frame {k}")
        q, _ = ctx.almeida(want, *CAM)
        assert np.abs(q - r["quat"]).max() <= QUAT_BOUND, k
    ctx.lk_reset(); ctx.set_klt()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    prev, cur = CASES["warp96"]
    ctx.set_klt()

    def refused(fn, *a, **k):
        with pytest.raises(OfpsHipError) as e:
            fn(*a, **k)
        assert e.value.code == EINVAL, e.value

    for bad in (dict(cell=12), dict(cell=64), dict(score_radius=0), dict(score_radius=4), dict(min_score=0), dict(min_score=-5),
                dict(min_eig=0), dict(min_eig=65536), dict(max_residual=-1), dict(max_residual=4081)):
        refused(ctx.set_klt, **bad)
    assert ctx.get_klt() == dict(cell=16, score_radius=2, min_score=1, min_eig=1, max_residual=0)     # a refused call changes nothing
    for L, w, K in ((0, 4, 10), (7, 4, 10), (2, 0, 10), (2, 8, 10), (2, 4, 0), (2, 4, 31), (5, 4, 10)):   # 96 x 64 has no 5 levels of 8 x 8
        refused(ctx.klt_flow, prev, cur, L, w, K)
        refused(ctx.klt_track, prev, cur, np.array([[5, 5]]), L, w, K)
        refused(ctx.lk_decode, prev, cur, L, w, K, sparse=True)
    refused(ctx.klt_features, prev[:7])
    assert ctx.klt_slot_count(96, 64, 12) == 0 and ctx.klt_slot_count(97, 65, 16) == 35
    # the four excluded flag combinations, before anything is uploaded: the stream does not start
    ctx.lk_reset()
    for other in (dict(contrast_mask=True), dict(fullres_records=True), dict(farneback=True), dict(farneback=True, use_previous=True)):
        refused(ctx.lk_decode, prev, cur, 2, 4, 10, sparse=True, **other)
        refused(ctx.lk_push_frame, prev, 2, 4, 10, sparse=True, **other)
        refused(ctx.lk_push_frame_fused, prev, 2, 4, 10, sparse=True, **other)
    assert ctx.lk_push_frame(prev, 2, 4, 10, sparse=True) is None         # still the stream's first frame
    ctx.lk_reset()


# ------------------------------------------------------------------------------------------------ without the flag
def test_dense_decoders_without_the_flag_are_untouched(ctx):
    from ofps_amd.runtime import HipContext
    fr = synth.luma_sequence(2, 160, 96, max_step=2, seed=3)
    rng = np.random.default_rng(1)
    bgr = np.clip(synth.luma_sequence(2, 320, 180, max_step=3, seed=9)[..., None].astype(int) + rng.integers(-30, 31, (1, 180, 320, 3)), 0, 255).astype(np.uint8)
    fresh = HipContext(0)                                     # never sees a klt call
    try:
        ctx.set_klt(8, 3, 7, 9, 160)
        ctx.klt_flow(fr[0], fr[1], 2, 4, 10)
        a, ga = ctx.lk_decode(fr[0], fr[1], 3, 4, 3, contrast_mask=True)
        b, gb = fresh.lk_decode(fr[0], fr[1], 3, 4, 3, contrast_mask=True)
        assert ga == gb and len(a) > 0
        np.testing.assert_array_equal(_bits(a), _bits(b))
        a, ga = ctx.lk_decode(bgr[0], bgr[1], 5, 6, 3, contrast_mask=True, farneback=True, reduced=True, fmt=ctx.FMT_BGR)
        b, gb = fresh.lk_decode(bgr[0], bgr[1], 5, 6, 3, contrast_mask=True, farneback=True, reduced=True, fmt=ctx.FMT_BGR)
        assert ga == gb == (150, 84) and len(a) > 0
        np.testing.assert_array_equal(_bits(a), _bits(b))
    finally:
        fresh.close()
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ plugin
def test_plugin_properties_reach_the_context():
    from ofps_amd.plugins import HipKltDecoder
    prev, cur = kc.warp_pair(160, 96, (1.3, -0.6))
    dec = HipKltDecoder(iter([prev, cur]))
    try:
        names = [p[0] for p in dec.props()]
        for want in ("Cell size", "Score radius", "Min score", "Min eigenvalue", "Max residual", "Levels", "Window radius", "Iterations"):
            assert want in names
        for name, value in (("Cell size", 8), ("Score radius", 3), ("Min score", 5), ("Min eigenvalue", 2), ("Max residual", 160), ("Levels", 2),
                            ("Window radius", 4), ("Iterations", 10)):
            assert dec.set_prop(name, value)
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt() == dict(cell=8, score_radius=3, min_score=5, min_eig=2, max_residual=160)
        want = dec.ctx.klt_flow(prev, cur, 2, 4, 10)
        assert len(field) == len(want) > 0
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(want))
        with pytest.raises(EOFError):
            dec.process_frame(field)
    finally:
        dec.ctx.close()


# ------------------------------------------------------------------------------------------------ C++ host
def test_cpp_host_decoder_by_name(ctx, tmp_path):
    import os
    import subprocess
    import json
    from ofps_amd import mvec
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ofps_amd", "host", "ofps_hip_tool")
    fr = _stream_frames()
    raw = tmp_path / "clip.y"
    raw.write_bytes(b"".join(f.tobytes() for f in fr))
    out = tmp_path / "clip_klt.mvec"
    arg = f"{raw}?w={SW}&h={SH}&fps=30"
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "4", "Levels=3", "Window radius=4", "Min eigenvalue=2", "Cell size=8@2",
                        "Cell size=16@3"], check=True, capture_output=True, text=True)
    frames = list(mvec.read_frames(open(out, "rb")))
    assert json.loads(p.stdout)["frames"] == 4 == len(frames) and len(frames[0]) == 0
    for k, cell in ((1, 16), (2, 8), (3, 16)):
        ctx.set_klt(cell, 2, 1, 2, 0)
        want = ctx.klt_flow(fr[k - 1], fr[k], 3, 4, 10)
        assert len(want) > 0, k
        np.testing.assert_array_equal(_bits(frames[k]), _bits(want), err_msg=f"frame {k}")
    ctx.set_klt()
    for loop in ("detect", "track"):                          # the detect and track loops take the decoder by the same name
        subprocess.run([tool, loop, "hip_klt", arg] + (["3"] if loop == "detect" else []), check=True, capture_output=True, text=True)
