"""-m gpu: hip_klt's mean removal (include/ofps_hip.h N3m) through the C ABI, bit for bit against the restatement tests/indep_klt_zm.py: the
stage forms (ofps_hip_klt_track / _flow, host and _dev) on the cases of tests/klt_zm_cases.py with guard words behind every output; the
batch form in chain and key mode against one-pair calls and the restatement; the fused sparse form of the dense decoders' stream against
ofps_hip_klt_flow + ofps_hip_detect + ofps_hip_almeida; the batched stream and two multi-device workers against the single-context stream;
the plugin and the C++ host by name; the setting switched off against a context that never saw the setter; the refusals.  Every comparison
is bit for bit but the quaternion's (2e-6, the bound of the existing fused tests).  Expectations are computed once per process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import indep_klt as ik
import indep_klt_zm as iz
import klt_batch_cases as bc
import klt_cases as kc
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
    c.set_klt_mean_removal(1)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
    """the two _dev forms that track, on frames with `pad` bytes of row padding -> (quads of `points`, records, count, slots)"""
    H, W = prev.shape
    ns = ctx.klt_slot_count(W, H)
    dp, stride = _dev_frame(ctx, prev, pad)
    dc, _ = _dev_frame(ctx, cur, pad)
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
    b_pts, b_quad = _DevBuf(ctx, max(2 * len(pts), 1), pts if len(pts) else None), _DevBuf(ctx, max(4 * len(pts), 1))
    b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns)
    try:
        ctx.klt_track_dev(dp, dc, W, H, stride, b_pts.ptr, len(pts), L, w, K, b_quad.ptr)
        ctx.klt_flow_dev(dp, dc, W, H, stride, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        count = int(b_cnt.read(np.uint32)[0])
        return (b_quad.read(np.int32)[:4 * len(pts)].reshape(-1, 4), b_rec.read(np.float32).reshape(-1, 4)[:count], count,
                b_slots.read(np.int32).reshape(-1, 6))
    finally:
        for b in (b_pts, b_quad, b_rec, b_cnt, b_slots):
            b.free()
        ctx.free(dp); ctx.free(dc)


def _check_stage_forms(ctx, name, params, pad=0):
    """host and _dev forms of _flow and _track on one case and parameter set against the restatement"""
    prev, cur = zc.case(name)
    exp = zc.expect(name, params)
    L, w, K = _set(ctx, params)
    what = f"{name} {params} pad {pad}"
    stride = None
    pv, cv = prev, cur
    if pad:
        (pv, stride), (cv, _) = kc.padded(prev, pad), kc.padded(cur, pad)
    ent, slots = ctx.klt_flow(pv, cv, L, w, K, want_slots=True, stride=stride)
    np.testing.assert_array_equal(slots, exp["slots"], err_msg=what + ": slots")
    assert len(ent) == exp["count"], what
    np.testing.assert_array_equal(_bits(ent), _bits(exp["records"]), err_msg=what + ": record bits")
    pts, quads = _quads_of(exp)
    np.testing.assert_array_equal(ctx.klt_track(pv, cv, pts, L, w, K, stride=stride), quads, err_msg=what + ": quadruples")
    dq, drec, dcount, dslots = _dev_forms(ctx, prev, cur, pad, L, w, K, pts)
    np.testing.assert_array_equal(dq, quads, err_msg=what + ": track_dev")
    np.testing.assert_array_equal(dslots, exp["slots"], err_msg=what + ": flow_dev slots")
    assert dcount == exp["count"], what
    np.testing.assert_array_equal(_bits(drec), _bits(exp["records"]), err_msg=what + ": flow_dev record bits")
    return slots


# ------------------------------------------------------------------------------------------------ stage forms against the restatement
@pytest.mark.parametrize("name", zc.SMALL_NAMES)
def test_stage_forms_match_the_restatement(ctx, name):
    """the seven small cases x PARAM_SETS: w = 1, 4, 7, L = 1 .. 4, K = 1, 10, 30"""
    try:
        for params in kc.PARAM_SETS:
            _check_stage_forms(ctx, name, params)
    finally:
        ctx.set_klt()


@pytest.mark.parametrize("offset", zc.RELIT_OFFSETS)
def test_relit_pair_with_clipped_pixels(ctx, offset):
    prev, cur = zc.case(f"warp96{offset:+d}")
    assert (cur == 255).any() if offset > 0 else (cur == 0).any()         # pixels clip: the exact invariance does not hold, the definition does
    try:
        for params in (zc.SET0, zc.SET0_R64):
            _check_stage_forms(ctx, f"warp96{offset:+d}", params)
    finally:
        ctx.set_klt()


def test_an_offset_that_clips_no_pixel_changes_no_slot(ctx):
    try:
        base = _check_stage_forms(ctx, "inv", zc.SET0_R64)
        assert (base[:, 5] == ik.ST_KEPT).all()
        for o in zc.INVARIANT_OFFSETS:
            np.testing.assert_array_equal(_check_stage_forms(ctx, f"inv{o:+d}", zc.SET0_R64), base, err_msg=str(o))
    finally:
        ctx.set_klt()


@pytest.mark.parametrize("params", [kc.DEFAULT_SET, R160], ids=["R0", "R160"])
def test_decoder_defaults_on_the_relit_320_pair(ctx, params):
    try:
        slots = _check_stage_forms(ctx, "warp320+20", params)
        assert (slots[:, 5] == ik.ST_KEPT).sum() > 150
    finally:
        ctx.set_klt()


@pytest.mark.parametrize("pad", [12, 13])
def test_padded_rows(ctx, pad):
    try:
        _check_stage_forms(ctx, "warp97+20", zc.SET0_R64, pad)
    finally:
        ctx.set_klt()


def test_host_forms_leave_the_words_behind_their_outputs_alone(ctx):
    prev, cur = zc.case("warp97+20")
    H, W = prev.shape
    ctx.set_klt()
    ns = ctx.klt_slot_count(W, H)
    lib, h = ctx._lib, ctx._h
    u8, i32, f32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ent = np.full(4 * ns + GUARD, GUARD_WORD, np.uint32)
    slots = np.full(6 * ns + GUARD, GUARD_WORD, np.uint32)
    pts = np.array([[10, 10], [40, 30], [96, 64]], np.int32)
    quads = np.full(4 * len(pts) + GUARD, GUARD_WORD, np.uint32)
    n = C.c_uint32(0)
    p, c = np.ascontiguousarray(prev), np.ascontiguousarray(cur)
    assert lib.ofps_hip_klt_flow(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, 2, 4, 10, ent.ctypes.data_as(f32), C.byref(n),
                                 slots.ctypes.data_as(i32)) == 0
    assert lib.ofps_hip_klt_track(h, p.ctypes.data_as(u8), c.ctypes.data_as(u8), W, H, W, pts.ctypes.data_as(i32), len(pts), 2, 4, 10,
                                  quads.ctypes.data_as(i32)) == 0
    for a, words in ((ent, 4 * ns), (slots, 6 * ns), (quads, 4 * len(pts))):
        assert (a[words:] == GUARD_WORD).all()
    exp = zc.expect("warp97+20", zc.SET0)
    assert n.value == exp["count"]
    np.testing.assert_array_equal(slots[:6 * ns].view(np.int32).reshape(-1, 6), exp["slots"])
    np.testing.assert_array_equal(quads[:4 * len(pts)].view(np.int32).reshape(-1, 4), iz.track(prev, cur, pts, 2, 4, 10))


def test_track_on_caller_given_points(ctx):
    prev, cur = zc.case("warp97+20")
    H, W = prev.shape
    ctx.set_klt(16, 2, 1, 1, 64)
    try:
        rng = np.random.default_rng(5)
        pts = np.concatenate([[[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W // 2, H // 2]],
                              np.column_stack([rng.integers(0, W, 27), rng.integers(0, H, 27)])]).astype(np.int32)
        for L, w, K in ((1, 1, 1), (2, 4, 10), (3, 7, 30)):
            want = iz.track(prev, cur, pts, L, w, K, 1, 64)
            np.testing.assert_array_equal(ctx.klt_track(prev, cur, pts, L, w, K), want, err_msg=f"L={L} w={w} K={K}")
        # the _dev form answers status 3 for a point outside the frame and reads nothing out of bounds; the host form refuses it
        outside = np.array([[-1, 5], [W, 5], [5, -1], [5, H], [-(2 ** 31), 2 ** 31 - 1], [2 ** 31 - 1, -(2 ** 31)]], np.int64).astype(np.int32)
        allpts = np.concatenate([pts, outside])
        dq, _, _, _ = _dev_forms(ctx, prev, cur, 0, 2, 4, 10, allpts)
        np.testing.assert_array_equal(dq[:len(pts)], iz.track(prev, cur, pts, 2, 4, 10, 1, 64))
        np.testing.assert_array_equal(dq[len(pts):], np.tile(np.array([0, 0, 0, ik.ST_LEFT], np.int32), (len(outside), 1)))
        with pytest.raises(OfpsHipError) as e:
            ctx.klt_track(prev, cur, outside[:1], 2, 4, 10)
        assert e.value.code == EINVAL
    finally:
        ctx.set_klt()


def test_features_do_not_change(ctx):
    prev, _ = zc.case("warp97+20")
    ctx.set_klt()
    np.testing.assert_array_equal(ctx.klt_features(prev), zc.expect("warp97+20", zc.SET0)["features"])


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


@pytest.mark.parametrize("ref_mode", [0, 1], ids=["chain", "key"])
def test_batch_form_on_the_flicker_sequence(ctx, ref_mode):
    fr = zc.flicker_sequence()
    params = zc.SET0_R64 if ref_mode else zc.SET0
    L, w, K = _set(ctx, params)
    try:
        restated = [(e["records"], int(e["count"]), e["slots"]) for e in zc.flicker_expect(params, ref_mode)]
        pairs = []
        for k in range(len(fr) - 1):
            a, b = bc.pair_of(k, ref_mode)
            ent, slots = ctx.klt_flow(fr[a], fr[b], L, w, K, want_slots=True)
            pairs.append((ent, len(ent), slots))
        for want, what in ((restated, "restatement"), (pairs, "one-pair calls")):
            _check_items(_batch_dev(ctx, fr, ref_mode, L, w, K), want, f"dev, {what}")
            _check_items(ctx.klt_flow_batch(fr, L, w, K, ref_mode=ref_mode, want_slots=True), want, f"host, {what}")
    finally:
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ fused sparse form
@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
def test_fused_sparse_form(ctx, use_ransac):
    fr = zc.flicker_sequence()
    L, w, K = _set(ctx, zc.SET0)
    tail = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1],
                use_ransac=use_ransac, num_iters=64, inlier_deg=0.05, num_samples=200)
    try:
        ctx.lk_reset()
        first = ctx.lk_push_frame_fused(np.ascontiguousarray(fr[0]), L, w, K, sparse=True, seed=SEED, **tail)
        assert not first["have_vectors"]
        restated = zc.flicker_expect(zc.SET0)
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
        ctx.lk_reset(); ctx.set_klt()


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
    fr = zc.flicker_sequence()
    L, w, K = _set(ctx, zc.SET0)
    try:
        single = _single_stream(ctx, fr, L, w, K)
        batched = _batched_stream(ctx, fr, (3, 3), L, w, K)
    finally:
        ctx.set_klt()
    restated = zc.flicker_expect(zc.SET0)
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
    cell, r, min_score, min_eig, R, _, _, _ = zc.SET0
    env = dict(os.environ, OFPS_HIP_BATCH_DECODER="1", OFPS_HIP_KLT_MEAN_REMOVAL="1", OFPS_HIP_KLT_CELL=str(cell), OFPS_HIP_KLT_SCORE_RADIUS=str(r),
               OFPS_HIP_KLT_MIN_SCORE=str(min_score), OFPS_HIP_KLT_MIN_EIG=str(min_eig), OFPS_HIP_KLT_MAX_RESIDUAL=str(R), OFPS_HIP_KLT_LEVELS=str(L),
               OFPS_HIP_KLT_RADIUS=str(w), OFPS_HIP_KLT_ITERS=str(K), KLT_CHILD_SEED=str(SEED))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_klt_zm_child.py")], env=env, capture_output=True, text=True, timeout=120)
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
    assert ctx.get_klt_mean_removal() == 1
    ctx.set_option("OFPS_HIP_KLT_MEAN_REMOVAL", 0)
    assert ctx.get_klt_mean_removal() == 0
    ctx.set_option("OFPS_HIP_KLT_MEAN_REMOVAL", 1)
    assert ctx.get_klt_mean_removal() == 1
    ctx.set_option("OFPS_HIP_KLT_MEAN_REMOVAL", None)
    assert ctx.get_klt_mean_removal() == 0                     # the default
    ctx.set_klt_mean_removal(1)
    code = ("import sys; sys.path.insert(0, %r); from ofps_amd.runtime import HipContext; c = HipContext(0); "
            "print(c.get_klt_mean_removal()); c.close()" % ROOT)
    for value, want in (("1", 1), ("0", 0), ("yes", 0)):       # a malformed variable is reported once and ignored
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OFPS_HIP_KLT_MEAN_REMOVAL=value), capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert int(p.stdout.strip().splitlines()[-1]) == want, value
        assert ("OFPS_HIP_KLT_MEAN_REMOVAL" in p.stderr) == (value == "yes")


# ------------------------------------------------------------------------------------------------ plugin and C++ host
def test_plugin_property_reaches_the_context():
    from ofps_amd.plugins import HipKltDecoder
    fr = zc.flicker_sequence()
    dec = HipKltDecoder(iter([fr[0], fr[1], fr[2]]))
    try:
        assert ("Mean removal", "bool", False, None, None) in dec.props()
        for name, value in (("Levels", 2), ("Window radius", 4), ("Iterations", 10)):
            assert dec.set_prop(name, value)
        assert dec.set_prop("Mean removal", True)
        assert ("Mean removal", "bool", True, None, None) in dec.props()
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt_mean_removal() == 1
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(zc.flicker_expect(zc.SET0)[0]["records"]))
        assert dec.set_prop("Mean removal", False)             # and back: the next pair is the plain tracker's
        field = []
        assert dec.process_frame(field) is True
        assert dec.ctx.get_klt_mean_removal() == 0
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(zc.flicker_expect(zc.SET0, 0, False)[1]["records"]))
    finally:
        dec.ctx.close()


def test_cpp_host_property_by_name(tmp_path):
    from ofps_amd import mvec
    tool = os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool")
    fr = zc.flicker_sequence()
    raw = tmp_path / "clip.y"
    raw.write_bytes(b"".join(np.ascontiguousarray(f).tobytes() for f in fr[:4]))
    out = tmp_path / "clip_klt.mvec"
    arg = f"{raw}?w=128&h=96&fps=30"
    # on for frames 1 and 2, off before frame 3 is read
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "4", "Levels=2", "Window radius=4", "Mean removal=true", "Mean removal=false@3"],
                       check=True, capture_output=True, text=True, timeout=120)
    frames = list(mvec.read_frames(open(out, "rb")))
    assert json.loads(p.stdout)["frames"] == 4 == len(frames) and len(frames[0]) == 0
    zm, plain = zc.flicker_expect(zc.SET0), zc.flicker_expect(zc.SET0, 0, False)
    for k, want in ((1, zm[0]), (2, zm[1]), (3, plain[2])):
        np.testing.assert_array_equal(_bits(frames[k]), _bits(want["records"]), err_msg=f"frame {k}")
    assert zm[2]["records"].tobytes() != plain[2]["records"].tobytes()
    p = subprocess.run([tool, "extract", "hip_klt", arg, str(out), "2", "Mean removal=maybe", "No such property=1"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "No such property" in p.stderr
    # a saved configuration carries it like every other property
    cfg = {"decoder": [{"selected_plugin": "hip_klt", "arg": arg, "extra": False}, True],
           "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": None}, True],
           "settings": {"worker": {"decoder_properties": {"Mean removal": {"Bool": True}, "Levels": {"Usize": {"val": 2, "min": 1, "max": 6}}},
                                   "realtime_processing": False, "detector_properties": {}},
                        "overlay_mf": False, "max_frame_gap": 3, "min_frames": 1, "draw_perf_stats": {"summary_window": False, "graph_window": False}}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    got = json.loads(subprocess.run([tool, "parse-config", str(path)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert got["decoder_properties"]["Mean removal"] == ["Bool", True]
    det = json.loads(subprocess.run([tool, "detect", "--config", str(path)], check=True, capture_output=True, text=True, timeout=120)
                     .stdout.strip().splitlines()[-1])
    assert det["frames"] == 4
    # the stream benchmark's flag
    r = json.loads(subprocess.run([tool, "stream-bench", "128", "96", "12", "batch", "3", "--klt", "--klt-mean-removal"], check=True, capture_output=True,
                                  text=True, timeout=120).stdout.strip().splitlines()[-1])
    assert r["decoder"] == "hip_klt" and r["mean_removal"] == 1 and 0 < r["last_n_vectors"] <= 48


# ------------------------------------------------------------------------------------------------ feature off
def _off_answers(c):
    """klt_flow, the batch form and a push_frames_async ticket on the flicker sequence, as bytes"""
    fr = zc.flicker_sequence()
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
    fr = zc.flicker_sequence()
    assert ctx.get_klt_mean_removal() == 1
    on = _off_answers(ctx)                                     # calls with the setting on
    ctx.set_klt_mean_removal(0)
    fresh = HipContext(0)
    try:
        assert fresh.get_klt_mean_removal() == 0
        off, want = _off_answers(ctx), _off_answers(fresh)
        assert off == want
        assert on[1] != off[1] and on[4] != off[4]             # and the setting did something
        plain = zc.flicker_expect(zc.SET0_R64, 0, False)
        np.testing.assert_array_equal(np.frombuffer(off[1], np.int32).reshape(-1, 6), plain[0]["slots"])
    finally:
        fresh.close()
        ctx.set_klt_mean_removal(1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    assert ctx.get_klt_mean_removal() == 1

    def valid():
        _check_stage_forms(ctx, "warp96+20", zc.SET0_R64)

    try:
        for bad in (2, -1):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_klt_mean_removal(bad)
            assert e.value.code == EINVAL, bad
            assert ctx.get_klt_mean_removal() == 1, bad        # the setting stays as it was
            valid()
        for bad in ("on", "2", "-1", "1x"):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_option("OFPS_HIP_KLT_MEAN_REMOVAL", bad)
            assert e.value.code == EINVAL, bad
            assert ctx.get_klt_mean_removal() == 1, bad
        valid()
        assert ctx._lib.ofps_hip_set_klt_mean_removal(None, 1) == EINVAL and ctx._lib.ofps_hip_get_klt_mean_removal(None) == EINVAL
    finally:
        ctx.set_klt()
