"""-m gpu: hip_sad's mean removal (include/ofps_hip.h N1m) through the C ABI, bit-exact against the restatement
tests/indep_sad_prefilter.py throughout: the filter alone (host and _dev forms), the whole search on the relit scenes through every
single-context entry point, its composition with PRUNED mode, the quarter-pel refinement, the search levels and their predictors, the
contrast gate, the consistency check and the fused per-frame path, one multi-device child process, radius 0 after radius 4, the errors and
the plugin property.  Inputs and expectations: tests/sad_prefilter_cases.py (shared, computed once, read-only)."""
import json
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from ofps_amd import _lib
from ofps_amd._lib import OfpsHipError

import indep_sad_hier as ih
import indep_sad_pred as ipred
import indep_sad_prefilter as ip
import indep_sad_qpel as iq
import sad_consistency_cases as cc
import sad_gate_cases as gc
import sad_prefilter_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6                                         # the fused path's documented parity with ofps_hip_almeida (include/ofps_hip.h N1g)
R4 = pc.RADIUS


@pytest.fixture()
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(ent_g, best_g, ent_e, best_e, what=""):
    np.testing.assert_array_equal(best_g, best_e, err_msg=what)
    np.testing.assert_array_equal(_bits(ent_g), _bits(ent_e), err_msg=what)


# ---------------------------------------------------------------- the filter alone
@lru_cache(maxsize=64)
def _filter_expect(kind, W, H, stride, r):
    f = pc.filter_frame(kind, W, H, stride)
    want = ip.prefilter(f[:, :W], r)
    want.setflags(write=False)
    return f, want


@pytest.mark.parametrize("r", pc.FILTER_RADII)
@pytest.mark.parametrize("W,H,stride", pc.FILTER_SIZES)
def test_filter_matches_the_restatement(ctx, W, H, stride, r):
    for kind in pc.FILTER_KINDS:
        f, want = _filter_expect(kind, W, H, stride, r)
        np.testing.assert_array_equal(ctx.sad_prefilter(f[:, :W], r, stride=stride), want, err_msg=f"{kind}, strided")
        np.testing.assert_array_equal(ctx.sad_prefilter(f[:, :W].copy(), r), want, err_msg=f"{kind}, dense")


def _filter_dev(ctx, src, W, H, stride, r, dst_stride, frames=1, pitch=None, dst_pitch=None):
    """`frames` frames of `src` (a flat byte buffer) through ofps_hip_sad_prefilter_dev -> the whole destination buffer, 0xA5 where untouched"""
    pitch = pitch or stride * H
    dst_pitch = dst_pitch or dst_stride * H
    guard = np.full(frames * dst_pitch + 64, 0xA5, np.uint8)
    d_src, d_dst = ctx.malloc(src.nbytes), ctx.malloc(guard.nbytes)
    try:
        ctx.memcpy_h2d(d_src, src); ctx.memcpy_h2d(d_dst, guard)
        for k in range(frames):
            ctx.sad_prefilter_dev(d_src + k * pitch, W, H, stride, r, d_dst + k * dst_pitch, dst_stride)
        ctx.sync()
        out = np.zeros_like(guard)
        ctx.memcpy_d2h(out, d_dst)
    finally:
        ctx.free(d_src); ctx.free(d_dst)
    return out


@pytest.mark.parametrize("r", pc.FILTER_RADII)
@pytest.mark.parametrize("W,H,stride", pc.FILTER_SIZES)
def test_filter_dev_into_a_dense_destination_writes_nothing_beside_it(ctx, W, H, stride, r):
    """dst_stride = W: for the odd widths neither side's rows are 4-byte aligned (the byte forms of loads and stores)"""
    for kind in ("random", "blocks3"):
        f, want = _filter_expect(kind, W, H, stride, r)
        out = _filter_dev(ctx, np.ascontiguousarray(f).reshape(-1), W, H, stride, r, W)
        np.testing.assert_array_equal(out[:W * H].reshape(H, W), want, err_msg=kind)
        assert (out[W * H:] == 0xA5).all()


@pytest.mark.parametrize("r", pc.FILTER_RADII)
def test_filter_dev_batch_of_three_with_a_pitch_larger_than_a_frame(ctx, r):
    """37 x 23 at a device stride of 40 (rows 4-byte aligned: the dword forms), frames 40 * 23 + 24 bytes apart on both sides"""
    W, H, stride = 37, 23, 40
    pitch = stride * H + 24
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, 3 * pitch, dtype=np.uint8)                 # junk in the stride margin and between the frames
    out = _filter_dev(ctx, src, W, H, stride, r, stride, frames=3, pitch=pitch, dst_pitch=pitch)
    for k in range(3):
        fr = src[k * pitch:k * pitch + stride * H].reshape(H, stride)
        got = out[k * pitch:k * pitch + stride * H].reshape(H, stride)
        np.testing.assert_array_equal(got[:, :W], ip.prefilter(fr[:, :W], r), err_msg=f"frame {k}")
        assert (got[:, W:] == 0xA5).all() and (out[k * pitch + stride * H:(k + 1) * pitch] == 0xA5).all()


# ---------------------------------------------------------------- the whole search on the relit scenes
@pytest.mark.parametrize("lighting", ["step", "ramp"])
@pytest.mark.parametrize("i", range(len(pc.SCENES)))
def test_relit_scene_through_sad_flow(ctx, i, lighting):
    W, H, B, R, d = pc.SCENES[i]
    prev, cur = pc.relit_pair(W, H, d, lighting)
    plain_g = ctx.sad_flow(prev, cur, B, R, want_best=True)
    _same(*plain_g, *pc.expect(i, lighting, 0), "radius 0")
    ctx.set_sad_prefilter(R4)
    assert ctx.get_sad_prefilter() == R4
    ent_g, best_g = ctx.sad_flow(prev, cur, B, R, want_best=True)
    _same(ent_g, best_g, *pc.expect(i, lighting, R4), f"radius {R4}")
    inner = pc.interior(W, H, B, d, R4)
    print(f"scene {i} {lighting}: {int((pc.hits(best_g, d) & inner).sum())} of {int(inner.sum())} interior blocks return d, "
          f"the plain search {int((pc.hits(plain_g[1], d) & inner).sum())}")
    assert not (inner & ~pc.hits(best_g, d)).any()
    assert int((pc.hits(plain_g[1], d) & inner).sum()) <= pc.PLAIN_AT_MOST[(i, lighting)]
    # the SAD field is the SAD of the FILTERED blocks
    Fp, Fc = pc.filtered_pair(W, H, d, lighting, R4)
    k = int(np.flatnonzero(inner)[0]); x0, y0 = (k % (W // B)) * B, (k // (W // B)) * B
    dx, dy, sad = (int(v) for v in best_g[k])
    assert sad == int(np.abs(Fc[y0:y0 + B, x0:x0 + B].astype(np.int64) - Fp[y0 + dy:y0 + dy + B, x0 + dx:x0 + dx + B].astype(np.int64)).sum())


def _dev_run(ctx, fr, stride, ref_mode, B, R, with_best=True):
    n, H, W = fr.shape
    buf = np.random.default_rng(3).integers(0, 256, (n, H, stride), dtype=np.uint8); buf[:, :, :W] = fr      # junk in the stride margin
    nblk = (W // B) * (H // B)
    d_fr, d_ent, d_best = ctx.malloc(buf.nbytes), ctx.malloc((n - 1) * nblk * 16), ctx.malloc((n - 1) * nblk * 12)
    try:
        ctx.memcpy_h2d(d_fr, buf)
        ctx.sad_flow_dev(d_fr, n, W, H, stride, stride * H, ref_mode, B, R, d_ent, d_best if with_best else None)
        ent = np.zeros((n - 1, nblk, 4), np.float32); best = np.zeros((n - 1, nblk, 3), np.int32)
        ctx.memcpy_d2h(ent, d_ent)
        if with_best:
            ctx.memcpy_d2h(best, d_best)
    finally:
        for p in (d_fr, d_ent, d_best):
            ctx.free(p)
    return ent, best


@pytest.mark.parametrize("ref_mode", [0, 1])
def test_sad_flow_dev_three_frames(ctx, ref_mode):
    f = pc.sequence()[:3]
    ctx.set_sad_prefilter(R4)
    for stride, with_best in ((pc.SEQ_W, True), (pc.SEQ_W + 4, False)):                 # 64-byte rows; rows only 4-byte aligned, no out_best
        ent, best = _dev_run(ctx, f, stride, ref_mode, pc.SEQ_B, pc.SEQ_R, with_best)
        for k in range(2):
            ent_e, best_e = pc.sequence_expect(0 if ref_mode else k, k + 1)
            np.testing.assert_array_equal(_bits(ent[k]), _bits(ent_e), err_msg=f"stride {stride} pair {k}")
            if with_best:
                np.testing.assert_array_equal(best[k], best_e)


def test_pruned_mode_equals_exhaustive(ctx):
    """block 16, range 16: the geometry PRUNED applies to"""
    W, H, B, _, d = pc.SCENES[0]
    prev, cur = pc.relit_pair(W, H, d, "step")
    ent_e, best_e = ip.search(prev, cur, 16, 16, R4)
    ctx.set_sad_prefilter(R4)
    _same(*ctx.sad_flow(prev, cur, 16, 16, want_best=True), ent_e, best_e, "exhaustive")
    ctx.set_sad_mode(ctx.SAD_PRUNED)
    _same(*ctx.sad_flow(prev, cur, 16, 16, want_best=True), ent_e, best_e, "pruned")


def test_quarter_pel_interpolates_the_filtered_frames(ctx):
    ctx.set_sad_prefilter(R4); ctx.set_sad_motion_scale(4)
    for i, lighting in ((0, "step"), (1, "ramp")):
        W, H, B, R, d = pc.SCENES[i]
        prev, cur = pc.relit_pair(W, H, d, lighting)
        Fp, Fc = pc.filtered_pair(W, H, d, lighting, R4)
        ent_e, best_e = iq.refine(Fp, Fc, B, R, pc.expect(i, lighting, R4)[1])
        _same(*ctx.sad_flow(prev, cur, B, R, want_best=True), ent_e, best_e, f"scene {i}")
    # without out_best the integer winners live in the context's own scratch
    f = pc.sequence()
    Fa, Fb = ip.prefilter(f[0], R4), ip.prefilter(f[1], R4)
    ent, _ = _dev_run(ctx, f[:2], pc.SEQ_W, 0, pc.SEQ_B, pc.SEQ_R, with_best=False)
    np.testing.assert_array_equal(_bits(ent[0]), _bits(iq.refine(Fa, Fb, pc.SEQ_B, pc.SEQ_R, pc.sequence_expect(0, 1)[1])[0]))


def _top(prev, cur, B, R):
    return ip.full_search(prev, cur, B, R)


@pytest.mark.parametrize("predictors", [0, 1])
def test_search_levels_build_their_pyramid_from_the_filtered_frames(ctx, predictors):
    W, H, B, R, levels, d = pc.BEYOND
    prev, cur = pc.relit_pair(W, H, d, "step")
    Fp, Fc = ip.prefilter(prev, R4), ip.prefilter(cur, R4)
    if predictors:
        ent_e, best_e = ipred.search(Fp, Fc, B, R, levels, 1, top=_top)[:2]
    else:
        ent_e, best_e, _ = ih.search(Fp, Fc, B, R, levels, top=_top)
    ctx.set_sad_prefilter(R4); ctx.set_sad_levels(levels); ctx.set_sad_predictors(predictors)
    ent_g, best_g = ctx.sad_flow(prev, cur, B, R, want_best=True)
    _same(ent_g, best_g, ent_e, best_e)
    ctx.set_sad_prefilter(0)
    raw = ctx.sad_flow(prev, cur, B, R, want_best=True)[1]
    inner = pc.interior(W, H, B, d, 2 * R4 + 2)                                          # the window of the halved level, and its rounding
    print(f"predictors {predictors}: {int((pc.hits(best_g, d) & inner).sum())} of {int(inner.sum())} interior blocks return d, "
          f"without mean removal {int((pc.hits(raw, d) & inner).sum())}")
    assert int((pc.hits(best_g, d) & inner).sum()) > int((pc.hits(raw, d) & inner).sum())


@pytest.mark.parametrize("gate", [1, pc.SEQ_B * pc.SEQ_B])
def test_checked_dev_counts_the_gate_on_the_raw_frame(ctx, gate):
    """gate + limit 1 on pair (1, 2) of the sequence: the consistency check compares the two directions' winners on the filtered pair, the
    contrast gate counts mask pixels of the UNFILTERED current frame.  Gate 1 keeps every block of this texture; at gate B * B the raw and
    the filtered frame's flags differ, and so do the kept sets"""
    f = pc.sequence()
    W, H, B, R = pc.SEQ_W, pc.SEQ_H, pc.SEQ_B, pc.SEQ_R
    ent0, F = pc.sequence_expect(1, 2)
    G = pc.sequence_expect(2, 1)[1]
    round_trip = cc.keep_flags(F, G, W, H, B, 1)
    gate_raw = gc.keep_flags(f[2], B, gate)
    gate_filtered = gc.keep_flags(ip.prefilter(f[2], R4), B, gate)
    keep = round_trip & gate_raw
    print(f"gate {gate}: kept {int(keep.sum())} of {pc.SEQ_NBLK}; the gate alone keeps {int(gate_raw.sum())} on the raw frame, "
          f"{int(gate_filtered.sum())} on the filtered one")
    if gate > 1:
        assert not np.array_equal(keep, round_trip & gate_filtered)                      # the case tells the two frames apart
    pair = np.ascontiguousarray(f[1:3])
    ctx.set_sad_prefilter(R4)
    d = [ctx.malloc(pair.nbytes), ctx.malloc(pc.SEQ_NBLK * 16), ctx.malloc(pc.SEQ_NBLK * 12), ctx.malloc(16)]
    try:
        ctx.memcpy_h2d(d[0], pair)
        ctx.sad_flow_checked_dev(d[0], d[0] + W * H, W, H, W, B, R, gate, 1, d[1], d[2], d[3])
        ctx.sync()
        ent = np.zeros((pc.SEQ_NBLK, 4), np.float32); best = np.zeros((pc.SEQ_NBLK, 3), np.int32); cnt = np.zeros(4, np.uint32)
        ctx.memcpy_d2h(ent, d[1]); ctx.memcpy_d2h(best, d[2]); ctx.memcpy_d2h(cnt, d[3])
    finally:
        for p in d:
            ctx.free(p)
    n = int(cnt[0])
    assert n == int(keep.sum())
    np.testing.assert_array_equal(_bits(ent[:n]), _bits(cc.check_filter(ent0, keep)))
    np.testing.assert_array_equal(best[:n], cc.check_filter(F, keep))
    # the context's own settings through ofps_hip_sad_flow: the same kept set
    ctx.set_sad_gate(gate); ctx.set_sad_consistency(1)
    _same(*ctx.sad_flow(f[1], f[2], B, R, want_best=True), cc.check_filter(ent0, keep), cc.check_filter(F, keep))


def _prm(seed):
    return dict(block=pc.SEQ_B, search_range=pc.SEQ_R, detector=True, estimator=True, aspect=pc.SEQ_CAM[0], fov_y_deg=pc.SEQ_CAM[1],
                use_ransac=False, seed=seed, **pc.SEQ_DETECTOR, **pc.SEQ_RANSAC)


def _check_tail(ctx, k, entries, motion_area, quat):
    q = ctx.almeida(entries, *pc.SEQ_CAM, use_ransac=False, seed=pc.SEQ_SEED + k, **pc.SEQ_RANSAC)[0]
    err = float(np.abs(quat - q).max())
    det = ctx.detect(entries, **pc.SEQ_DETECTOR)
    print(f"frame {k}: |fused - almeida| {err:.3g}, area {motion_area}, detect {gc.area_of(det)}")
    assert err <= QUAT_BOUND
    assert motion_area == gc.area_of(det)


def test_push_frame_one_fused_ticket(ctx):
    ctx.set_sad_prefilter(R4)
    f = pc.sequence()
    ctx.reset_frames()
    for k in range(3):
        r = ctx.push_frame(f[k], want_entries=True, **_prm(pc.SEQ_SEED + k))
        if not k:
            assert not r["have_vectors"]
            continue
        assert r["have_vectors"] and r["n_vectors"] == pc.SEQ_NBLK
        np.testing.assert_array_equal(_bits(r["entries"]), _bits(pc.sequence_expect(k - 1, k)[0]), err_msg=f"frame {k}")
        _check_tail(ctx, k, r["entries"], gc.area_of(r["motion"]), r["quat"])


def test_push_frames_async_batch_of_four(ctx):
    ctx.set_sad_prefilter(R4)
    n = len(pc.SEQ_LIGHT)
    ctx.reset_frames()
    buf = ctx.pinned_array((n, pc.SEQ_H, pc.SEQ_W), np.uint8)
    ents = ctx.pinned_array((n, pc.SEQ_NBLK, 4))
    try:
        np.copyto(buf, pc.sequence())
        res = ctx.frames_wait(ctx.push_frames_async(buf, out_entries=ents, **_prm(pc.SEQ_SEED)))
        assert [r["have_vectors"] for r in res] == [False, True, True, True]
        for k in range(1, n):
            np.testing.assert_array_equal(_bits(ents[k]), _bits(pc.sequence_expect(k - 1, k)[0]), err_msg=f"frame {k}")
            m = res[k]["motion"]
            _check_tail(ctx, k, ents[k].copy(), 0 if m is None else m[0], res[k]["quat"])
    finally:
        ctx.free_pinned(buf); ctx.free_pinned(ents)


def test_multi_device_workers_take_the_radius_from_the_environment(ctx):
    env = dict(os.environ, OFPS_HIP_SAD_PREFILTER=str(R4))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_prefilter_child.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    f = np.ascontiguousarray(pc.sequence())
    n = len(f)
    for ref_mode in (0, 1):
        want = np.stack([pc.sequence_expect(0 if ref_mode else k, k + 1)[0] for k in range(n - 1)])
        assert out[f"sad_flow_ref{ref_mode}"] == _bits(want).reshape(-1).tolist(), ref_mode
    assert [s["have_vectors"] for s in out["stream"]] == [False, True, True, True]
    for k in range(1, n):
        assert out["stream"][k]["entries"] == _bits(pc.sequence_expect(k - 1, k)[0]).reshape(-1).tolist(), k


# ---------------------------------------------------------------- radius 0 again
def test_radius_zero_after_four_equals_a_context_that_never_set_it(ctx):
    from ofps_amd.runtime import HipContext

    def run(c):
        f = pc.sequence()
        out = [c.sad_flow(f[0], f[1], pc.SEQ_B, pc.SEQ_R, want_best=True)]
        out.append(_dev_run(c, f[:3], pc.SEQ_W, 1, pc.SEQ_B, pc.SEQ_R))
        c.set_sad_motion_scale(4)
        out.append(c.sad_flow(f[1], f[2], pc.SEQ_B, pc.SEQ_R, want_best=True))
        c.set_sad_motion_scale(1)
        c.set_sad_levels(2)
        out.append(c.sad_flow(f[1], f[2], pc.SEQ_B, pc.SEQ_R, want_best=True))
        c.set_sad_levels(1)
        c.set_sad_gate(1); c.set_sad_consistency(1)
        out.append(c.sad_flow(f[1], f[2], pc.SEQ_B, pc.SEQ_R, want_best=True))
        c.set_sad_gate(0); c.set_sad_consistency(0)
        c.reset_frames()
        for k in range(3):
            r = c.push_frame(f[k], want_entries=True, **_prm(pc.SEQ_SEED + k))
            if k:
                out.append((r["entries"], r["quat"], np.float32(gc.area_of(r["motion"]))))
        return out

    fresh = HipContext(0)
    try:
        ref = run(fresh)
    finally:
        fresh.close()
    ctx.set_sad_prefilter(R4)
    with_filter = run(ctx)
    assert not np.array_equal(with_filter[0][1], ref[0][1])                              # the option did something in between
    ctx.set_sad_prefilter(0)
    assert ctx.get_sad_prefilter() == 0
    again = run(ctx)
    _same(*ref[0], *pc.sequence_expect(0, 1, 0), "today's bytes")
    for a, b in zip(again, ref):
        for x, y in zip(a, b):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


# ---------------------------------------------------------------- errors, option, plugin
def test_bad_radii_are_einval_and_the_context_stays_usable(ctx):
    lib = _lib.load()
    f = pc.sequence()
    assert ctx.get_sad_prefilter() == 0
    for bad in (-1, 17):
        assert lib.ofps_hip_set_sad_prefilter(ctx._h, bad) == EINVAL
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_sad_prefilter(bad)
        assert ei.value.code == EINVAL and str(bad) in str(ei.value) and ctx.get_sad_prefilter() == 0
    ctx.set_option("OFPS_HIP_SAD_PREFILTER", 16)                                        # the option table sets the same field
    assert ctx.get_sad_prefilter() == 16
    for bad in ("-1", "17"):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_PREFILTER", bad)
        assert ei.value.code == EINVAL and bad in str(ei.value) and ctx.get_sad_prefilter() == 16
    ctx.set_option("OFPS_HIP_SAD_PREFILTER", None)
    assert ctx.get_sad_prefilter() == 0
    for bad in (0, 17):                                                                  # the building block takes [1, 16]
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_prefilter(f[0], bad)
        assert ei.value.code == EINVAL and str(bad) in str(ei.value)
    d = ctx.malloc(64)
    try:
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_prefilter_dev(d, 8, 8, 8, 0, d, 8)
        assert ei.value.code == EINVAL
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_prefilter_dev(d, 8, 8, 4, 1, d, 8)                                   # stride < W
        assert ei.value.code == EINVAL
    finally:
        ctx.free(d)
    _same(*ctx.sad_flow(f[0], f[1], pc.SEQ_B, pc.SEQ_R, want_best=True), *pc.sequence_expect(0, 1, 0))      # the context still works
    ctx.set_sad_prefilter(R4)
    _same(*ctx.sad_flow(f[0], f[1], pc.SEQ_B, pc.SEQ_R, want_best=True), *pc.sequence_expect(0, 1))


def test_plugin_property():
    from ofps_amd.plugins import HipSadDecoder
    dec = HipSadDecoder(iter(pc.sequence()))
    try:
        names = [p[0] for p in dec.props()]
        assert ("Mean removal", "usize", 0, 0, 16) in dec.props()
        assert names.index("Mean removal") + 1 == names.index("Neighbour predictors")
        assert dec.set_prop("Block size", pc.SEQ_B) and dec.set_prop("Search range", pc.SEQ_R)
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(pc.sequence_expect(0, 1, 0)[0]))
        assert dec.set_prop("Mean removal", R4)
        field = []
        assert dec.process_frame(field) is True and dec.ctx.get_sad_prefilter() == R4
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(pc.sequence_expect(1, 2)[0]))
    finally:
        dec.ctx.close()
