"""-m gpu: hip_sad's search levels (include/ofps_hip.h N1h) through the C ABI, bit-exact against the restatement tests/indep_sad_hier.py
throughout: the two building blocks alone (ofps_hip_sad_down2, ofps_hip_sad_refine on synthetic parents), the whole search through every
single-context entry point, its composition with the quarter-pel refinement, the contrast gate, the consistency check and the fused
per-frame path, one multi-device child process, levels 1 after levels 2, the errors and the plugin property.
Inputs and expectations: tests/sad_hier_cases.py (shared, computed once, read-only)."""
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
import indep_sad_qpel as iq
import sad_consistency_cases as cc
import sad_gate_cases as gc
import sad_hier_cases as hc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6                                         # the fused path's documented parity with ofps_hip_almeida (include/ofps_hip.h N1g)
L = 2                                                    # the composition cases: gc.frames() at block 16, range 8, levels 2


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


# ---------------------------------------------------------------- the building blocks
@pytest.mark.parametrize("W,H,stride", hc.DOWN2_SIZES)
def test_down2_matches_the_restatement(ctx, W, H, stride):
    buf = hc.down2_frame(W, H, stride)
    want = ih.down2(buf[:, :W])
    assert want.shape == (H >> 1, W >> 1)
    np.testing.assert_array_equal(ctx.sad_down2(buf[:, :W], stride=stride), want)
    np.testing.assert_array_equal(ctx.sad_down2(buf[:, :W].copy()), want)                # dense rows


def test_down2_dev_into_a_dense_destination_writes_nothing_beside_it(ctx):
    W, H, stride = 37, 23, 40
    buf = hc.down2_frame(W, H, stride)
    Wo, Ho = W >> 1, H >> 1
    guard = np.full(Wo * Ho + 64, 0xA5, np.uint8)
    d_src, d_dst = ctx.malloc(buf.nbytes), ctx.malloc(guard.nbytes)
    try:
        ctx.memcpy_h2d(d_src, buf); ctx.memcpy_h2d(d_dst, guard)
        ctx.sad_down2_dev(d_src, W, H, stride, d_dst, Wo)                               # dst_stride = 18: rows not even 4-byte aligned
        ctx.sync()
        out = np.zeros_like(guard)
        ctx.memcpy_d2h(out, d_dst)
    finally:
        ctx.free(d_src); ctx.free(d_dst)
    np.testing.assert_array_equal(out[:Wo * Ho].reshape(Ho, Wo), ih.down2(buf[:, :W]))
    assert (out[Wo * Ho:] == 0xA5).all()


@lru_cache(maxsize=64)
def _refine_expect(W, H, B, kind, flat=False):
    prev, cur = hc.refine_pair(W, H)
    if flat:
        prev = cur = np.full((H, W), 131, np.uint8)
    pnbx, pnby = hc.parent_lattice(W, H, B)
    par = hc.parents(kind, pnbx, pnby)
    best, _ = ih.refine(prev, cur, B, par.reshape(-1, 3), pnbx, pnby, 127)
    return prev, cur, par, best, ih.entries(best, B, W, H)


@pytest.mark.parametrize("kind", hc.PARENT_KINDS)
@pytest.mark.parametrize("W,H,B", hc.REFINE_FRAMES)
def test_refine_on_synthetic_parents(ctx, W, H, B, kind):
    prev, cur, par, best_e, ent_e = _refine_expect(W, H, B, kind)
    best_g, ent_g = ctx.sad_refine(prev, cur, B, par, 127, want_entries=True)
    _same(ent_g, best_g, ent_e, best_e)
    np.testing.assert_array_equal(ctx.sad_refine(prev, cur, B, par, 127), best_e)        # without records


@pytest.mark.parametrize("W,H,B", hc.REFINE_FRAMES)
def test_refine_of_a_flat_pair_breaks_ties_towards_zero(ctx, W, H, B):
    for kind in ("zero", "alternating", "edge4"):
        prev, cur, par, best_e, ent_e = _refine_expect(W, H, B, kind, flat=True)
        assert (best_e[:, 2] == 0).all()
        best_g, ent_g = ctx.sad_refine(prev, cur, B, par, 127, want_entries=True)
        _same(ent_g, best_g, ent_e, best_e, kind)


def test_refine_dev_on_rows_only_four_byte_aligned(ctx):
    """50 x 38 at block 12 with a device stride of 52: the generic form, rows 4-byte aligned only"""
    W, H, B, stride = 50, 38, 12, 52
    prev, cur, par, best_e, ent_e = _refine_expect(W, H, B, "alternating")
    nblk = (W // B) * (H // B)
    buf = np.zeros((2, H, stride), np.uint8); buf[0, :, :W] = prev; buf[1, :, :W] = cur
    par = np.ascontiguousarray(par)
    d = [ctx.malloc(buf.nbytes), ctx.malloc(par.nbytes), ctx.malloc(nblk * 12), ctx.malloc(nblk * 16)]
    try:
        ctx.memcpy_h2d(d[0], buf); ctx.memcpy_h2d(d[1], par)
        ctx.sad_refine_dev(d[0], d[0] + H * stride, W, H, stride, B, d[1], par.shape[1], par.shape[0], 127, d[2], d[3])
        ctx.sync()
        best = np.zeros((nblk, 3), np.int32); ent = np.zeros((nblk, 4), np.float32)
        ctx.memcpy_d2h(best, d[2]); ctx.memcpy_d2h(ent, d[3])
    finally:
        for p in d:
            ctx.free(p)
    _same(ent, best, ent_e, best_e)


# ---------------------------------------------------------------- the whole search
@pytest.mark.parametrize("i", range(len(hc.PLANTED)))
def test_planted_shift_through_sad_flow(ctx, i):
    W, H, B, R, levels, d, n_reach, _ = hc.PLANTED[i]
    prev, cur, ent_e, best_e, _ = hc.planted_expect(i)
    ctx.set_sad_levels(levels)
    ent_g, best_g = ctx.sad_flow(prev, cur, B, R, want_best=True)
    _same(ent_g, best_g, ent_e, best_e)
    reach = hc.reachable(W, H, B, levels, d)
    hit = (best_g[:, 0] == d[0]) & (best_g[:, 1] == d[1])
    print(f"case {i}: {int(reach.sum())} of {len(reach)} blocks fall under the rule, {int(hit.sum())} return d")
    assert int(reach.sum()) == n_reach and not (reach & ~hit).any()
    ctx.set_sad_levels(1)
    plain = ctx.sad_flow(prev, cur, B, R, want_best=True)[1]
    assert not ((plain[:, 0] == d[0]) & (plain[:, 1] == d[1])).any()


def test_top_search_is_sad_flow_of_the_downsampled_pair(ctx):
    for i in (2, 3):
        W, H, B, R, levels, _, _, _ = hc.PLANTED[i]
        prev, cur, _, _, per_level = hc.planted_expect(i)
        pp, pc = ih.pyramid(prev, levels), ih.pyramid(cur, levels)
        for l in range(1, levels):
            np.testing.assert_array_equal(ctx.sad_down2(pp[l - 1]), pp[l])
        assert ctx.get_sad_levels() == 1
        top = ctx.sad_flow(pp[-1], pc[-1], B, R, want_best=True)[1]
        np.testing.assert_array_equal(top, per_level[-1])
        # ... and the refinement steps, one by one, lead from it to the whole search's output
        best = top
        for l in range(levels - 2, -1, -1):
            ph, pw = pp[l + 1].shape
            best = ctx.sad_refine(pp[l], pc[l], B, best.reshape(ph // B, pw // B, 3), ih.reaches(R, levels)[l])
            np.testing.assert_array_equal(best, per_level[l])


def _dev_run(ctx, fr, stride, ref_mode, B, R, with_best=True):
    n, H, W = fr.shape
    buf = np.zeros((n, H, stride), np.uint8); buf[:, :, :W] = fr
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


@lru_cache(maxsize=16)
def _frames_expect(a, b, levels=L):
    """pair (a, b) of gc.frames() through the restatement -> (entries, best) read-only"""
    f = gc.frames()
    ent, best, _ = ih.search(f[a], f[b], gc.BLOCK, gc.RANGE, levels)
    ent.setflags(write=False); best.setflags(write=False)
    return ent, best


@pytest.mark.parametrize("ref_mode", [0, 1])
def test_sad_flow_dev_three_frames(ctx, ref_mode):
    f = gc.frames()[:3]
    ctx.set_sad_levels(L)
    for stride, with_best in ((gc.FRAME_W, True), (gc.FRAME_W + 4, False)):             # 16-byte rows; rows only 4-byte aligned, no out_best
        ent, best = _dev_run(ctx, f, stride, ref_mode, gc.BLOCK, gc.RANGE, with_best)
        for k in range(2):
            ent_e, best_e = _frames_expect(0 if ref_mode else k, k + 1)
            np.testing.assert_array_equal(_bits(ent[k]), _bits(ent_e), err_msg=f"stride {stride} pair {k}")
            if with_best:
                np.testing.assert_array_equal(best[k], best_e)


def test_pruned_mode_equals_exhaustive(ctx):
    prev, cur = hc.planted_pair(320, 192, (33, -26))
    ent_e, best_e, _ = ih.search(prev, cur, 16, 16, 2)
    ctx.set_sad_levels(2)
    _same(*ctx.sad_flow(prev, cur, 16, 16, want_best=True), ent_e, best_e, "exhaustive")
    ctx.set_sad_mode(ctx.SAD_PRUNED)
    _same(*ctx.sad_flow(prev, cur, 16, 16, want_best=True), ent_e, best_e, "pruned")


# ---------------------------------------------------------------- composition
def test_quarter_pel_refines_the_level_zero_winners(ctx):
    f = gc.frames()
    R0 = ih.reach(gc.RANGE, L)
    ctx.set_sad_levels(L); ctx.set_sad_motion_scale(4)
    for k in (1, 2):
        _, best0 = _frames_expect(k - 1, k)
        ent_e, best_e = iq.refine(f[k - 1], f[k], gc.BLOCK, R0, best0)
        _same(*ctx.sad_flow(f[k - 1], f[k], gc.BLOCK, gc.RANGE, want_best=True), ent_e, best_e, f"pair {k}")
    # without out_best the level-0 winners live in the context's own scratch
    ent, _ = _dev_run(ctx, f[:2], gc.FRAME_W, 0, gc.BLOCK, gc.RANGE, with_best=False)
    np.testing.assert_array_equal(_bits(ent[0]), _bits(iq.refine(f[0], f[1], gc.BLOCK, R0, _frames_expect(0, 1)[1])[0]))


@lru_cache(maxsize=8)
def _chain_keep(k, gate):
    """keep flags of frame k of gc.frames(): the consistency check at limit 1 over the restatement's winners of both directions [and the gate]"""
    F = _frames_expect(k - 1, k)[1]
    G = _frames_expect(k, k - 1)[1]
    keep = cc.keep_flags(F, G, gc.FRAME_W, gc.FRAME_H, gc.BLOCK, cc.LIMIT)
    return keep & gc.frame_keep(k, gate) if gate else keep


@pytest.mark.parametrize("scale", [1, 4])
def test_checked_dev_with_gate_and_limit(ctx, scale):
    f = gc.frames()
    k = 2
    keep = _chain_keep(k, 1)
    assert 0 < int(keep.sum()) < gc.NBLK
    ent0, best0 = _frames_expect(k - 1, k)
    if scale == 4:
        ent0, best0 = iq.refine(f[k - 1], f[k], gc.BLOCK, ih.reach(gc.RANGE, L), best0)
    ctx.set_sad_levels(L); ctx.set_sad_motion_scale(scale)
    pair = np.ascontiguousarray(f[k - 1:k + 1])
    d = [ctx.malloc(pair.nbytes), ctx.malloc(gc.NBLK * 16), ctx.malloc(gc.NBLK * 12), ctx.malloc(16)]
    try:
        ctx.memcpy_h2d(d[0], pair)
        ctx.sad_flow_checked_dev(d[0], d[0] + gc.FRAME_W * gc.FRAME_H, gc.FRAME_W, gc.FRAME_H, gc.FRAME_W, gc.BLOCK, gc.RANGE, 1, cc.LIMIT,
                                 d[1], d[2], d[3])
        ctx.sync()
        ent = np.zeros((gc.NBLK, 4), np.float32); best = np.zeros((gc.NBLK, 3), np.int32); cnt = np.zeros(4, np.uint32)
        ctx.memcpy_d2h(ent, d[1]); ctx.memcpy_d2h(best, d[2]); ctx.memcpy_d2h(cnt, d[3])
    finally:
        for p in d:
            ctx.free(p)
    n = int(cnt[0])
    assert n == int(keep.sum())
    np.testing.assert_array_equal(_bits(ent[:n]), _bits(cc.check_filter(ent0, keep)))
    np.testing.assert_array_equal(best[:n], cc.check_filter(best0, keep))
    # the context's own settings through ofps_hip_sad_flow: the same kept set
    ctx.set_sad_gate(1); ctx.set_sad_consistency(cc.LIMIT)
    ent_s, best_s = ctx.sad_flow(f[k - 1], f[k], gc.BLOCK, gc.RANGE, want_best=True)
    _same(ent_s, best_s, cc.check_filter(ent0, keep), cc.check_filter(best0, keep))
    # a limit above 2 * R_0 + 1 keeps every block
    ctx.set_sad_gate(0); ctx.set_sad_consistency(2 * ih.reach(gc.RANGE, L) + 2)
    assert len(ctx.sad_flow(f[k - 1], f[k], gc.BLOCK, gc.RANGE)) == gc.NBLK


def _prm(seed):
    return dict(block=gc.BLOCK, search_range=gc.RANGE, detector=True, estimator=True, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1],
                use_ransac=False, seed=seed, **gc.FRAME_DETECTOR, **gc.FRAME_RANSAC)


def _one_pair_records(ctx):
    f = gc.frames()
    want = [None] + [ctx.sad_flow(f[k - 1], f[k], gc.BLOCK, gc.RANGE) for k in range(1, gc.N_FRAMES)]
    for k in range(1, gc.N_FRAMES):
        np.testing.assert_array_equal(_bits(want[k]), _bits(_frames_expect(k - 1, k)[0]), err_msg=f"pair {k}")
    return want


def _check_tail(ctx, k, entries, motion_area, field, dim, quat):
    q = ctx.almeida(entries, *gc.FRAME_CAM, use_ransac=False, seed=gc.SEED + k, **gc.FRAME_RANSAC)[0]
    err = float(np.abs(quat - q).max())
    det = ctx.detect(entries, **gc.FRAME_DETECTOR)
    print(f"frame {k}: |fused - almeida| {err:.3g}, area {motion_area}, detect {gc.area_of(det)}")
    assert err <= QUAT_BOUND
    assert motion_area == gc.area_of(det)
    if det is not None:
        if field is not None:
            np.testing.assert_array_equal(_bits(field), _bits(det[1]))
        if dim is not None:
            assert dim == det[1].shape[0]


def test_push_frame_async_two_tickets_in_flight(ctx):
    ctx.set_sad_levels(L)
    want = _one_pair_records(ctx)
    f = gc.frames()
    ctx.reset_frames()
    dim = ctx.block_dim(gc.FRAME_DETECTOR["min_size"], gc.FRAME_DETECTOR["subdivide"])
    pins = [ctx.pinned_frame(gc.FRAME_H, gc.FRAME_W) for _ in range(3)]
    ents = [ctx.pinned_array((gc.NBLK, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    tickets, got = [], []

    def collect(k):
        r = ctx.frame_wait(tickets[k])
        got.append((r, ents[k % 2].copy(), flds[k % 2].copy()))

    try:
        for k in range(gc.N_FRAMES):
            if k >= 2:
                collect(k - 2)
            np.copyto(pins[k % 3], f[k])
            tickets.append(ctx.push_frame_async(pins[k % 3], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(gc.SEED + k)))
        collect(gc.N_FRAMES - 2); collect(gc.N_FRAMES - 1)
    finally:
        for p in pins + ents + flds:
            ctx.free_pinned(p)
    assert not got[0][0]["have_vectors"]
    for k in range(1, gc.N_FRAMES):
        r, ent, fld = got[k]
        assert r["have_vectors"] and r["n_vectors"] == gc.NBLK
        np.testing.assert_array_equal(_bits(ent), _bits(want[k]), err_msg=f"frame {k}")
        _check_tail(ctx, k, ent, 0 if r["motion"] is None else r["motion"][0], fld if r["motion"] is not None else None, None, r["quat"])


def test_push_frames_async_batch_of_four(ctx):
    ctx.set_sad_levels(L)
    want = _one_pair_records(ctx)
    ctx.reset_frames()
    buf = ctx.pinned_array((gc.N_FRAMES, gc.FRAME_H, gc.FRAME_W), np.uint8)
    ents = ctx.pinned_array((gc.N_FRAMES, gc.NBLK, 4))
    try:
        np.copyto(buf, gc.frames())
        res = ctx.frames_wait(ctx.push_frames_async(buf, out_entries=ents, **_prm(gc.SEED)))
        assert [r["have_vectors"] for r in res] == [False, True, True, True]
        for k in range(1, gc.N_FRAMES):
            np.testing.assert_array_equal(_bits(ents[k]), _bits(want[k]), err_msg=f"frame {k}")
            m = res[k]["motion"]
            _check_tail(ctx, k, ents[k].copy(), 0 if m is None else m[0], None, None if m is None else m[1], res[k]["quat"])
    finally:
        ctx.free_pinned(buf); ctx.free_pinned(ents)


def test_multi_device_workers_take_the_levels_from_the_environment(ctx):
    env = dict(os.environ, OFPS_HIP_SAD_LEVELS=str(L))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_hier_child.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    f = np.ascontiguousarray(gc.frames())
    ctx.set_sad_levels(L)
    for ref_mode in (0, 1):
        ent, _ = _dev_run(ctx, f, gc.FRAME_W, ref_mode, gc.BLOCK, gc.RANGE)
        assert out[f"sad_flow_ref{ref_mode}"] == _bits(ent).reshape(-1).tolist(), ref_mode
        np.testing.assert_array_equal(_bits(ent[0]), _bits(_frames_expect(0, 1)[0]))
    assert [s["have_vectors"] for s in out["stream"]] == [False, True, True, True]
    for k in range(1, gc.N_FRAMES):
        assert out["stream"][k]["entries"] == _bits(_frames_expect(k - 1, k)[0]).reshape(-1).tolist(), k


# ---------------------------------------------------------------- levels 1 again
def test_levels_one_after_two_equals_a_context_that_never_set_it(ctx):
    from ofps_amd.runtime import HipContext

    def run(c):
        f = gc.frames()
        out = [c.sad_flow(f[0], f[1], gc.BLOCK, gc.RANGE, want_best=True)]
        out.append(_dev_run(c, f[:3], gc.FRAME_W, 1, gc.BLOCK, gc.RANGE))
        c.set_sad_motion_scale(4)
        out.append(c.sad_flow(f[1], f[2], gc.BLOCK, gc.RANGE, want_best=True))
        c.set_sad_motion_scale(1)
        c.set_sad_gate(1); c.set_sad_consistency(cc.LIMIT)
        out.append(c.sad_flow(f[1], f[2], gc.BLOCK, gc.RANGE, want_best=True))
        c.set_sad_gate(0); c.set_sad_consistency(0)
        c.reset_frames()
        for k in range(3):
            r = c.push_frame(f[k], want_entries=True, want_field=True, **_prm(gc.SEED + k))
            if k:
                out.append((r["entries"], r["quat"], np.float32(gc.area_of(r["motion"]))))
        return out

    fresh = HipContext(0)
    try:
        ref = run(fresh)
    finally:
        fresh.close()
    ctx.set_sad_levels(2)
    with_levels = run(ctx)
    assert not np.array_equal(with_levels[0][1], ref[0][1])                              # the option did something in between
    ctx.set_sad_levels(1)
    assert ctx.get_sad_levels() == 1
    again = run(ctx)
    np.testing.assert_array_equal(_bits(ref[0][0]), _bits(gc.frame_vectors(1)[0]))       # today's bytes
    for a, b in zip(again, ref):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


# ---------------------------------------------------------------- errors, option, plugin
def test_bad_levels_ranges_and_frames_are_einval_and_the_context_stays_usable(ctx):
    lib = _lib.load()
    prev, cur = hc.refine_pair(64, 48)
    want = ctx.sad_flow(prev, cur, 16, 8, want_best=True)
    assert ctx.get_sad_levels() == 1
    for bad in (0, 4):
        assert lib.ofps_hip_set_sad_levels(ctx._h, bad) == EINVAL
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_sad_levels(bad)
        assert ei.value.code == EINVAL and str(bad) in str(ei.value) and ctx.get_sad_levels() == 1
    ctx.set_option("OFPS_HIP_SAD_LEVELS", 3)                                            # the option table sets the same field
    assert ctx.get_sad_levels() == 3
    for bad in ("0", "4", "two"):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_LEVELS", bad)
        assert ei.value.code == EINVAL and bad in str(ei.value) and ctx.get_sad_levels() == 3
    ctx.set_option("OFPS_HIP_SAD_LEVELS", None)
    assert ctx.get_sad_levels() == 1
    big = np.zeros((192, 320), np.uint8)
    for levels, R, frame, B, names in ((3, 32, big, 16, ("32", "137")), (2, 63, big, 16, ("63", "129")), (2, 8, np.zeros((24, 24), np.uint8), 16, ("24", "16"))):
        ctx.set_sad_levels(levels)
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow(frame, frame, B, R)
        assert ei.value.code == EINVAL and all(n in str(ei.value) for n in names), str(ei.value)
    assert ctx.sad_reach(62, 2) == 127 and ctx.sad_reach(8, 3) == 41
    for R, levels in ((63, 2), (32, 3), (8, 0), (8, 4)):
        with pytest.raises(ValueError):
            ctx.sad_reach(R, levels)
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_refine(prev, cur, 16, np.zeros((1, 2, 3), np.int32), 128)                # reach outside [0, 127]
    assert ei.value.code == EINVAL and "128" in str(ei.value)
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_down2(np.zeros((1, 8), np.uint8))                                       # H < 2
    assert ei.value.code == EINVAL
    ctx.set_sad_levels(1)
    _same(*ctx.sad_flow(prev, cur, 16, 8, want_best=True), *want)                        # the context still works
    ctx.set_sad_levels(2)
    ent_e, best_e, _ = ih.search(prev, cur, 16, 8, 2)
    _same(*ctx.sad_flow(prev, cur, 16, 8, want_best=True), ent_e, best_e)


def test_plugin_property():
    from ofps_amd.plugins import HipSadDecoder
    dec = HipSadDecoder(iter(gc.frames()))
    try:
        assert ("Search levels", "usize", 1, 1, 3) in dec.props()
        assert dec.props()[-1][0] == "Search levels" and dec.props()[-2][0] == "Consistency check"
        assert dec.set_prop("Search range", gc.RANGE)
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(gc.frame_vectors(1)[0]))
        assert dec.set_prop("Search levels", L)
        field = []
        assert dec.process_frame(field) is True and dec.ctx.get_sad_levels() == L
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(_frames_expect(1, 2)[0]))
    finally:
        dec.ctx.close()
