"""-m gpu: the neighbour and zero predictors of hip_sad's search levels (include/ofps_hip.h N1p) through the C ABI, bit-exact against the
restatement tests/indep_sad_pred.py throughout: ofps_hip_sad_refine_pred on synthetic parents, the whole search on the two-motion scenes
through the single-context entry points, its composition with the PRUNED mode, the quarter-pel refinement, the contrast gate + consistency
check and the fused per-frame path, one multi-device child process, the field's state, the errors and the plugin property.
Inputs and expectations: tests/sad_pred_cases.py, tests/sad_hier_cases.py (shared, computed once, read-only)."""
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
import indep_sad_pred as ip
import indep_sad_qpel as iq
import sad_consistency_cases as cc
import sad_gate_cases as gc
import sad_hier_cases as hc
import sad_pred_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6                                         # the fused path's documented parity with ofps_hip_almeida (include/ofps_hip.h N1g)
L = 2                                                    # the composition cases: gc.frames() at block 16, range 8, levels 2
NEIGH = ip.PRED_NEIGHBOURS
REFINE_FRAMES = hc.REFINE_FRAMES + ((16, 16, 16),)        # + a 1 x 1 parent lattice: no neighbour at all, only parent and zero


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


def _keys(best):
    return [(int(s), int(dx) * int(dx) + int(dy) * int(dy), int(dy), int(dx)) for dx, dy, s in np.asarray(best)]


# ---------------------------------------------------------------- the refinement step alone
@lru_cache(maxsize=64)
def _refine_expect(W, H, B, kind):
    prev, cur = hc.refine_pair(W, H)
    pnbx, pnby = hc.parent_lattice(W, H, B)
    par = hc.parents(kind, pnbx, pnby)
    best, _, n_pred = ip.refine(prev, cur, B, par.reshape(-1, 3), pnbx, pnby, 127, NEIGH)
    return prev, cur, par, best, ih.entries(best, B, W, H), n_pred


@pytest.mark.parametrize("kind", hc.PARENT_KINDS)
@pytest.mark.parametrize("W,H,B", REFINE_FRAMES)
def test_refine_pred_on_synthetic_parents(ctx, W, H, B, kind):
    prev, cur, par, best_e, ent_e, n_pred = _refine_expect(W, H, B, kind)
    if kind == "zero":
        assert (n_pred == 1).all()
    if (W, H, B) == (40, 24, 8):
        assert par.shape[:2] == (1, 2)                                                  # no vertical neighbours
    if (W, H, B) == (16, 16, 16):
        assert par.shape[:2] == (1, 1)
    best_g, ent_g = ctx.sad_refine_pred(prev, cur, B, par, 127, NEIGH, want_entries=True)
    _same(ent_g, best_g, ent_e, best_e)
    np.testing.assert_array_equal(ctx.sad_refine_pred(prev, cur, B, par, 127, NEIGH), best_e)      # without records


@pytest.mark.parametrize("W,H,B", REFINE_FRAMES)
def test_refine_pred_mode_zero_is_sad_refine(ctx, W, H, B):
    for kind in ("alternating", "edge5"):
        prev, cur, par = _refine_expect(W, H, B, kind)[:3]
        b0, e0 = ctx.sad_refine(prev, cur, B, par, 127, want_entries=True)
        b1, e1 = ctx.sad_refine_pred(prev, cur, B, par, 127, ip.PRED_PARENT, want_entries=True)
        _same(e1, b1, e0, b0, kind)
        np.testing.assert_array_equal(b0, ih.refine(prev, cur, B, par.reshape(-1, 3), par.shape[1], par.shape[0], 127)[0])


@pytest.mark.parametrize("W,H,B,stride", [(50, 38, 12, 52), (40, 24, 8, 44), (64, 48, 16, 68)])
def test_refine_pred_dev_on_rows_only_four_byte_aligned(ctx, W, H, B, stride):
    prev, cur, par, best_e, ent_e, _ = _refine_expect(W, H, B, "alternating")
    nblk = (W // B) * (H // B)
    buf = np.zeros((2, H, stride), np.uint8); buf[0, :, :W] = prev; buf[1, :, :W] = cur
    par = np.ascontiguousarray(par)
    d = [ctx.malloc(buf.nbytes), ctx.malloc(par.nbytes), ctx.malloc(nblk * 12), ctx.malloc(nblk * 16)]
    try:
        ctx.memcpy_h2d(d[0], buf); ctx.memcpy_h2d(d[1], par)
        ctx.sad_refine_pred_dev(d[0], d[0] + H * stride, W, H, stride, B, d[1], par.shape[1], par.shape[0], 127, NEIGH, d[2], d[3])
        ctx.sync()
        best = np.zeros((nblk, 3), np.int32); ent = np.zeros((nblk, 4), np.float32)
        ctx.memcpy_d2h(best, d[2]); ctx.memcpy_d2h(ent, d[3])
    finally:
        for p in d:
            ctx.free(p)
    _same(ent, best, ent_e, best_e)


# ---------------------------------------------------------------- the whole search on the two-motion scenes
@pytest.mark.parametrize("i", range(len(pc.TWO_MOTIONS)))
def test_two_motions_through_sad_flow(ctx, i):
    W, H, B, R, levels, bnd, dl, dr, n_under, _, n_miss0 = pc.TWO_MOTIONS[i]
    under, want = pc.rule(W, H, B, levels, bnd, dl, dr)
    ctx.set_sad_levels(levels)
    got = {}
    for mode in (ip.PRED_PARENT, NEIGH):
        prev, cur, ent_e, best_e, _ = pc.two_motion_expect(i, mode)
        ctx.set_sad_predictors(mode)
        ent_g, best_g = ctx.sad_flow(prev, cur, B, R, want_best=True)
        _same(ent_g, best_g, ent_e, best_e, f"mode {mode}")
        got[mode] = best_g
    miss0, miss1 = pc.misses(got[0], under, want), pc.misses(got[NEIGH], under, want)
    print(f"scene {i}: {int(under.sum())} blocks under the rule, mode 0 misses {int(miss0.sum())}, mode 1 {int(miss1.sum())}")
    assert int(under.sum()) == n_under and not miss1.any(), np.flatnonzero(miss1)
    assert int(miss0.sum()) == n_miss0 >= 1
    if levels == 2:                                                                      # same parents, a superset of candidates
        assert all(a <= b for a, b in zip(_keys(got[NEIGH]), _keys(got[0])))


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


@pytest.mark.parametrize("ref_mode", [0, 1])
def test_two_motions_through_sad_flow_dev_three_frames(ctx, ref_mode):
    """scenes 0 and 1 share their geometry and their previous frame: [prev, cur of scene 0, cur of scene 1].  Ref mode 1 searches both scenes
    against prev; ref mode 0 searches scene 0 and then the pair of the two current frames, halved once for both pairs"""
    W, H, B, R, levels = pc.TWO_MOTIONS[0][:5]
    assert pc.TWO_MOTIONS[1][:5] == (W, H, B, R, levels)
    prev, cur0 = pc.two_motion_expect(0, NEIGH)[:2]
    prev1, cur1 = pc.two_motion_expect(1, NEIGH)[:2]
    np.testing.assert_array_equal(prev, prev1)
    fr = np.stack([prev, cur0, cur1])
    ctx.set_sad_levels(levels); ctx.set_sad_predictors(NEIGH)
    ent, best = _dev_run(ctx, fr, W + 4, ref_mode, B, R)                                  # rows only 4-byte aligned
    _same(ent[0], best[0], *pc.two_motion_expect(0, NEIGH)[2:4], "pair 0")
    if ref_mode:
        _same(ent[1], best[1], *pc.two_motion_expect(1, NEIGH)[2:4], "pair 1")
    else:
        ent_e, best_e, _, _ = ip.search(cur0, cur1, B, R, levels, NEIGH)
        _same(ent[1], best[1], ent_e, best_e, "pair 1")
    for k in range(2 if ref_mode else 1):
        under, want = pc.rule(W, H, B, levels, *pc.TWO_MOTIONS[k][5:8])
        assert not pc.misses(best[k], under, want).any()
    ctx.set_sad_predictors(ip.PRED_PARENT)
    _, best_p = _dev_run(ctx, fr, W + 4, ref_mode, B, R)
    for k in range(2):
        assert all(a <= b for a, b in zip(_keys(best[k]), _keys(best_p[k])))


def test_pruned_mode_equals_exhaustive(ctx):
    prev, cur, ent_e, best_e, _ = pc.two_motion_expect(0, NEIGH)
    W, H, B, R, levels = pc.TWO_MOTIONS[0][:5]
    ctx.set_sad_levels(levels); ctx.set_sad_predictors(NEIGH)
    ctx.set_sad_mode(ctx.SAD_PRUNED)
    _same(*ctx.sad_flow(prev, cur, B, R, want_best=True), ent_e, best_e, "pruned")


# ---------------------------------------------------------------- composition
@lru_cache(maxsize=16)
def _frames_expect(a, b, mode=NEIGH):
    """pair (a, b) of gc.frames() through the restatement -> (entries, best) read-only"""
    f = gc.frames()
    ent, best, _, _ = ip.search(f[a], f[b], gc.BLOCK, gc.RANGE, L, mode)
    ent.setflags(write=False); best.setflags(write=False)
    return ent, best


def test_quarter_pel_refines_the_level_zero_winners(ctx):
    f = gc.frames()
    R0 = ih.reach(gc.RANGE, L)
    ctx.set_sad_levels(L); ctx.set_sad_predictors(NEIGH); ctx.set_sad_motion_scale(4)
    _, best0 = _frames_expect(0, 1)
    ent_e, best_e = iq.refine(f[0], f[1], gc.BLOCK, R0, best0)
    _same(*ctx.sad_flow(f[0], f[1], gc.BLOCK, gc.RANGE, want_best=True), ent_e, best_e)


def test_checked_dev_with_gate_and_limit_runs_both_directions_in_mode_one(ctx):
    f = gc.frames()
    k = 2
    F, G = _frames_expect(k - 1, k)[1], _frames_expect(k, k - 1)[1]
    keep = cc.keep_flags(F, G, gc.FRAME_W, gc.FRAME_H, gc.BLOCK, cc.LIMIT) & gc.frame_keep(k, 1)
    assert 0 < int(keep.sum()) < gc.NBLK
    ent0, best0 = _frames_expect(k - 1, k)
    ctx.set_sad_levels(L); ctx.set_sad_predictors(NEIGH)
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


def _prm(seed):
    return dict(block=gc.BLOCK, search_range=gc.RANGE, detector=True, estimator=True, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1],
                use_ransac=False, seed=seed, **gc.FRAME_DETECTOR, **gc.FRAME_RANSAC)


def test_one_fused_ticket_equals_the_stages_one_by_one(ctx):
    f = gc.frames()
    ctx.set_sad_levels(L); ctx.set_sad_predictors(NEIGH)
    want = ctx.sad_flow(f[0], f[1], gc.BLOCK, gc.RANGE)
    np.testing.assert_array_equal(_bits(want), _bits(_frames_expect(0, 1)[0]))
    ctx.reset_frames()
    pins = [ctx.pinned_frame(gc.FRAME_H, gc.FRAME_W) for _ in range(2)]
    ent = ctx.pinned_array((gc.NBLK, 4))
    try:
        np.copyto(pins[0], f[0]); np.copyto(pins[1], f[1])
        r0 = ctx.frame_wait(ctx.push_frame_async(pins[0], out_entries=ent, **_prm(gc.SEED)))
        assert not r0["have_vectors"]
        r = ctx.frame_wait(ctx.push_frame_async(pins[1], out_entries=ent, **_prm(gc.SEED + 1)))
        got = ent.copy()
    finally:
        for p in pins + [ent]:
            ctx.free_pinned(p)
    assert r["have_vectors"] and r["n_vectors"] == gc.NBLK
    np.testing.assert_array_equal(_bits(got), _bits(want))
    q = ctx.almeida(got, *gc.FRAME_CAM, use_ransac=False, seed=gc.SEED + 1, **gc.FRAME_RANSAC)[0]
    assert float(np.abs(r["quat"] - q).max()) <= QUAT_BOUND
    assert (0 if r["motion"] is None else r["motion"][0]) == gc.area_of(ctx.detect(got, **gc.FRAME_DETECTOR))


def test_multi_device_workers_take_the_mode_from_the_environment(ctx):
    env = dict(os.environ, OFPS_HIP_SAD_LEVELS=str(L), OFPS_HIP_SAD_PREDICTORS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_pred_child.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    f = np.ascontiguousarray(gc.frames())
    ctx.set_sad_levels(L); ctx.set_sad_predictors(NEIGH)
    for ref_mode in (0, 1):
        ent, _ = _dev_run(ctx, f, gc.FRAME_W, ref_mode, gc.BLOCK, gc.RANGE)
        assert out[f"sad_flow_ref{ref_mode}"] == _bits(ent).reshape(-1).tolist(), ref_mode
        np.testing.assert_array_equal(_bits(ent[0]), _bits(_frames_expect(0, 1)[0]))
    assert [s["have_vectors"] for s in out["stream"]] == [False, True, True, True]
    for k in range(1, gc.N_FRAMES):
        assert out["stream"][k]["entries"] == _bits(_frames_expect(k - 1, k)[0]).reshape(-1).tolist(), k


# ---------------------------------------------------------------- the field's state
def test_mode_zero_after_one_equals_a_context_that_never_set_it(ctx):
    from ofps_amd.runtime import HipContext

    def run(c):
        f = gc.frames()
        out = [c.sad_flow(f[0], f[1], gc.BLOCK, gc.RANGE, want_best=True)]
        out.append(_dev_run(c, f[:3], gc.FRAME_W, 1, gc.BLOCK, gc.RANGE))
        c.set_sad_gate(1); c.set_sad_consistency(cc.LIMIT)
        out.append(c.sad_flow(f[1], f[2], gc.BLOCK, gc.RANGE, want_best=True))
        c.set_sad_gate(0); c.set_sad_consistency(0)
        return out

    fresh = HipContext(0)
    try:
        fresh.set_sad_levels(L)
        assert fresh.get_sad_predictors() == 0
        ref = run(fresh)
    finally:
        fresh.close()
    ctx.set_sad_levels(L); ctx.set_sad_predictors(NEIGH)
    assert ctx.get_sad_predictors() == 1
    with_mode = run(ctx)
    _same(*with_mode[0], *_frames_expect(0, 1))
    ctx.set_sad_predictors(ip.PRED_PARENT)
    assert ctx.get_sad_predictors() == 0
    again = run(ctx)
    _same(*again[0], *_frames_expect(0, 1, ip.PRED_PARENT))
    for a, b in zip(again, ref):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def test_mode_one_at_levels_one_is_the_plain_search(ctx):
    f = gc.frames()
    plain = ctx.sad_flow(f[0], f[1], gc.BLOCK, gc.RANGE, want_best=True)
    np.testing.assert_array_equal(_bits(plain[0]), _bits(gc.frame_vectors(1)[0]))       # the plain search's bytes
    ctx.set_sad_predictors(NEIGH)                                                       # stored, no effect, no error
    assert ctx.get_sad_levels() == 1 and ctx.get_sad_predictors() == 1
    _same(*ctx.sad_flow(f[0], f[1], gc.BLOCK, gc.RANGE, want_best=True), *plain)
    ent, best = _dev_run(ctx, f[:3], gc.FRAME_W, 0, gc.BLOCK, gc.RANGE)
    _same(ent[0], best[0], *plain)


def test_bad_modes_are_einval_and_the_context_stays_usable(ctx):
    lib = _lib.load()
    prev, cur, par = _refine_expect(64, 48, 16, "alternating")[:3]
    assert ctx.get_sad_predictors() == 0
    for bad in (-1, 2):
        assert lib.ofps_hip_set_sad_predictors(ctx._h, bad) == EINVAL
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_sad_predictors(bad)
        assert ei.value.code == EINVAL and str(bad) in str(ei.value) and ctx.get_sad_predictors() == 0
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_refine_pred(prev, cur, 16, par, 127, bad)
        assert ei.value.code == EINVAL and str(bad) in str(ei.value)
    assert lib.ofps_hip_set_sad_predictors(None, 1) == EINVAL and lib.ofps_hip_get_sad_predictors(None) == EINVAL
    ctx.set_option("OFPS_HIP_SAD_PREDICTORS", 1)                                        # the option table sets the same field
    assert ctx.get_sad_predictors() == 1
    for bad in ("2", "-1", "on"):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_PREDICTORS", bad)
        assert ei.value.code == EINVAL and bad in str(ei.value) and ctx.get_sad_predictors() == 1
    ctx.set_option("OFPS_HIP_SAD_PREDICTORS", None)
    assert ctx.get_sad_predictors() == 0
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_refine_pred(prev, cur, 16, par, 128, NEIGH)                             # the existing call's checks: reach outside [0, 127]
    assert ei.value.code == EINVAL and "128" in str(ei.value)
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_refine_pred(prev, cur, 65, par, 127, NEIGH)                             # block outside [1, 64]
    assert ei.value.code == EINVAL
    np.testing.assert_array_equal(ctx.sad_refine_pred(prev, cur, 16, par, 127, NEIGH), _refine_expect(64, 48, 16, "alternating")[3])


def test_plugin_property():
    from ofps_amd.plugins import HipSadDecoder
    dec = HipSadDecoder(iter(gc.frames()))
    try:
        assert ("Neighbour predictors", "bool", False, None, None) in dec.props()
        assert dec.set_prop("Search range", gc.RANGE) and dec.set_prop("Search levels", L)
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True and dec.ctx.get_sad_predictors() == 0
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(_frames_expect(0, 1, ip.PRED_PARENT)[0]))
        assert dec.set_prop("Neighbour predictors", True)
        field = []
        assert dec.process_frame(field) is True and dec.ctx.get_sad_predictors() == 1
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(_frames_expect(1, 2)[0]))
    finally:
        dec.ctx.close()
