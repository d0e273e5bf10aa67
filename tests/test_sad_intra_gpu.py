"""-m gpu: hip_sad's intra test and scene-cut rule (include/ofps_hip.h N1i) against the restatement tests/indep_sad_intra.py on the cases of
tests/sad_intra_cases.py.  Activities, flags, counters, records and winners are integers or copies: every equality is bit for bit.  The one
exception is the quaternion of the fused path's device-count form, held to the solver's documented parity with ofps_hip_almeida on the same
records: 2e-6 (least squares).  tests/test_sad_intra_cpu.py proves on the restatement that the inputs separate the ratios.

Where a search runs in a mode the CPU oracle does not restate here (search levels with neighbour predictors, mean removal), the INTEGER
winners the verdicts are computed from are the library's own unfiltered winners in that mode -- tests/test_sad_pred_gpu.py and
tests/test_sad_prefilter_gpu.py hold those to their restatements -- and the verdicts are the restatement's of this test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import indep_sad_intra as ii
import indep_sad_median as im
import sad_consistency_cases as cc
import sad_gate_cases as gc
import sad_intra_cases as ic
import sad_median_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1, 0, 0, 0], np.float32)
EINVAL = -1
QUAT_BOUND = 2e-6                                        # least squares: the solver's documented parity
B, R = mc.SCENE_B, mc.SCENE_R
Q = ic.SCENE_Q


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _settings:
    """context settings for the length of a block; everything back to the defaults behind it"""
    DEFAULT = dict(intra=0, cut=0, median=0, limit=0, gate=0, scale=1, levels=1, predictors=0, prefilter=0, pruned=False, batch_filter=0)

    def __init__(self, ctx, **kw):
        self.ctx, self.v = ctx, dict(self.DEFAULT, **kw)

    def _apply(self, v):
        c = self.ctx
        c.set_sad_intra(v["intra"]); c.set_sad_cut(v["cut"]); c.set_sad_median(v["median"]); c.set_sad_consistency(v["limit"])
        c.set_sad_gate(v["gate"]); c.set_sad_motion_scale(v["scale"]); c.set_sad_levels(v["levels"]); c.set_sad_predictors(v["predictors"])
        c.set_sad_prefilter(v["prefilter"]); c.set_sad_batch_filter(v["batch_filter"])
        c.set_sad_mode(c.SAD_PRUNED if v["pruned"] else c.SAD_EXHAUSTIVE)

    def __enter__(self):
        self._apply(self.v)

    def __exit__(self, *exc):
        self._apply(self.DEFAULT)


# --------------------------------------------------------------------------------------------------------------- the activity alone
def _activity_dev(ctx, buf, W, H, block, offset=0):
    """buf: [H, stride] u8 -> the _dev form's output, 64 guard words behind it checked.  offset: the frame starts that many bytes into its
    device allocation (an unaligned base)"""
    import torch
    stride = buf.shape[1]
    n = (W // block) * (H // block)
    d_all = torch.full((offset + buf.size,), 255, dtype=torch.uint8, device="cuda")
    d_all[offset:] = torch.from_numpy(np.array(buf).reshape(-1)).cuda()
    d_out = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.block_activity_dev(d_all.data_ptr() + offset, W, H, stride, block, d_out.data_ptr())
    ctx.sync()
    out = d_out.cpu().numpy()
    assert (out[n:] == -1).all(), "guard words"
    return out[:n].view(np.uint32)


@pytest.mark.parametrize("name", list(ic.ACTIVITY))
def test_activity_of_the_derived_cases(ctx, name):
    frame, block, want = ic.ACTIVITY[name]()
    H, W = frame.shape
    got = ctx.block_activity(frame, block)
    assert got.dtype == np.uint32 and got.shape == (H // block, W // block)
    assert got.reshape(-1).tolist() == want, name                    # the values the case derives from the definition
    assert _activity_dev(ctx, frame, W, H, block).tolist() == want, name + " dev"


@pytest.mark.parametrize("W,H,block,stride", ic.SHAPES, ids=[f"{w}x{h}-b{b}-s{s}" for w, h, b, s in ic.SHAPES])
def test_activity_on_ragged_shapes(ctx, W, H, block, stride):
    buf = ic.shape_frame(W, H, stride)
    want = ic.shape_activity(W, H, block, stride)
    np.testing.assert_array_equal(_activity_dev(ctx, buf, W, H, block), want)
    for offset in (4, 1):                                            # a base that is a multiple of 4 only, and of nothing
        np.testing.assert_array_equal(_activity_dev(ctx, buf, W, H, block, offset), want, err_msg=f"base + {offset}")
    np.testing.assert_array_equal(ctx.block_activity(buf[:, :W], block, stride=stride).reshape(-1), want)       # the host form takes the stride
    if block > 1:
        assert ctx.block_activity(buf[:block - 1, :W], block).size == 0                 # no full block: nothing to do


# --------------------------------------------------------------------------------------------------------------- the verdict alone
def _intra_dev(ctx, best, act, kin, W, H, block, ratio, cut, want_counts=True, in_place=False):
    import torch
    n = len(best)
    d_best = torch.from_numpy(np.array(best, np.int32)).cuda()
    d_act = torch.from_numpy(np.array(act, np.uint32).view(np.int32)).cuda()
    d_keep = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
    d_kin = None
    if kin is not None:
        if in_place:
            d_keep[:n] = torch.from_numpy(np.array(kin, np.uint8)).cuda()
            d_kin = d_keep
        else:
            d_kin = torch.from_numpy(np.array(kin, np.uint8)).cuda()
    d_cnt = torch.full((2 + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_intra_dev(d_best.data_ptr(), d_act.data_ptr(), None if d_kin is None else d_kin.data_ptr(), W, H, block, ratio, cut, d_keep.data_ptr(),
                      d_cnt.data_ptr() if want_counts else None)
    ctx.sync()
    keep, cnt = d_keep.cpu().numpy(), d_cnt.cpu().numpy()
    assert (keep[n:] == 7).all() and (cnt[2:] == -1).all(), "guard words"
    if not want_counts:
        assert (cnt == -1).all()
    return keep[:n], (tuple(int(c) for c in cnt[:2]) if want_counts else None)


def _check_verdict(ctx, best, act, kin, W, H, block, ratio, cut, what):
    want_keep, want_counts, _ = ii.verdict(best, act, kin, ratio, cut)
    keep, counts = ctx.sad_intra(best, act, kin, W, H, block, ratio, cut)
    np.testing.assert_array_equal(keep, want_keep, err_msg=what)
    assert tuple(int(c) for c in counts) == want_counts, what
    np.testing.assert_array_equal(ctx.sad_intra(best, act, kin, W, H, block, ratio, cut, want_counts=False)[0], want_keep, err_msg=what)
    for want_c in (True, False):
        for in_place in ((False, True) if kin is not None else (False,)):
            keep, counts = _intra_dev(ctx, best, act, kin, W, H, block, ratio, cut, want_c, in_place)
            np.testing.assert_array_equal(keep, want_keep, err_msg=f"{what} dev counts={want_c} in_place={in_place}")
            assert counts == (want_counts if want_c else None), what
    return want_keep, want_counts


@pytest.mark.parametrize("gated", [False, True], ids=["all-ones", "gated"])
def test_verdicts_of_the_derived_field(ctx, gated):
    best, act, kin = ic.field(gated)
    for ratio in ic.RATIOS:
        keep, counts = _check_verdict(ctx, best, act, kin, ic.FIELD_W, ic.FIELD_H, ic.FIELD_BLOCK, ratio, 0, f"q {ratio}")
        np.testing.assert_array_equal(keep, ic.field_keep(ratio, gated))               # the hand-derived flags, of the library itself
        assert counts == ic.FIELD_COUNTS[(ratio, gated)]
    cut_at, none_at = ic.FIELD_CUT[gated]
    keep, _ = _check_verdict(ctx, best, act, kin, ic.FIELD_W, ic.FIELD_H, ic.FIELD_BLOCK, 8, cut_at, f"P {cut_at}")
    assert not keep.any()
    keep, _ = _check_verdict(ctx, best, act, kin, ic.FIELD_W, ic.FIELD_H, ic.FIELD_BLOCK, 8, none_at, f"P {none_at}")
    np.testing.assert_array_equal(keep, ic.field_keep(8, gated))
    keep, counts = _check_verdict(ctx, best, act, np.zeros(12, np.uint8), ic.FIELD_W, ic.FIELD_H, ic.FIELD_BLOCK, 8, 1, "no candidate")
    assert counts == (0, 0) and not keep.any()
    _check_verdict(ctx, best, act, np.zeros(12, np.uint8), ic.FIELD_W, ic.FIELD_H, ic.FIELD_BLOCK, 8, 0, "no candidate, P 0")


def test_verdicts_on_a_synthetic_lattice(ctx):
    """120 x 67 = 8,040 blocks: 8 workgroups of 1,024, the last one partial (872); equalities, flat blocks and unkept blocks among them"""
    best, act, kin = ic.synthetic(120, 67)
    for ratio, cut in ((8, 0), (1, 0), (255, 0), (8, 30), (8, 100)):
        _check_verdict(ctx, best, act, kin, 1920, 1080, 16, ratio, cut, f"synthetic q {ratio} P {cut}")
    _check_verdict(ctx, best, act, None, 1920, 1080, 16, 8, 0, "synthetic without keep_in")


def test_scene_cut_threshold(ctx):
    F, act = mc.scene_vectors()[1], ic.scene_activity()
    keep, counts = ctx.sad_intra(F, act, None, mc.SCENE_W, mc.SCENE_H, B, Q, ic.SCENE_NO_CUT)
    assert tuple(counts) == (96, 23) and int(keep.sum()) == 73                          # 2300 < 2304
    keep, counts = ctx.sad_intra(F, act, None, mc.SCENE_W, mc.SCENE_H, B, Q, ic.SCENE_CUT)
    assert tuple(counts) == (96, 23) and not keep.any()                                 # 2300 >= 2208
    np.testing.assert_array_equal(ctx.block_activity(mc.scene()[1], B).reshape(-1), act)


# --------------------------------------------------------------------------------------------------------------- the scene through the search
def _scene_gate(gate):
    return None if not gate else gc.keep_flags(mc.scene()[1], B, gate).astype(np.uint8)


def _scene_want(intra, cut=0, gate=0, limit=0, median=0, F=None, G=None):
    """the restatements chained as the definition chains them: gate AND NOT intra -> AND check -> median over those; the cut from gate and
    intra alone, vetoing the final flags.  F, G: the integer winners of both directions (default: the plain search's)"""
    F = mc.scene_vectors()[1] if F is None else F
    kin = _scene_gate(gate)
    keep, (n_cand, n_intra), _ = ii.verdict(F, ic.scene_activity(), kin, intra, 0)
    if limit:
        G = mc.scene_vectors(reverse=True)[1] if G is None else G
        keep = keep & cc.keep_flags(F, G, mc.SCENE_W, mc.SCENE_H, B, limit).astype(np.uint8)
    if median:
        keep = im.keep_flags(F, keep, mc.SCENE_NBX, mc.SCENE_NBY, median)
    if cut and 100 * n_intra >= cut * n_cand:
        keep = np.zeros_like(keep)
    return keep.astype(bool)


def test_sad_flow_follows_the_contexts_ratio(ctx):
    prev, cur = mc.scene()
    ent0, F = mc.scene_vectors()
    for q in ic.SCENE_RATIOS:
        keep = ic.scene_keep(q).astype(bool)
        with _settings(ctx, intra=q):
            assert ctx.get_sad_intra() == q
            ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
            ent_only = ctx.sad_flow(prev, cur, B, R)
        assert len(ent) == len(best) == ic.SCENE_KEPT[q], q
        np.testing.assert_array_equal(_bits(ent), _bits(ent0[keep]), err_msg=f"q {q}: records")
        np.testing.assert_array_equal(best, F[keep], err_msg=f"q {q}: out_best")
        np.testing.assert_array_equal(_bits(ent_only), _bits(ent))
    for kw in (dict(cut=ic.SCENE_NO_CUT), dict(cut=ic.SCENE_CUT), dict(gate=1), dict(limit=1), dict(median=2), dict(gate=1, limit=1, median=2),
               dict(gate=1, cut=30)):
        keep = _scene_want(Q, **kw)
        with _settings(ctx, intra=Q, **kw):
            ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
        np.testing.assert_array_equal(_bits(ent), _bits(ent0[keep]), err_msg=f"{kw}: records")
        np.testing.assert_array_equal(best, F[keep], err_msg=f"{kw}: out_best")
    assert not _scene_want(Q, cut=ic.SCENE_CUT).any() and _scene_want(Q, cut=ic.SCENE_NO_CUT).sum() == 73
    with _settings(ctx, cut=50):                                                        # P alone: accepted, no effect
        ent = ctx.sad_flow(prev, cur, B, R)
    np.testing.assert_array_equal(_bits(ent), _bits(ent0))


def test_noise_against_noise_gives_no_record(ctx):
    prev, cur, ent0, F = mc.sparse_pair()
    for q in (1, 8, 16):
        with _settings(ctx, intra=q):
            ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
            ctx.reset_frames()
            ctx.push_frame(prev, **_prm(1))
            r = ctx.push_frame(cur, want_entries=True, want_field=True, **_prm(2))
            ctx.reset_frames()
        assert len(ent) == len(best) == 0, q
        assert r["have_vectors"] and r["n_vectors"] == 0 and r["motion"] is None
        np.testing.assert_array_equal(r["quat"], IDENTITY)


def _flow_intra_dev(ctx, frames, ref_mode, gate, limit, median, intra, cut, pitch_extra=0, want_best=True):
    """frames [n, H, W] -> per pair (records, triples) of ofps_hip_sad_flow_intra_dev; frames `pitch_extra` bytes further apart than a frame,
    64 guard words behind every output"""
    import torch
    n, H, W = frames.shape
    nblk = (W // B) * (H // B)
    pitch = W * H + pitch_extra
    buf = np.full((n, pitch), 255, np.uint8)
    buf[:, :W * H] = np.asarray(frames).reshape(n, -1)
    d = torch.from_numpy(buf).cuda()
    d_ent = torch.full(((n - 1) * nblk * 4 + 64,), np.nan, dtype=torch.float32, device="cuda")
    d_best = torch.full(((n - 1) * nblk * 3 + 64,), -77, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n - 1 + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_flow_intra_dev(d.data_ptr(), n, W, H, W, pitch, ref_mode, B, R, gate, limit, median, intra, cut, d_ent.data_ptr(),
                           d_best.data_ptr() if want_best else None, d_cnt.data_ptr())
    ctx.sync()
    ent, best, cnt = d_ent.cpu().numpy(), d_best.cpu().numpy(), d_cnt.cpu().numpy()
    assert np.isnan(ent[(n - 1) * nblk * 4:]).all() and (best[(n - 1) * nblk * 3:] == -77).all() and (cnt[n - 1:] == -1).all(), "guard words"
    ent, best = ent[:(n - 1) * nblk * 4].reshape(n - 1, nblk, 4), best[:(n - 1) * nblk * 3].reshape(n - 1, nblk, 3)
    return [(ent[k, :cnt[k]], best[k, :cnt[k]]) for k in range(n - 1)]


@pytest.mark.parametrize("kw", [dict(), dict(gate=1), dict(limit=1), dict(median=2), dict(gate=1, limit=1, median=2), dict(cut=ic.SCENE_CUT),
                                dict(cut=ic.SCENE_NO_CUT)], ids=["alone", "gate1", "check1", "median2", "all", "cut", "no-cut"])
def test_intra_dev_form_with_explicit_values(ctx, kw):
    prev, cur = mc.scene()
    ent0, F = mc.scene_vectors()
    keep = _scene_want(Q, **kw)
    assert ctx.get_sad_intra() == 0 and ctx.get_sad_cut() == 0                          # the device form takes its own values
    (ent, best), = _flow_intra_dev(ctx, np.stack([prev, cur]), 0, kw.get("gate", 0), kw.get("limit", 0), kw.get("median", 0), Q, kw.get("cut", 0))
    assert len(ent) == int(keep.sum())
    np.testing.assert_array_equal(_bits(ent), _bits(ent0[keep]))
    np.testing.assert_array_equal(best, F[keep])
    (ent, _), = _flow_intra_dev(ctx, np.stack([prev, cur]), 0, kw.get("gate", 0), kw.get("limit", 0), kw.get("median", 0), Q, kw.get("cut", 0),
                               want_best=False)
    np.testing.assert_array_equal(_bits(ent), _bits(ent0[keep]))


@pytest.mark.parametrize("n_frames,ref_mode", [(3, 0), (4, 0), (4, 1)], ids=["2-items", "3-items", "3-items-key"])
def test_intra_dev_form_over_items_with_a_padded_pitch(ctx, n_frames, ref_mode):
    """items of one launch: the activity of item k is the current frame of pair k, `pitch` > a frame behind the previous one's; one item is
    a cut by the rule.  The yardstick is the same call on each pair alone, which the tests above hold to the restatement, and the restated
    counts"""
    f = ic.stream_frames()[:n_frames]
    got = _flow_intra_dev(ctx, f, ref_mode, 0, 0, 0, ic.STREAM_Q, ic.STREAM_P, pitch_extra=200)
    for k, (ent, best) in enumerate(got):
        (e1, b1), = _flow_intra_dev(ctx, np.stack([f[0 if ref_mode else k], f[k + 1]]), 0, 0, 0, 0, ic.STREAM_Q, ic.STREAM_P)
        np.testing.assert_array_equal(_bits(ent), _bits(e1), err_msg=f"item {k}")
        np.testing.assert_array_equal(best, b1, err_msg=f"item {k}")
        if not ref_mode:
            assert len(ent) == ic.STREAM_KEPT[k + 1], k
            np.testing.assert_array_equal(_bits(ent), _bits(ic.stream_expect(k + 1)[0]), err_msg=f"item {k}")
            np.testing.assert_array_equal(best, ic.stream_expect(k + 1)[1], err_msg=f"item {k}")
    if not ref_mode:
        assert [len(e) for e, _ in got][:2] == [73, 0]


MODES = {  # id: (settings of the search, the integer winners are the restatement's plain ones)
    "scale4": (dict(scale=4), True),
    "levels2-predictors": (dict(levels=2, predictors=1), False),
    "prefilter4": (dict(prefilter=4), False),
    "pruned": (dict(pruned=True), True),
    "scale4-levels2-check1": (dict(scale=4, levels=2, limit=1), False),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_scene_in_the_other_search_modes(ctx, mode):
    """the records are the mode's unfiltered ones (quarter-pel at scale 4), the verdicts the INTEGER winners' SADs against the RAW frame's
    activities (mean removal: the filtered frames' SADs), the triples the mode's compacted"""
    kw, plain = MODES[mode]
    prev, cur = mc.scene()
    check = kw.get("limit", 0)
    search = {k: v for k, v in kw.items() if k != "limit"}
    with _settings(ctx, **search):
        e_ref, b_ref = ctx.sad_flow(prev, cur, B, R, want_best=True)                    # what the caller gets, unfiltered
    with _settings(ctx, **dict(search, scale=1)):
        F = ctx.sad_flow(prev, cur, B, R, want_best=True)[1]                            # the mode's integer winners
        G = ctx.sad_flow(cur, prev, B, R, want_best=True)[1]
    if plain:
        np.testing.assert_array_equal(F, mc.scene_vectors()[1])
    keep = _scene_want(Q, limit=check, F=F, G=G)
    assert 0 < int(keep.sum()) < mc.SCENE_NBLK
    with _settings(ctx, intra=Q, **kw):
        ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
        (ent_dev, best_dev), = _flow_intra_dev(ctx, np.stack([prev, cur]), 0, 0, check, 0, Q, 0)
    for e, b, what in ((ent, best, "sad_flow"), (ent_dev, best_dev, "intra_dev")):
        assert len(e) == int(keep.sum()), f"{mode} {what}"
        np.testing.assert_array_equal(_bits(e), _bits(e_ref[keep]), err_msg=f"{mode} {what}: records")
        np.testing.assert_array_equal(b, b_ref[keep], err_msg=f"{mode} {what}: triples")
    if kw.get("scale") == 4:
        assert not np.array_equal(b_ref, F)              # quarter-pel triples went to the caller, integer winners to the test


# --------------------------------------------------------------------------------------------------------------- the fused path
def _prm(seed, use_ransac=False):
    return dict(block=B, search_range=R, detector=True, estimator=True, aspect=mc.SCENE_CAM[0], fov_y_deg=mc.SCENE_CAM[1], use_ransac=use_ransac,
                seed=seed, **mc.SCENE_DETECTOR, **mc.SCENE_RANSAC)


def _check_ticket(ctx, got, want_ent, seed, what):
    assert got["have"] and got["n"] == len(want_ent) == len(got["entries"]), what
    np.testing.assert_array_equal(_bits(got["entries"]), _bits(want_ent), err_msg=what + ": records")
    if got["n"] == 0:                                    # a cut: identity, no motion
        np.testing.assert_array_equal(got["quat"], IDENTITY, err_msg=what)
        assert got["motion"] is None, what
        return
    q = ctx.almeida(got["entries"], *mc.SCENE_CAM, use_ransac=False, seed=seed, **mc.SCENE_RANSAC)[0]
    want = ctx.detect(got["entries"], **mc.SCENE_DETECTOR)
    err = float(np.abs(got["quat"] - q).max())
    print(f"{what}: kept {got['n']}, quat {got['quat']} (|fused - almeida| {err:.3g}), area {gc.area_of(got['motion'])}")
    assert err <= QUAT_BOUND and np.isfinite(got["quat"]).all(), what
    assert (got["motion"] is None) == (want is None), what
    if want is not None:
        assert got["motion"][0] == want[0], what
        if got["motion"][1] is not None and not np.isscalar(got["motion"][1]):
            np.testing.assert_array_equal(_bits(got["motion"][1]), _bits(want[1]), err_msg=what + ": field")


def _single_pushes(ctx, frames, seeds):
    ctx.reset_frames()
    out = []
    for fr, s in zip(frames, seeds):
        r = ctx.push_frame(fr, want_entries=True, want_field=True, **_prm(s))
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=r["entries"], quat=r["quat"], motion=r["motion"]))
    ctx.reset_frames()
    return out


def test_fused_tickets_and_a_cut_frame(ctx):
    f = ic.stream_frames()
    seeds = [mc.SCENE_SEED + k for k in range(len(f))]
    with _settings(ctx):
        plain = _single_pushes(ctx, f[:2], seeds)
    with _settings(ctx, intra=ic.STREAM_Q, cut=ic.STREAM_P):
        got = _single_pushes(ctx, f, seeds)
    assert not got[0]["have"] and got[0]["motion"] is None
    np.testing.assert_array_equal(got[0]["quat"], IDENTITY)
    for k in range(1, len(f)):
        _check_ticket(ctx, got[k], ic.stream_expect(k)[0], seeds[k], f"fused ticket {k}")
    assert [g["n"] for g in got[1:]] == list(ic.STREAM_KEPT[1:]) and plain[1]["n"] == mc.SCENE_NBLK
    assert np.abs(got[1]["quat"] - plain[1]["quat"]).max() > 1e-5, "the estimator answered as without the test"
    with _settings(ctx, intra=ic.STREAM_Q):              # without the rule the cut pair keeps its 36 self-matching blocks
        assert _single_pushes(ctx, f[:3], seeds)[2]["n"] == ic.STREAM_KEPT_WITHOUT_CUT[2]
    with _settings(ctx, intra=Q, cut=ic.SCENE_CUT):      # the scene pair itself at the threshold: 2300 >= 2208
        r = _single_pushes(ctx, f[:2], seeds)[1]
    assert r["have"] and r["n"] == 0 and r["motion"] is None
    np.testing.assert_array_equal(r["quat"], IDENTITY)


def test_fused_async_pair_of_tickets(ctx):
    """frames prev, cur, half with two tickets in flight, gate and median test on as well: the pairs (prev, cur) and (cur, half), a cut"""
    f = ic.stream_frames()[:3]
    dim = ctx.block_dim(mc.SCENE_DETECTOR["min_size"], mc.SCENE_DETECTOR["subdivide"])
    pins = [ctx.pinned_frame(mc.SCENE_H, mc.SCENE_W) for _ in range(3)]
    ents = [ctx.pinned_array((mc.SCENE_NBLK, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    out, tickets = [], []

    def collect(k):
        r = ctx.frame_wait(tickets[k])
        m = None if r["motion"] is None else (r["motion"][0], flds[k % 2].copy())
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=ents[k % 2][:r["n_vectors"]].copy() if r["have_vectors"] else None,
                        quat=r["quat"], motion=m))

    try:
        with _settings(ctx, intra=ic.STREAM_Q, cut=ic.STREAM_P, gate=1, median=2):
            ctx.reset_frames()
            for k in range(3):
                if k >= 2:
                    collect(k - 2)
                np.copyto(pins[k], f[k])
                tickets.append(ctx.push_frame_async(pins[k], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(mc.SCENE_SEED + k)))
            collect(1)
            collect(2)
    finally:
        ctx.reset_frames()
        for p in pins + ents + flds:
            ctx.free_pinned(p)
    assert not out[0]["have"]
    keep = _scene_want(ic.STREAM_Q, cut=ic.STREAM_P, gate=1, median=2)
    assert 0 < keep.sum() < 73
    _check_ticket(ctx, out[1], mc.scene_vectors()[0][keep], mc.SCENE_SEED + 1, "async ticket 1")
    _check_ticket(ctx, out[2], np.zeros((0, 4), np.float32), mc.SCENE_SEED + 2, "async ticket 2")


def test_batched_form_with_the_batch_filter_equals_single_pushes(ctx):
    """two tickets of three frames, one frame of each a cut by the rule"""
    f = np.ascontiguousarray(ic.stream_frames())
    seeds = [mc.SCENE_SEED + k for k in range(len(f))]
    with _settings(ctx, intra=ic.STREAM_Q, cut=ic.STREAM_P, batch_filter=1):
        want = _single_pushes(ctx, f, seeds)
        bufs = [ctx.pinned_array((3, mc.SCENE_H, mc.SCENE_W), np.uint8) for _ in range(2)]
        ents = [ctx.pinned_array((3, mc.SCENE_NBLK, 4)) for _ in range(2)]
        try:
            ctx.reset_frames()
            tickets = []
            for j in range(2):
                np.copyto(bufs[j], f[3 * j:3 * j + 3])
                tickets.append(ctx.push_frames_async(bufs[j], out_entries=ents[j], **_prm(seeds[3 * j])))
            res = [r for t in tickets for r in ctx.frames_wait(t)]
            got_ent = [ents[k // 3][k % 3].copy() for k in range(6)]
        finally:
            ctx.reset_frames()
            for p in bufs + ents:
                ctx.free_pinned(p)
    with _settings(ctx, intra=ic.STREAM_Q, cut=ic.STREAM_P):       # the switch off: the batched form ignores both fields
        buf = ctx.pinned_array((3, mc.SCENE_H, mc.SCENE_W), np.uint8)
        try:
            np.copyto(buf, f[:3])
            off = ctx.frames_wait(ctx.push_frames_async(buf, **_prm(seeds[0])))
        finally:
            ctx.reset_frames()
            ctx.free_pinned(buf)
    assert [r["n_vectors"] for r in off] == [0, mc.SCENE_NBLK, mc.SCENE_NBLK]
    assert not res[0]["have_vectors"] and res[0]["n_vectors"] == 0
    assert [r["n_vectors"] for r in res[1:]] == list(ic.STREAM_KEPT[1:])
    for k in range(1, 6):
        w, r = want[k], res[k]
        assert r["have_vectors"] and r["n_vectors"] == w["n"], k
        np.testing.assert_array_equal(_bits(got_ent[k][:w["n"]]), _bits(w["entries"]), err_msg=f"frame {k}")
        np.testing.assert_array_equal(_bits(w["entries"]), _bits(ic.stream_expect(k)[0]), err_msg=f"frame {k}")
        assert (r["motion"] is None) == (w["motion"] is None), k
        if w["motion"] is not None:
            assert r["motion"][0] == w["motion"][0], k                                  # the island's area
        assert np.abs(r["quat"] - w["quat"]).max() <= QUAT_BOUND, k
        if w["n"] == 0:
            np.testing.assert_array_equal(r["quat"], IDENTITY)


def test_multi_device_workers_take_ratio_and_cut_from_the_environment():
    env = dict(os.environ, OFPS_HIP_SAD_INTRA=str(ic.STREAM_Q), OFPS_HIP_SAD_CUT=str(ic.STREAM_P), OFPS_HIP_SAD_BATCH_FILTER="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_intra_child.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert [s["have_vectors"] for s in out] == [False] + [True] * 5
    assert [s["n_vectors"] for s in out[1:]] == list(ic.STREAM_KEPT[1:])
    for k in range(1, 6):
        assert out[k]["entries"] == _bits(ic.stream_expect(k)[0]).reshape(-1).tolist(), k
        if ic.STREAM_KEPT[k] == 0:
            assert out[k]["quat"] == _bits(IDENTITY).tolist() and out[k]["motion"] is None, k


# --------------------------------------------------------------------------------------------------------------- off, errors, scope
def test_ratio_0_after_ratio_8_equals_a_fresh_context(ctx):
    from ofps_amd.runtime import HipContext
    prev, cur = mc.scene()

    def run(c):
        c.reset_frames()
        c.push_frame(prev, **_prm(mc.SCENE_SEED))
        r = c.push_frame(cur, want_entries=True, want_field=True, **_prm(mc.SCENE_SEED + 1))
        c.reset_frames()
        return r, c.sad_flow(prev, cur, B, R, want_best=True)

    fresh = HipContext(0)
    try:
        ref, ref_sad = run(fresh)                         # a context that never saw the test
    finally:
        fresh.close()
    with _settings(ctx, intra=Q, cut=ic.SCENE_NO_CUT):
        on, on_sad = run(ctx)
    assert on["n_vectors"] == len(on_sad[0]) == 73
    assert ctx.get_sad_intra() == 0 and ctx.get_sad_cut() == 0
    again, again_sad = run(ctx)
    assert again["n_vectors"] == mc.SCENE_NBLK
    np.testing.assert_array_equal(_bits(again_sad[0]), _bits(ref_sad[0]))
    np.testing.assert_array_equal(again_sad[1], ref_sad[1])
    np.testing.assert_array_equal(_bits(again["entries"]), _bits(ref["entries"]))
    np.testing.assert_array_equal(_bits(again["quat"]), _bits(ref["quat"]))
    assert (again["motion"] is None) == (ref["motion"] is None)
    if ref["motion"] is not None:
        assert again["motion"][0] == ref["motion"][0]
        np.testing.assert_array_equal(_bits(again["motion"][1]), _bits(ref["motion"][1]))


def test_forms_that_ignore_both_fields(ctx):
    import torch
    prev, cur = mc.scene()
    ent0, F = mc.scene_vectors()
    with _settings(ctx, intra=Q, cut=ic.SCENE_CUT):
        d = torch.from_numpy(np.stack([prev, cur])).cuda()
        d_ent = torch.zeros((mc.SCENE_NBLK, 4), dtype=torch.float32, device="cuda")
        d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.sad_flow_dev(d.data_ptr(), 2, mc.SCENE_W, mc.SCENE_H, mc.SCENE_W, mc.SCENE_W * mc.SCENE_H, 0, B, R, d_ent.data_ptr())
        ctx.sync()
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()), _bits(ent0))          # nblk records
        # the explicit-argument forms take their own values and nobody else's
        ctx.sad_flow_filtered_dev(d.data_ptr(), 2, mc.SCENE_W, mc.SCENE_H, mc.SCENE_W, mc.SCENE_W * mc.SCENE_H, 0, B, R, 0, 0, 2, d_ent.data_ptr(),
                                  None, d_cnt.data_ptr())
        ctx.sync()
        keep = mc.scene_keep(2).astype(bool)
        assert int(d_cnt.cpu().numpy()[0]) == int(keep.sum())
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()[:int(keep.sum())]), _bits(ent0[keep]))
        ctx.sad_flow_median_dev(d[0].data_ptr(), d[1].data_ptr(), mc.SCENE_W, mc.SCENE_H, mc.SCENE_W, B, R, 0, 0, 2, d_ent.data_ptr(), None,
                                d_cnt.data_ptr())
        ctx.sync()
        assert int(d_cnt.cpu().numpy()[0]) == int(keep.sum())


def test_bad_values_and_the_options(ctx):
    import torch
    from ofps_amd import _lib
    from ofps_amd.runtime import OfpsHipError
    lib = _lib.load()
    assert ctx.get_sad_intra() == 0 and ctx.get_sad_cut() == 0
    for name, setter, getter, top in (("intra", lib.ofps_hip_set_sad_intra, ctx.get_sad_intra, 255), ("cut", lib.ofps_hip_set_sad_cut, ctx.get_sad_cut, 100)):
        for bad in (-1, top + 1, 1 << 20):
            assert setter(ctx._h, bad) == EINVAL and getter() == 0, name
            assert str(bad) in lib.ofps_hip_last_error(ctx._h).decode()                 # the value is in the message
        for ok in (top, 1, 0):
            assert setter(ctx._h, ok) == 0 and getter() == ok, name
    ctx.set_sad_cut(100)                                 # accepted while the ratio is 0
    assert ctx.get_sad_cut() == 100 and ctx.get_sad_intra() == 0
    ctx.set_sad_cut(0)
    best, act, _ = ic.field()
    for ratio, cut in ((0, 0), (-1, 0), (256, 0), (8, -1), (8, 101)):                   # the standalone forms: ratio in [1, 255], cut in [0, 100]
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_intra(best, act, None, ic.FIELD_W, ic.FIELD_H, ic.FIELD_BLOCK, ratio, cut)
        assert ei.value.code == EINVAL, (ratio, cut)
    d = torch.zeros(96 * 64, dtype=torch.int32, device="cuda")                          # real device memory behind every pointer: these calls must
    torch.cuda.synchronize()                                                            # be refused before anything is enqueued, but are not trusted to
    p = d.data_ptr()
    for args in ((p, p, None, 35, 29, 65, 8, 0, p, None),  # block outside [1, 64]
                 (0, p, None, 35, 29, 8, 8, 0, p, None),   # null winners
                 (p, 0, None, 35, 29, 8, 8, 0, p, None),   # null activities
                 (p, p, None, 35, 29, 8, 8, 0, 0, None),   # null flags
                 (p, p, None, 35, 29, 8, 0, 0, p, None), (p, p, None, 35, 29, 8, 8, 101, p, None)):
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_intra_dev(*args)
        assert ei.value.code == EINVAL, args
    for args in ((0, 96, 64, 96, 8, p), (p, 96, 64, 95, 8, p), (p, 96, 64, 96, 0, p), (p, 96, 64, 96, 65, p), (p, 96, 64, 96, 8, 0)):
        with pytest.raises(OfpsHipError) as ei:
            ctx.block_activity_dev(*args)
        assert ei.value.code == EINVAL, args
    for mp, limit, med, intra, cut in ((0, 0, 0, 0, 0), (0, 0, 0, 256, 0), (0, 0, 0, -1, 0), (0, 0, 0, 8, 101), (0, 0, 0, 8, -1), (-1, 0, 0, 8, 0),
                                       (65, 0, 0, 8, 0), (0, -1, 0, 8, 0), (0, 130, 0, 8, 0), (0, 0, 256, 8, 0)):
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow_intra_dev(p, 2, 96, 64, 96, 96 * 64, 0, 8, 8, mp, limit, med, intra, cut, p, None, p)
        assert ei.value.code == EINVAL, (mp, limit, med, intra, cut)
    ctx.sync()
    for opt, getter, top in (("OFPS_HIP_SAD_INTRA", ctx.get_sad_intra, 255), ("OFPS_HIP_SAD_CUT", ctx.get_sad_cut, 100)):
        ctx.set_option(opt, 3)                           # the option table sets the same field
        assert getter() == 3
        for bad in (-3, top + 1):
            with pytest.raises(OfpsHipError) as ei:
                ctx.set_option(opt, bad)
            assert ei.value.code == EINVAL and getter() == 3 and str(bad) in str(ei.value)
        ctx.set_option(opt, None)
        assert getter() == 0


def test_plugin_properties():
    from ofps_amd.plugins import HipSadDecoder
    f = ic.stream_frames()
    dec = HipSadDecoder(iter([f[0], f[1], f[2], f[3]]))
    try:
        names = [p[0] for p in dec.props()]
        assert ("Intra test", "usize", 0, 0, 255) in dec.props() and ("Scene cut", "usize", 0, 0, 100) in dec.props()
        assert names.index("Median test") + 1 == names.index("Intra test") and names.index("Intra test") + 1 == names.index("Scene cut")
        assert dec.set_prop("Block size", B) and dec.set_prop("Search range", R)
        field = []
        assert dec.process_frame(field) is False
        assert dec.set_prop("Intra test", ic.STREAM_Q) and dec.set_prop("Scene cut", ic.STREAM_P)
        assert dec.process_frame(field) is True and dec.ctx.get_sad_intra() == ic.STREAM_Q and dec.ctx.get_sad_cut() == ic.STREAM_P
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(ic.stream_expect(1)[0]))
        field = []
        assert dec.process_frame(field) is True and field == []          # a cut frame: Ok(true) with an empty list
        assert dec.set_prop("Intra test", 0)
        assert dec.process_frame(field) is True and len(field) == mc.SCENE_NBLK
    finally:
        dec.ctx.close()
