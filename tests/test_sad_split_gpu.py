"""-m gpu: hip_sad's split blocks (include/ofps_hip.h N1s) through the C ABI, bit-exact against the restatement
tests/indep_sad_split.py: the step alone (ofps_hip_sad_split[_dev]) on every case and threshold of tests/sad_split_cases.py, the search forms
(ofps_hip_sad_flow, ofps_hip_sad_flow_split_dev) alone and composed with gate + median test, mean removal and levels + predictors, T = 0
against a context that never heard of the setter, the refusals, the fused per-frame forms and the decoder's property.
Inputs and expectations are computed once per process and shared read-only."""
import json
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from ofps_amd import mvec
from ofps_amd._lib import OfpsHipError

import indep_sad_hier as ih
import indep_sad_median as im
import indep_sad_pred as ip
import indep_sad_prefilter as ipf
import indep_sad_split as isp
import sad_gate_cases as gc
import sad_split_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool")
EINVAL, EUNSUPPORTED = -1, -3
QUAT_BOUND = 2e-6                                         # the fused path's documented parity with ofps_hip_almeida (include/ofps_hip.h N1g)
W, H, B, R = sc.STREAM_W, sc.STREAM_H, sc.STREAM_B, sc.STREAM_R
NBLK = (W // B) * (H // B)
T = sc.STREAM_T


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_step(got, want, what):
    np.testing.assert_array_equal(got["sub_best"], want["sub_best"], err_msg=what + ": sub triples")
    np.testing.assert_array_equal(got["split"], want["split"], err_msg=what + ": split flags")
    if got["entries"] is not None:
        np.testing.assert_array_equal(got["slot_flags"], want["slot_flags"], err_msg=what + ": slot flags")
        np.testing.assert_array_equal(_bits(got["entries"]), _bits(want["entries"]), err_msg=what + ": raw records")


class _settings:
    """context settings for the length of a block; everything back to the defaults behind it"""
    DEFAULT = dict(split=0, median=0, gate=0, scale=1, levels=1, predictors=0, prefilter=0)

    def __init__(self, ctx, **kw):
        self.ctx, self.v = ctx, dict(self.DEFAULT, **kw)

    def _apply(self, v):
        c = self.ctx
        c.set_sad_split(v["split"]); c.set_sad_median(v["median"]); c.set_sad_gate(v["gate"]); c.set_sad_motion_scale(v["scale"])
        c.set_sad_levels(v["levels"]); c.set_sad_predictors(v["predictors"]); c.set_sad_prefilter(v["prefilter"])

    def __enter__(self):
        self._apply(self.v)

    def __exit__(self, *exc):
        self._apply(self.DEFAULT)


# --------------------------------------------------------------------------------------------------------------- the step alone
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_step_alone_on_every_case_and_threshold(ctx, name):
    prev, cur = sc.pair(name)
    _, _, blk, rng = sc.geometry(name)
    best = sc.parents(name)
    for with_keep in (False, True):
        keep = sc.keep_pattern(len(best)) if with_keep else None
        for t in sc.THRESHOLDS:
            want = sc.expect(name, t, with_keep)
            _same_step(ctx.sad_split(prev, cur, blk, best, keep, rng, t), want, f"{name} T={t} keep={with_keep}")
    want = sc.expect(name, 16)
    _same_step(ctx.sad_split(prev, cur, blk, best, None, rng, 16, want_entries=False), want, f"{name}: without records")
    pp, pc = sc.padded(prev), sc.padded(cur)                                           # padded rows: stride = W + 12
    _same_step(ctx.sad_split(pp, pc, blk, best, None, rng, 16, stride=pp.strides[0]), want, f"{name}: padded rows")


def _split_dev(ctx, prev, cur, stride, blk, best, keep, reach, t):
    """the _dev form on frames with rows of `stride` bytes; every output starts as 0xEE"""
    import torch
    Hh, Ww = prev.shape
    nblk = len(best)
    frames = np.full((2, Hh, stride), 255, np.uint8)
    frames[0, :, :Ww] = prev; frames[1, :, :Ww] = cur
    d_fr = torch.from_numpy(frames).cuda()
    d_best = torch.from_numpy(np.array(best)).cuda()
    d_keep = None if keep is None else torch.from_numpy(np.array(keep)).cuda()
    d_sub = torch.full((nblk, 4, 3), -286331154, dtype=torch.int32, device="cuda")
    d_split = torch.full((nblk,), 0xEE, dtype=torch.uint8, device="cuda")
    d_ent = torch.full((nblk, 4, 4), float("nan"), dtype=torch.float32, device="cuda")
    d_slot = torch.full((nblk, 4), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_split_dev(d_fr[0].data_ptr(), d_fr[1].data_ptr(), Ww, Hh, stride, blk, d_best.data_ptr(), None if keep is None else d_keep.data_ptr(),
                      reach, t, d_sub.data_ptr(), d_split.data_ptr(), d_ent.data_ptr(), d_slot.data_ptr())
    ctx.sync()
    return {"sub_best": d_sub.cpu().numpy(), "split": d_split.cpu().numpy(), "entries": d_ent.cpu().numpy(), "slot_flags": d_slot.cpu().numpy()}


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_step_through_the_dev_form(ctx, name):
    """dense rows, rows padded by 12 (4-byte aligned: the packed kernels at block 16 and 8) and by 13 (the byte-wise kernel for every block)"""
    prev, cur = sc.pair(name)
    Ww, _, blk, rng = sc.geometry(name)
    best = sc.parents(name)
    for stride in (Ww, Ww + sc.PAD, Ww + 13):
        for with_keep in (False, True):
            keep = sc.keep_pattern(len(best)) if with_keep else None
            got = _split_dev(ctx, prev, cur, stride, blk, best, keep, rng, 16)
            _same_step(got, sc.expect(name, 16, with_keep), f"{name} stride={stride} keep={with_keep}")


@pytest.mark.parametrize("name", ["boundary24", "small_blocks", "generic12"])
def test_step_on_wild_parents(ctx, name):
    """triples far outside any search, and a negative SAD: every predictor is clamped into the frame, the rule is signed"""
    prev, cur = sc.pair(name)
    _, _, blk, rng = sc.geometry(name)
    best = sc.wild_parents(len(sc.parents(name)))
    want = isp.split_step(prev, cur, blk, best, None, rng, 16)
    _same_step(ctx.sad_split(prev, cur, blk, best, None, rng, 16), want, name)


# --------------------------------------------------------------------------------------------------------------- the search forms
def _flow_split_dev(ctx, prev, cur, blk, rng, gate, limit, median, t):
    import torch
    Hh, Ww = prev.shape
    nblk = (Ww // blk) * (Hh // blk)
    d_prev, d_cur = torch.from_numpy(np.array(prev)).cuda(), torch.from_numpy(np.array(cur)).cuda()
    d_ent = torch.zeros((4 * nblk, 4), dtype=torch.float32, device="cuda")
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_flow_split_dev(d_prev.data_ptr(), d_cur.data_ptr(), Ww, Hh, Ww, blk, rng, gate, limit, median, t, d_ent.data_ptr(), d_cnt.data_ptr())
    ctx.sync()
    n = int(d_cnt.cpu().numpy()[0])
    return d_ent.cpu().numpy()[:n]


@pytest.mark.parametrize("name", ["boundary24", "boundary28", "noise_only", "ragged", "one_block", "small_blocks", "corner_minus"])
def test_search_forms_on_the_cases(ctx, name):
    prev, cur = sc.pair(name)
    Ww, Hh, blk, rng = sc.geometry(name)
    best = sc.parents(name)
    for t in (1, 16, 4080):
        want = isp.records(sc.expect(name, t))
        assert len(want) == len(best) + 3 * int(sc.expect(name, t)["split"].sum())
        with _settings(ctx, split=t):
            assert ctx.sad_record_capacity(Ww, Hh, blk) == 4 * len(best)
            ent, tri = ctx.sad_flow(prev, cur, blk, rng, want_best=True)
        assert len(ent) == len(want), f"{name} T={t}"
        np.testing.assert_array_equal(_bits(ent), _bits(want), err_msg=f"{name} T={t}: sad_flow")
        np.testing.assert_array_equal(tri, best, err_msg=f"{name} T={t}: the triples stay the parents'")
        if Ww % 4 == 0:
            dev = _flow_split_dev(ctx, prev, cur, blk, rng, 0, 0, 0, t)
            assert len(dev) == len(want)
            np.testing.assert_array_equal(_bits(dev), _bits(want), err_msg=f"{name} T={t}: sad_flow_split_dev")
    assert ctx.get_sad_split() == 0 and ctx.sad_record_capacity(Ww, Hh, blk) == len(best)


@pytest.mark.parametrize("geometry", [(320, 208, 16), (1920, 1080, 16), (1920, 1080, 8)], ids=["1040-slots", "32160-slots", "129600-slots"])
def test_large_lattices_compact_like_the_raw_slots(ctx, geometry):
    """lattices past the restatement's reach, on both sides of the size at which the compaction changes kernels: the search form's records
    are the step's raw slots (ofps_hip_sad_split on the plain search's winners) compacted on the host, and the count is the flags' sum"""
    from ofps_amd import synth
    Ww, Hh, blk = geometry
    fr = synth.luma_sequence(2, Ww, Hh, max_step=8)
    _, best = ctx.sad_flow(fr[0], fr[1], blk, 8, want_best=True)
    step = ctx.sad_split(fr[0], fr[1], blk, best, None, 8, T)
    want = isp.records(step)
    assert step["split"].any() and len(want) == len(best) + 3 * int(step["split"].sum())
    with _settings(ctx, split=T):
        ent = ctx.sad_flow(fr[0], fr[1], blk, 8)
    np.testing.assert_array_equal(_bits(ent), _bits(want))
    np.testing.assert_array_equal(_bits(_flow_split_dev(ctx, fr[0], fr[1], blk, 8, 0, 0, 0, T)), _bits(want))


@lru_cache(maxsize=1)
def _stream_pair():
    s = sc.stream()
    return s[0], s[1]


def test_search_with_gate_and_median_test(ctx):
    prev, cur = _stream_pair()
    best = ipf.full_search(prev, cur, B, R)
    kin = gc.keep_flags(cur, B, 1).astype(np.uint8)
    keep = im.keep_flags(best, kin, W // B, H // B, 2)
    step = isp.split_step(prev, cur, B, best, keep, R, T)
    want = isp.records(step)
    assert 0 < int(keep.sum()) and step["split"].any() and len(want) == int(keep.sum()) + 3 * int(step["split"].sum())
    with _settings(ctx, split=T, gate=1, median=2):
        ent, tri = ctx.sad_flow(prev, cur, B, R, want_best=True)
    np.testing.assert_array_equal(_bits(ent), _bits(want))
    np.testing.assert_array_equal(tri[:int(keep.sum())], best[keep != 0])               # the parents' triples, compacted by the keep flags
    dev = _flow_split_dev(ctx, prev, cur, B, R, 1, 0, 2, T)
    np.testing.assert_array_equal(_bits(dev), _bits(want))


def test_search_with_mean_removal(ctx):
    prev, cur = _stream_pair()
    fp, fc = ipf.prefilter(prev, 4), ipf.prefilter(cur, 4)
    best = ipf.full_search(fp, fc, B, R)
    step = isp.split_step(fp, fc, B, best, None, R, T)                                  # the step reads the frames the search read
    assert step["split"].any()
    with _settings(ctx, split=T, prefilter=4):
        ent, tri = ctx.sad_flow(prev, cur, B, R, want_best=True)
    np.testing.assert_array_equal(tri, best)
    np.testing.assert_array_equal(_bits(ent), _bits(isp.records(step)))


def test_search_with_levels_and_predictors(ctx):
    prev, cur = _stream_pair()
    _, best, _, _ = ip.search(prev, cur, B, R, 2, ip.PRED_NEIGHBOURS)
    reach = ih.reach(R, 2)
    step = isp.split_step(prev, cur, B, best, None, reach, T)                           # level 0 only
    with _settings(ctx, split=T, levels=2, predictors=1):
        ent, tri = ctx.sad_flow(prev, cur, B, R, want_best=True)
    np.testing.assert_array_equal(tri, best)
    np.testing.assert_array_equal(_bits(ent), _bits(isp.records(step)))


# --------------------------------------------------------------------------------------------------------------- T = 0
def _prm(seed):
    return dict(block=B, search_range=R, detector=True, estimator=True, aspect=sc.STREAM_CAM[0], fov_y_deg=sc.STREAM_CAM[1], use_ransac=False,
                seed=seed, **sc.STREAM_DETECTOR)


def test_threshold_0_equals_a_context_that_never_heard_of_the_setter(ctx):
    from ofps_amd.runtime import HipContext
    prev, cur = _stream_pair()

    def run(c):
        c.reset_frames()
        c.push_frame(prev, **_prm(1))
        r = c.push_frame(cur, want_entries=True, want_field=True, **_prm(2))
        c.reset_frames()
        return r, c.sad_flow(prev, cur, B, R, want_best=True), c.sad_record_capacity(W, H, B)

    fresh = HipContext(0)
    try:
        ref, ref_sad, ref_cap = run(fresh)
    finally:
        fresh.close()
    with _settings(ctx, split=T):
        on, on_sad, on_cap = run(ctx)
    assert on_cap == 4 * NBLK and on["n_vectors"] == len(on_sad[0]) > NBLK
    ctx.set_sad_split(0)
    again, again_sad, again_cap = run(ctx)
    assert ref_cap == again_cap == NBLK and again["n_vectors"] == ref["n_vectors"] == NBLK and len(again_sad[0]) == NBLK
    np.testing.assert_array_equal(_bits(again_sad[0]), _bits(ref_sad[0]))
    np.testing.assert_array_equal(again_sad[1], ref_sad[1])
    np.testing.assert_array_equal(_bits(again["entries"]), _bits(ref["entries"]))
    np.testing.assert_array_equal(_bits(again["quat"]), _bits(ref["quat"]))
    assert (again["motion"] is None) == (ref["motion"] is None)
    if ref["motion"] is not None:
        assert again["motion"][0] == ref["motion"][0]
        np.testing.assert_array_equal(_bits(again["motion"][1]), _bits(ref["motion"][1]))


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    import torch
    from ofps_amd import _lib
    lib = _lib.load()
    prev, cur = sc.pair("boundary24")
    best = sc.parents("boundary24")
    assert ctx.get_sad_split() == 0
    for bad in (-1, 4081, 1 << 20):
        assert lib.ofps_hip_set_sad_split(ctx._h, bad) == EINVAL and ctx.get_sad_split() == 0
        assert str(bad) in lib.ofps_hip_last_error(ctx._h).decode()
    for ok in (4080, 1, 0):
        ctx.set_sad_split(ok)
        assert ctx.get_sad_split() == ok
    for t in (0, -1, 4081):                                  # the explicit calls: T in [1, 4080]
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_split(prev, cur, 16, best, None, 8, t)
        assert ei.value.code == EINVAL
    p15 = np.zeros((45, 60), np.uint8)
    for blk, frame in ((15, p15), (6, np.zeros((48, 60), np.uint8)), (66, np.zeros((132, 132), np.uint8))):        # odd B, b < 4, B > 64
        nb = (frame.shape[1] // blk) * (frame.shape[0] // blk)
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_split(frame, frame, blk, np.zeros((nb, 3), np.int32), None, 8, 16)
        assert ei.value.code == EINVAL, blk
    with pytest.raises(OfpsHipError) as ei:                  # R0 + 3 > 127
        ctx.sad_split(prev, cur, 16, best, None, 125, 16)
    assert ei.value.code == EINVAL
    d = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")      # real device memory behind every pointer: refused before anything is enqueued
    torch.cuda.synchronize()
    p = d.data_ptr()
    for blk, rng, t in ((15, 8, 16), (6, 8, 16), (16, 8, 0), (16, 8, 4081)):
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow_split_dev(p, p, 64, 48, 64, blk, rng, 0, 0, 0, t, p, p)
        assert ei.value.code == EINVAL, (blk, rng, t)
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_split_dev(p, p, 64, 48, 64, 16, 0, None, 8, 16, p, p)       # null parents
    assert ei.value.code == EINVAL
    try:
        ctx.set_sad_split(16)
        for blk in (15, 6):
            f = np.zeros((90, 90), np.uint8)
            with pytest.raises(OfpsHipError) as ei:
                ctx.sad_flow(f, f, blk, 8)
            assert ei.value.code == EINVAL, blk
        ctx.set_sad_levels(2)                                # range 62 at levels 2 reaches 127: the sub-blocks' candidates would reach 130
        big = np.zeros((256, 256), np.uint8)
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow(big, big, 16, 62)
        assert ei.value.code == EINVAL
        ctx.set_sad_split(0)
        assert len(ctx.sad_flow(big, big, 16, 62)) == 256                               # ... which the search alone takes
        ctx.set_sad_split(16)
        ctx.set_sad_levels(1)
        ctx.set_sad_motion_scale(4)                          # quarter-pel sub-block vectors: a later step
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow(prev, cur, 16, 8)
        assert ei.value.code == EUNSUPPORTED
        ctx.reset_frames()
        with pytest.raises(OfpsHipError) as ei:              # the fused form refuses before anything is uploaded
            ctx.push_frame(prev, block=16, search_range=8)
        assert ei.value.code == EUNSUPPORTED
    finally:
        ctx.set_sad_motion_scale(1); ctx.set_sad_levels(1); ctx.set_sad_split(0)
        ctx.reset_frames()
    ctx.sync()
    ctx.set_option("OFPS_HIP_SAD_SPLIT", 32)                 # the option table sets the same field
    assert ctx.get_sad_split() == 32
    for bad in (-3, 4081):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_SPLIT", bad)
        assert ei.value.code == EINVAL and ctx.get_sad_split() == 32 and str(bad) in str(ei.value)
    ctx.set_option("OFPS_HIP_SAD_SPLIT", None)
    assert ctx.get_sad_split() == 0


# --------------------------------------------------------------------------------------------------------------- the fused forms
def _check_ticket(ctx, got, prev, cur, t, seed, what):
    """a fused ticket against ofps_hip_sad_flow of its pair at the same threshold, ofps_hip_detect and ofps_hip_almeida on those records"""
    with _settings(ctx, split=t):
        want = ctx.sad_flow(prev, cur, B, R)
    assert got["have"] and got["n"] == len(want) == len(got["entries"]), what
    np.testing.assert_array_equal(_bits(got["entries"]), _bits(want), err_msg=what + ": records")
    q = ctx.almeida(want, *sc.STREAM_CAM, use_ransac=False, seed=seed)[0]
    det = ctx.detect(want, **sc.STREAM_DETECTOR)
    err = float(np.abs(got["quat"] - q).max())
    print(f"{what}: {got['n']} records, quat {got['quat']} (|fused - almeida| {err:.3g})")
    assert err <= QUAT_BOUND and np.isfinite(got["quat"]).all(), what
    assert (got["motion"] is None) == (det is None), what
    if det is not None:
        assert got["motion"][0] == det[0], what
        np.testing.assert_array_equal(_bits(got["motion"][1]), _bits(det[1]), err_msg=what + ": field")


def test_fused_ticket(ctx):
    s = sc.stream()
    with _settings(ctx, split=T):
        ctx.reset_frames()
        r0 = ctx.push_frame(s[0], want_entries=True, **_prm(5))
        assert not r0["have_vectors"] and r0["motion"] is None
        r = ctx.push_frame(s[1], want_entries=True, want_field=True, **_prm(6))
    ctx.reset_frames()
    assert r["n_vectors"] > NBLK                              # blocks of the rectangle's rim were split
    got = dict(have=r["have_vectors"], n=r["n_vectors"], entries=r["entries"], quat=r["quat"], motion=r["motion"])
    _check_ticket(ctx, got, s[0], s[1], T, 6, "fused ticket")


def test_fused_async_two_tickets_follow_the_threshold_of_their_push(ctx):
    """four frames, two tickets in flight, the threshold changed between the pushes: T, 0, 4 * T"""
    s = sc.stream()
    ts = (T, T, 0, 4 * T)                                     # the context's threshold when frame k is pushed
    dim = ctx.block_dim(sc.STREAM_DETECTOR["min_size"], sc.STREAM_DETECTOR["subdivide"])
    pins = [ctx.pinned_frame(H, W) for _ in range(4)]
    ents = [ctx.pinned_array((4 * NBLK, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    out, tickets = [], []

    def collect(k):
        r = ctx.frame_wait(tickets[k])
        m = None if r["motion"] is None else (r["motion"][0], flds[k % 2].copy())
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=ents[k % 2][:r["n_vectors"]].copy() if r["have_vectors"] else None,
                        quat=r["quat"], motion=m))

    try:
        ctx.reset_frames()
        for k in range(4):
            if k >= 2:
                collect(k - 2)
            np.copyto(pins[k], s[k])
            ctx.set_sad_split(ts[k])
            tickets.append(ctx.push_frame_async(pins[k], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(10 + k)))
        collect(2)
        collect(3)
    finally:
        ctx.set_sad_split(0)
        ctx.reset_frames()
        for p in pins + ents + flds:
            ctx.free_pinned(p)
    assert not out[0]["have"]
    for k in (1, 2, 3):
        _check_ticket(ctx, out[k], s[k - 1], s[k], ts[k], 10 + k, f"async ticket {k} (T = {ts[k]})")
    assert out[2]["n"] == NBLK and out[1]["n"] > NBLK


def test_batched_forms_ignore_the_threshold(ctx):
    import torch
    s = sc.stream()
    with _settings(ctx):
        plain = [ctx.sad_flow(s[k], s[k + 1], B, R) for k in range(2)]
    ent = ctx.pinned_array((3, NBLK, 4))
    frames = np.ascontiguousarray(s[:3])
    try:
        ctx.set_sad_split(T)
        ctx.reset_frames()
        res = ctx.frames_wait(ctx.push_frames_async(frames, out_entries=ent, **_prm(3)))
        assert [r["n_vectors"] for r in res] == [0, NBLK, NBLK]                        # nblk records per frame, as documented
        for k in range(2):
            np.testing.assert_array_equal(_bits(ent[k + 1]), _bits(plain[k]))
        d = torch.from_numpy(np.array(s[:2])).cuda()
        d_ent = torch.zeros((NBLK, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.sad_flow_dev(d.data_ptr(), 2, W, H, W, W * H, 0, B, R, d_ent.data_ptr())
        ctx.sync()
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()), _bits(plain[0]))
    finally:
        ctx.set_sad_split(0)
        ctx.reset_frames()
        ctx.free_pinned(ent)


def test_plugin_property():
    from ofps_amd.plugins import HipSadDecoder
    s = sc.stream()
    dec = HipSadDecoder(iter([s[0], s[1], s[2]]))
    try:
        names = [p[0] for p in dec.props()]
        assert ("Split blocks", "usize", 0, 0, 4080) in dec.props()
        assert names.index("Scene cut") + 1 == names.index("Split blocks")
        assert dec.set_prop("Block size", B) and dec.set_prop("Search range", R)
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True and len(field) == NBLK
        assert dec.set_prop("Split blocks", T)
        field = []
        assert dec.process_frame(field) is True and dec.ctx.get_sad_split() == T
        best = ipf.full_search(s[1], s[2], B, R)
        want = isp.records(isp.split_step(s[1], s[2], B, best, None, R, T))
        assert len(field) == len(want) > NBLK
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(want))
    finally:
        dec.ctx.close()


def test_cpp_host_writes_the_variable_count_per_frame(tmp_path):
    """ofps_hip_tool extract with "Split blocks" set before frame 2 and cleared before frame 3: the .mvec holds each frame's own count"""
    s = sc.stream()
    raw = tmp_path / "clip.y"
    raw.write_bytes(np.ascontiguousarray(s).tobytes())
    out = tmp_path / "clip.mvec"
    p = subprocess.run([TOOL, "extract", "hip_sad", f"{raw}?w={W}&h={H}&fps=30", str(out), str(len(s)), f"Search range={R}", f"Split blocks={T}@2",
                        "Split blocks=0@3"], check=True, capture_output=True, text=True)
    frames = list(mvec.read_frames(open(out, "rb")))
    assert json.loads(p.stdout)["frames"] == len(s) == len(frames) and len(frames[0]) == 0
    for k, t in ((1, 0), (2, T), (3, 0)):
        best = ipf.full_search(s[k - 1], s[k], B, R)
        want = isp.records(isp.split_step(s[k - 1], s[k], B, best, None, R, t)) if t else ipf.entries(best, B, W, H)
        assert len(frames[k]) == len(want) and (len(want) > NBLK) == bool(t)
        np.testing.assert_array_equal(_bits(frames[k]), _bits(want))
