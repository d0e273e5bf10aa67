"""hip_klt's chained batch (include/ofps_hip.h N3pb) on the GPU, bit for bit against the restatement tests/indep_klt_batch_pred.py: the stage
form ofps_hip_klt_flow_batch_from[_dev], the switch in the batch form, the batched stream whose answers do not depend on how the frames are cut
into tickets, what makes the stream forget, the option, the refusals, the tool's flag and the multi-device workers, which ignore it all."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import indep_klt_batch_pred as ib
import indep_klt_pred as ip
import klt_batch_pred_cases as bc
import klt_pred_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6                                            # N3b's bound on the quaternion
GUARD = 64
GUARD_WORD = 0x5A17C0DE
CAM = (16 / 9, 39.6 * 9 / 16)
SEED = 77
VARIANTS = [(False, 0), (True, 0), (False, 64), (True, 64)]  # (mean removal, F)
VARIANT_IDS = ["plain", "zm", "F64", "zm-F64"]
W, H = bc.W, bc.H
TAIL = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=CAM[0], fov_y_deg=CAM[1], use_ransac=False)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    assert c.get_klt_prediction() == 0 and c.get_klt_batch_prediction() == 0 and c.get_klt_fb() == 0 and c.get_klt_mean_removal() == 0
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
    ctx.set_klt(); ctx.set_klt_fb(0); ctx.set_klt_mean_removal(0); ctx.set_klt_prediction(0); ctx.set_klt_batch_prediction(0)
    ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)


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


def _padded_stack(frames, pad):
    """-> a [n, H, W] view of a buffer whose rows are W + pad bytes, the padding 0xA5"""
    buf = np.full((len(frames), H, W + pad), 0xA5, np.uint8)
    buf[:, :, :W] = np.stack(frames)
    return buf[:, :, :W]


def _check_items(rec, counts, slots, want, what):
    assert len(counts) == len(want), what
    for k, w in enumerate(want):
        assert int(counts[k]) == w["count"], f"{what}: item {k} count {int(counts[k])} != {w['count']}"
        np.testing.assert_array_equal(_bits(rec[k][:w["count"]]), _bits(w["records"]), err_msg=f"{what}: item {k} record bits")
        if slots is not None:
            np.testing.assert_array_equal(slots[k], w["slots"], err_msg=f"{what}: item {k} slots")


def _batch_from_dev(ctx, frames, ref_mode, L, w, K, prev_slots, want_slots, pad=0, plain_entry=False):
    """the _dev form on a padded device copy of the frames, every output with guard words -> (records [pairs, ns, 4], counts, slots | None)"""
    view = _padded_stack(frames, pad)
    stride, pitch = W + pad, (W + pad) * H
    ns, pairs = ctx.klt_slot_count(W, H), len(frames) - 1
    d_fr = ctx.malloc(view.base.size)
    ctx.memcpy_h2d(d_fr, view.base)
    b_rec, b_cnt = _DevBuf(ctx, 4 * ns * pairs), _DevBuf(ctx, pairs)
    b_slots = _DevBuf(ctx, 6 * ns * pairs) if want_slots else None
    b_prev = _DevBuf(ctx, 6 * ns, prev_slots) if prev_slots is not None else None
    try:
        if plain_entry:
            assert prev_slots is None
            ctx.klt_flow_batch_dev(d_fr, len(frames), W, H, stride, pitch, ref_mode, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr if b_slots else None)
        else:
            ctx.klt_flow_batch_from_dev(d_fr, len(frames), W, H, stride, pitch, ref_mode, L, w, K, b_rec.ptr, b_cnt.ptr,
                                        b_slots.ptr if b_slots else None, b_prev.ptr if b_prev else None)
        ctx.sync()
        if b_prev:
            np.testing.assert_array_equal(b_prev.read(np.int32).reshape(-1, 6), prev_slots)       # read, not written
        return (b_rec.read(np.float32).reshape(pairs, ns, 4), b_cnt.read(np.uint32).copy(),
                b_slots.read(np.int32).reshape(pairs, ns, 6).copy() if b_slots else None)
    finally:
        for b in (b_rec, b_cnt, b_slots, b_prev):
            if b:
                b.free()
        ctx.free(d_fr)


# ------------------------------------------------------------------------------------------------ 1: the stage form
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("params", [bc.RAMP_SET, bc.DEFAULT_SET], ids=["L2w4", "defaults"])
@pytest.mark.parametrize("name", list(bc.SEQUENCES))
def test_batch_from_matches_the_restatement(ctx, name, params, variant):
    zm, F = variant
    ref_mode = bc.SEQUENCES[name]
    want = bc.expect(name, params, True, F, zm)
    plain = bc.expect(name, params, False, F, zm)
    assert any(a["slots"].tobytes() != b["slots"].tobytes() for a, b in zip(want, plain))        # the unchained answer is another one
    L, w, K = _set(ctx, params, F, zm)
    try:
        fr = np.stack(bc.frames(name))
        # from zero, the whole sequence: host form with slots, _dev form without
        rec, counts, slots = ctx.klt_flow_batch_from(fr, L, w, K, ref_mode)
        _check_items(rec, counts, slots, want, "host, NULL")
        rec, counts, _ = _batch_from_dev(ctx, bc.frames(name), ref_mode, L, w, K, None, want_slots=False)
        _check_items(rec, counts, None, want, "_dev, NULL, no slots")
        # from the slots of the item before: the sequence without its first two items; host form without slots, _dev form with
        tail, prev = bc.tail_frames(name, 2), want[1]["slots"]
        rec, counts = ctx.klt_flow_batch_from(np.stack(tail), L, w, K, ref_mode, prev, want_slots=False)
        _check_items(rec, counts, None, want[2:], "host, prev_slots, no slots")
        rec, counts, slots = _batch_from_dev(ctx, tail, ref_mode, L, w, K, prev, want_slots=True)
        _check_items(rec, counts, slots, want[2:], "_dev, prev_slots")
        # a batch of one pair: nothing to read but prev_slots, nothing to write but the one item
        one, prev = bc.tail_frames(name, 4)[:2], want[3]["slots"]
        for want_slots in (True, False):
            rec, counts, slots = _batch_from_dev(ctx, one, ref_mode, L, w, K, prev, want_slots)
            _check_items(rec, counts, slots, want[4:5], f"_dev, one pair, slots {want_slots}")
        rec, counts, slots = ctx.klt_flow_batch_from(np.stack(one), L, w, K, ref_mode, prev)
        _check_items(rec, counts, slots, want[4:5], "host, one pair")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("variant", [(False, 0), (True, 64)], ids=["plain", "zm-F64"])
@pytest.mark.parametrize("pad", [12, 13])
def test_batch_from_on_padded_rows(ctx, pad, variant):
    zm, F = variant
    L, w, K = _set(ctx, bc.RAMP_SET, F, zm)
    try:
        for name in ("ramp3", "const4"):
            want = bc.expect(name, bc.RAMP_SET, True, F, zm)
            view = _padded_stack(bc.frames(name), pad)
            assert view.strides == ((W + pad) * H, W + pad, 1)
            rec, counts, slots = ctx.klt_flow_batch_from(view, L, w, K, bc.SEQUENCES[name])
            _check_items(rec, counts, slots, want, f"host, {name}")
            rec, counts, slots = _batch_from_dev(ctx, bc.tail_frames(name, 1), bc.SEQUENCES[name], L, w, K, want[0]["slots"], True, pad=pad)
            _check_items(rec, counts, slots, want[1:], f"_dev, {name}")
    finally:
        _reset(ctx)


def test_batch_from_host_form_leaves_the_words_behind_its_outputs_alone_and_dev_form_refuses_overlapping_slots(ctx):
    want = bc.expect("const4", bc.RAMP_SET, True, 64)
    L, w, K = _set(ctx, bc.RAMP_SET, 64)
    try:
        ns = ctx.klt_slot_count(W, H)
        u8, i32, f32, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        fr = np.ascontiguousarray(np.stack(bc.tail_frames("const4", 1)))
        pairs = len(fr) - 1
        ent = np.full(4 * ns * pairs + GUARD, GUARD_WORD, np.uint32)
        slots = np.full(6 * ns * pairs + GUARD, GUARD_WORD, np.uint32)
        cnt = np.full(pairs + GUARD, GUARD_WORD, np.uint32)
        # the host form copies prev_slots first: it may lie inside out_slots
        slots[:6 * ns] = want[0]["slots"].view(np.uint32).ravel()
        assert ctx._lib.ofps_hip_klt_flow_batch_from(ctx._h, fr.ctypes.data_as(u8), len(fr), W, H, W, W * H, 1, L, w, K, ent.ctypes.data_as(f32),
                                                     cnt.ctypes.data_as(u32), slots.ctypes.data_as(i32), slots.ctypes.data_as(i32)) == 0
        for a, words in ((ent, 4 * ns * pairs), (slots, 6 * ns * pairs), (cnt, pairs)):
            assert (a[words:] == GUARD_WORD).all()
        rec = ent[:4 * ns * pairs].view(np.float32).reshape(pairs, ns, 4)
        _check_items(rec, cnt[:pairs], slots[:6 * ns * pairs].view(np.int32).reshape(pairs, ns, 6), want[1:], "host, prev_slots inside out_slots")
        for k, wk in enumerate(want[1:]):                       # the rows behind an item's kept records are not written
            assert (ent[:4 * ns * pairs].reshape(pairs, ns * 4)[k, 4 * wk["count"]:] == GUARD_WORD).all(), k
        # the _dev form refuses arrays that share a byte, before anything is enqueued
        buf = _DevBuf(ctx, 6 * ns * (pairs + 2), np.tile(want[0]["slots"], (pairs + 2, 1)))
        b_rec, b_cnt = _DevBuf(ctx, 4 * ns * pairs), _DevBuf(ctx, pairs)
        d_fr = ctx.malloc(fr.size)
        ctx.memcpy_h2d(d_fr, fr)
        try:
            last = 24 * ns * pairs                              # the byte behind out_slots at offset 0
            for off_prev, off_out in ((0, 0), (0, 4), (last - 4, 0), (24 * ns, 0), (24 * ns * (pairs - 1), 0), (24 * ns, 24 * ns * 2 - 4)):
                with pytest.raises(OfpsHipError) as e:
                    ctx.klt_flow_batch_from_dev(d_fr, len(fr), W, H, W, W * H, 1, L, w, K, b_rec.ptr, b_cnt.ptr, buf.ptr + off_out, buf.ptr + off_prev)
                assert e.value.code == EINVAL, (off_prev, off_out)
            for off_prev, off_out in ((last, 0), (0, 24 * ns)):  # side by side, behind and in front
                ctx.klt_flow_batch_from_dev(d_fr, len(fr), W, H, W, W * H, 1, L, w, K, b_rec.ptr, b_cnt.ptr, buf.ptr + off_out, buf.ptr + off_prev)
                ctx.sync()
                got = buf.read(np.int32).reshape(pairs + 2, ns, 6)
                first = off_out // (24 * ns)
                _check_items(b_rec.read(np.float32).reshape(pairs, ns, 4), b_cnt.read(np.uint32), got[first:first + pairs], want[1:], "side by side")
                ctx.memcpy_h2d(buf.ptr, np.concatenate([np.tile(want[0]["slots"], (pairs + 2, 1)).view(np.uint32).ravel(),
                                                        np.full(GUARD, GUARD_WORD, np.uint32)]))
        finally:
            for b in (buf, b_rec, b_cnt):
                b.free()
            ctx.free(d_fr)
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ 2: the switch in the batch form
def test_flow_batch_chains_with_both_settings_on_and_only_then(ctx):
    L, w, K = _set(ctx, bc.RAMP_SET)
    try:
        for name in ("ramp3", "const4"):
            ref_mode = bc.SEQUENCES[name]
            fr = np.stack(bc.frames(name))
            on, off = bc.expect(name, bc.RAMP_SET, True), bc.expect(name, bc.RAMP_SET, False)
            if name == "ramp3":
                assert all(a["slots"].tobytes() == b["slots"].tobytes() for a, b in zip(off, pc.ramp_expect("ramp3", pc.RAMP_SET, False)))
            for pred, bpred in ((0, 0), (1, 0), (0, 1), (1, 1)):
                ctx.set_klt_prediction(pred); ctx.set_klt_batch_prediction(bpred)
                want = on if pred and bpred else off
                rec, counts, slots = ctx.klt_flow_batch(fr, L, w, K, ref_mode=ref_mode, want_slots=True)
                _check_items(rec, counts, slots, want, f"{name} host {pred} {bpred}")
                rec, counts, slots = _batch_from_dev(ctx, bc.frames(name), ref_mode, L, w, K, None, True, plain_entry=True)
                _check_items(rec, counts, slots, want, f"{name} _dev {pred} {bpred}")
                # ... and _batch_from reads neither setting
                rec, counts, slots = ctx.klt_flow_batch_from(fr[:4], L, w, K, ref_mode)
                _check_items(rec, counts, slots, on[:3], f"{name} _batch_from {pred} {bpred}")
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ 3: the batched stream
def _stream(c, frames, sizes, before_push=None, seed0=SEED):
    """the frames through push_frames_async in tickets of `sizes`, every ticket but the first pushed before the one in front of it is collected
    -> per frame dict(have_vectors, n_vectors, motion, quat, entries).  before_push(i): called in front of ticket i's push"""
    out, start, pending = [], 0, []

    def collect():
        t, ent, first = pending.pop(0)
        for j, r in enumerate(c.frames_wait(t)):
            out.append(dict(r, entries=ent[j][:r["n_vectors"]].copy(), frame=first + j))

    for i, size in enumerate(sizes):
        if before_push:
            before_push(i)
        batch = np.ascontiguousarray(frames[start:start + size])
        ent = np.zeros((size, c.batch_record_capacity(batch.shape[2], batch.shape[1]), 4), np.float32)
        pending.append((c.push_frames_async(batch, seed=seed0 + start, out_entries=ent, **TAIL), ent, start))
        if len(pending) == 2:
            collect()
        start += size
    while pending:
        collect()
    return out


def _check_stream(got, want, what, first=0):
    """got[first] is a stream's first frame, got[first + 1 + k] item k of want"""
    assert not got[first]["have_vectors"] and got[first]["n_vectors"] == 0, what
    for k, w in enumerate(want):
        g = got[first + 1 + k]
        assert g["have_vectors"] and g["n_vectors"] == w["count"], f"{what}: pair {k} count {g['n_vectors']} != {w['count']}"
        np.testing.assert_array_equal(_bits(g["entries"]), _bits(w["records"]), err_msg=f"{what}: pair {k} record bits")


CUTS = [(7,), (4, 3), (1, 1, 1, 1, 1, 1, 1), (2, 5)]


@pytest.mark.parametrize("fb_limit", [0, 64])
def test_stream_answers_do_not_depend_on_the_cut(ctx, fb_limit):
    fr = np.stack(pc.ramp_frames("ramp3"))
    assert len(fr) == 7
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True, fb_limit)
    plain = pc.ramp_expect("ramp3", pc.RAMP_SET, False, fb_limit)
    assert any(a["records"].tobytes() != b["records"].tobytes() for a, b in zip(want, plain))
    L, w, K = _set(ctx, pc.RAMP_SET, fb_limit)
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
    ctx.set_klt_prediction(1); ctx.set_klt_batch_prediction(1)
    try:
        runs = {}
        for cut in CUTS:
            ctx.reset_frames()
            runs[cut] = _stream(ctx, fr, cut)
            _check_stream(runs[cut], want, f"cut {cut}")
        ref = runs[CUTS[2]]
        for cut in CUTS:
            for j, (g, r) in enumerate(zip(runs[cut], ref)):
                assert g["motion"] == r["motion"], (cut, j)
                print("cut", cut, "frame", j, "quaternion difference", float(np.abs(g["quat"] - r["quat"]).max()))
                assert np.abs(g["quat"] - r["quat"]).max() <= QUAT_BOUND, (cut, j)
        assert any(np.abs(r["quat"] - (1, 0, 0, 0)).max() > 1e-4 for r in ref)        # the estimator ran on something
        # either setting off: the parent's answer, whatever the cut
        for pred, bpred in ((1, 0), (0, 1)):
            ctx.set_klt_prediction(pred); ctx.set_klt_batch_prediction(bpred)
            ctx.reset_frames()
            _check_stream(_stream(ctx, fr, (4, 3)), plain, f"settings {pred} {bpred}")
    finally:
        ctx.reset_frames(); _reset(ctx)


def _chain(frames, prev_slots=None, fb_limit=0):
    cell, r, ms, e, R, L, w, K = pc.RAMP_SET
    return ib.flow_batch_from(frames, L, w, K, 0, prev_slots, cell=cell, r=r, min_score=ms, min_eig=e, max_residual=R, fb_limit=fb_limit)


def test_what_makes_the_stream_forget(ctx):
    fr = np.stack(pc.ramp_frames("ramp3"))
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True)
    plain = pc.ramp_expect("ramp3", pc.RAMP_SET, False)
    from_3 = _chain(fr[3:])                                    # the pairs (3, 4), (4, 5), (5, 6), the first from zero
    assert from_3[0]["slots"].tobytes() == plain[3]["slots"].tobytes() != want[3]["slots"].tobytes()
    assert from_3[1]["slots"].tobytes() not in (plain[4]["slots"].tobytes(), want[4]["slots"].tobytes())
    L, w, K = _set(ctx, pc.RAMP_SET)
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
    ctx.set_klt_prediction(1); ctx.set_klt_batch_prediction(1)
    try:
        # ofps_hip_reset_frames in mid-stream: the stream that follows starts from zero
        ctx.reset_frames()
        _check_stream(_stream(ctx, fr[:4], (2, 2)), want[:3], "before the reset")
        ctx.reset_frames()
        _check_stream(_stream(ctx, fr[3:], (2, 2), seed0=SEED + 3), from_3, "after the reset")

        # a ticket pushed with klt_prediction 0, with the switch 0, or with the search as decoder, in the middle: it leaves no slots
        def middle(what):
            def hook(i):
                ctx.set_klt_prediction(0 if (what == "prediction" and i == 1) else 1)
                ctx.set_klt_batch_prediction(0 if (what == "switch" and i == 1) else 1)
                if what == "sad" and i == 1:
                    ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)
                else:
                    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
            return hook
        for what in ("prediction", "switch", "sad"):
            ctx.reset_frames()
            got = _stream(ctx, fr, (2, 2, 3), middle(what))
            _check_stream(got[:2], want[:1], what + ": the first ticket")
            if what != "sad":                                  # frames 2 and 3: pairs (1, 2) and (2, 3), unchained
                for k in (1, 2):
                    np.testing.assert_array_equal(_bits(got[k + 1]["entries"]), _bits(plain[k]["records"]), err_msg=f"{what}: pair {k}")
            for k, wk in enumerate(from_3):                    # frames 4, 5, 6: chained again, from zero
                assert got[4 + k]["n_vectors"] == wk["count"], (what, k)
                np.testing.assert_array_equal(_bits(got[4 + k]["entries"]), _bits(wk["records"]), err_msg=f"{what}: pair {3 + k}")

        # a geometry change restarts the stream, the slots of the other lattice are not read; and back again
        ctx.set_klt_prediction(1); ctx.set_klt_batch_prediction(1); ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
        narrow = np.ascontiguousarray(fr[:, :, :144])
        ctx.reset_frames()
        got = _stream(ctx, fr[:3], (3,)) + _stream(ctx, narrow[2:6], (2, 2), seed0=SEED + 2) + _stream(ctx, fr[3:], (1, 3), seed0=SEED + 3)
        _check_stream(got, want[:2], "before the change")
        _check_stream(got, _chain(narrow[2:6]), "the narrow frames", first=3)
        _check_stream(got, from_3, "the first geometry again", first=7)
    finally:
        ctx.reset_frames(); _reset(ctx)


# ------------------------------------------------------------------------------------------------ 4: option, environment, refusals
def test_the_option_and_the_environment_variable_set_what_the_getter_reads(ctx):
    try:
        assert ctx.get_klt_batch_prediction() == 0
        ctx.set_option("OFPS_HIP_KLT_BATCH_PREDICTION", 1)
        assert ctx.get_klt_batch_prediction() == 1 and ctx.get_klt_prediction() == 0
        ctx.set_option("OFPS_HIP_KLT_BATCH_PREDICTION", 0)
        assert ctx.get_klt_batch_prediction() == 0
        ctx.set_klt_batch_prediction(1)
        ctx.set_option("OFPS_HIP_KLT_BATCH_PREDICTION", None)
        assert ctx.get_klt_batch_prediction() == 0              # the default
    finally:
        _reset(ctx)
    code = ("import sys; sys.path.insert(0, %r); from ofps_amd.runtime import HipContext; c = HipContext(0); "
            "print(c.get_klt_batch_prediction(), c.get_klt_prediction()); c.close()" % ROOT)
    env = dict(os.environ, OFPS_HIP_KLT_BATCH_PREDICTION="1")
    env.pop("OFPS_HIP_KLT_PREDICTION", None)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1].split() == ["1", "0"]


def test_refusals(ctx):
    fr = np.ascontiguousarray(np.stack(pc.ramp_frames("ramp3")[:4]))
    want = pc.ramp_expect("ramp3", pc.RAMP_SET, True)
    L, w, K = _set(ctx, pc.RAMP_SET)
    ctx.set_klt_prediction(1); ctx.set_klt_batch_prediction(1)

    def valid_call():
        assert ctx.get_klt_batch_prediction() == 1             # the setting stays as it was
        rec, counts, slots = ctx.klt_flow_batch(fr, L, w, K, want_slots=True)
        _check_items(rec, counts, slots, want[:3], "after a refusal")

    try:
        for bad in (-1, 2, 2 ** 31 - 1, -(2 ** 31)):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_klt_batch_prediction(bad)
            assert e.value.code == EINVAL, bad
        valid_call()
        for bad in ("yes", "-1", "2", "1x", " 1"):
            with pytest.raises(OfpsHipError) as e:
                ctx.set_option("OFPS_HIP_KLT_BATCH_PREDICTION", bad)
            assert e.value.code == EINVAL, bad
        valid_call()
        assert ctx._lib.ofps_hip_set_klt_batch_prediction(None, 1) == EINVAL and ctx._lib.ofps_hip_get_klt_batch_prediction(None) == EINVAL
        # everything _flow_batch refuses, refused before anything is read: the pointers are not device memory
        ns = ctx.klt_slot_count(W, H)
        good = dict(n_frames=4, W=W, H=H, stride=W, frame_pitch=W * H, ref_mode=0, levels=L, radius=w, iters=K)
        for change in (dict(n_frames=1), dict(n_frames=0), dict(ref_mode=2), dict(ref_mode=-1), dict(frame_pitch=W * H - 1), dict(stride=W - 1),
                       dict(levels=0), dict(levels=7), dict(radius=0), dict(radius=8), dict(iters=0), dict(iters=31), dict(W=4), dict(levels=5)):
            a = dict(good, **change)
            with pytest.raises(OfpsHipError) as e:
                ctx.klt_flow_batch_from_dev(4096, a["n_frames"], a["W"], a["H"], a["stride"], a["frame_pitch"], a["ref_mode"], a["levels"], a["radius"],
                                            a["iters"], 4096, 4096, 4096 + 4096, 4096 + 4096 + 24 * ns * 3)
            assert e.value.code == EINVAL, change
        with pytest.raises(OfpsHipError) as e:
            ctx.klt_flow_batch_from_dev(0, 4, W, H, W, W * H, 0, L, w, K, 4096, 4096, None, None)
        assert e.value.code == EINVAL
        u8, i32, f32, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        ent, cnt = np.zeros((3, ns, 4), np.float32), np.zeros(3, np.uint32)
        assert ctx._lib.ofps_hip_klt_flow_batch_from(None, fr.ctypes.data_as(u8), 4, W, H, W, W * H, 0, L, w, K, ent.ctypes.data_as(f32),
                                                     cnt.ctypes.data_as(u32), None, None) == EINVAL
        assert ctx._lib.ofps_hip_klt_flow_batch_from(ctx._h, fr.ctypes.data_as(u8), 4, W, H, W, W * H, 2, L, w, K, ent.ctypes.data_as(f32),
                                                     cnt.ctypes.data_as(u32), None, None) == EINVAL
        assert ctx._lib.ofps_hip_klt_flow_batch_from(ctx._h, None, 4, W, H, W, W * H, 0, L, w, K, ent.ctypes.data_as(f32),
                                                     cnt.ctypes.data_as(u32), None, None) == EINVAL
        valid_call()
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ 5: the tool and the multi-device workers
def test_stream_bench_reports_both_settings():
    tool = os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool")
    runs = [json.loads(subprocess.run([tool, "stream-bench", "128", "96", "12", "batch", "3", "--klt"] + extra, check=True, capture_output=True,
                                      text=True, timeout=120).stdout.strip().splitlines()[-1])
            for extra in (["--klt-predict"], ["--klt-predict", "--klt-batch-predict"], ["--klt-batch-predict"])]
    assert [(r["prediction"], r["batch_prediction"]) for r in runs] == [(1, 0), (1, 1), (0, 1)] and runs[0]["decoder"] == "hip_klt"
    print("last_n_vectors", [r["last_n_vectors"] for r in runs])
    assert runs[0]["last_n_vectors"] == runs[2]["last_n_vectors"]     # either flag alone changes nothing
    p = subprocess.run([tool, "stream-bench", "128", "96", "12", "batch", "3", "--klt-batch-predict"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--klt" in p.stderr


def test_multi_device_workers_ignore_both_settings():
    cell, r, min_score, min_eig, R, L, w, K = pc.RAMP_SET
    env = dict(os.environ, OFPS_HIP_BATCH_DECODER="1", OFPS_HIP_KLT_CELL=str(cell), OFPS_HIP_KLT_SCORE_RADIUS=str(r), OFPS_HIP_KLT_MIN_SCORE=str(min_score),
               OFPS_HIP_KLT_MIN_EIG=str(min_eig), OFPS_HIP_KLT_MAX_RESIDUAL=str(R), OFPS_HIP_KLT_LEVELS=str(L), OFPS_HIP_KLT_RADIUS=str(w),
               OFPS_HIP_KLT_ITERS=str(K), KLT_CHILD_SEED=str(SEED))
    for name in ("OFPS_HIP_KLT_MEAN_REMOVAL", "OFPS_HIP_KLT_FB", "OFPS_HIP_KLT_PREDICTION", "OFPS_HIP_KLT_BATCH_PREDICTION"):
        env.pop(name, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_klt_batch_pred_child.py")], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["capacity"] == 60
    assert child["settings_seen"] == {"both": [1, 1], "neither": [0, 0]}       # what a context made in that environment reads
    both, neither = child["both"], child["neither"]
    assert both == neither
    plain = pc.ramp_expect("ramp3", pc.RAMP_SET, False)
    assert [g["have_vectors"] for g in both] == [False] + [True] * 6
    for k, wk in enumerate(plain):
        assert both[k + 1]["n_vectors"] == wk["count"], k
        assert both[k + 1]["entries"] == _bits(wk["records"]).reshape(-1).tolist(), k
