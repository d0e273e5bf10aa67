"""-m gpu: a batch of two frames IS the one-pair call -- the identity hip_klt's one flow driver (klt.hip: ofps::klt_flow_device) rests on.
ofps_hip_klt_flow_batch[_dev] on two frames against ofps_hip_klt_flow[_dev], and ofps_hip_klt_flow_batch_from[_dev] with a prev_slots against
ofps_hip_klt_flow_from[_dev] with the same one, bit for bit in records, count and raw slots: plain, N3m, N3f, N3m + N3f, intra with cut and
N3f + intra at cells 8 and 16 on the repainted 128 x 96 pair, once with rows padded by 13 bytes, once without d_out_slots, and once at
2048 x 1032, whose 33,024 slots take the large compaction.  tests/test_klt_one_pair_is_a_batch_cpu.py shows from the restatements alone that
no 128 x 96 row can pass on empty or full output; the same bounds are asserted here on what the device returned."""
import numpy as np
import pytest

import klt_one_pair_cases as oc

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_WORD = 0x5A17C0DE


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _settings(ctx, name, cell, min_score=oc.MIN_SCORE, score_radius=2):
    zm, fb, q, cut = oc.SETTINGS[name]
    ctx.set_klt(cell, score_radius, min_score, 1, 0)
    ctx.set_klt_mean_removal(zm); ctx.set_klt_fb(fb); ctx.set_klt_intra(q); ctx.set_klt_cut(cut)


def _defaults(ctx):
    ctx.set_klt()
    ctx.set_klt_mean_removal(0); ctx.set_klt_fb(0); ctx.set_klt_intra(0); ctx.set_klt_cut(0)


def _frames(prev, cur, pad=0):
    """-> view [2, H, W] of a buffer whose rows are W + pad bytes, filler 0xA5"""
    H, W = prev.shape
    buf = np.full((2, H, W + pad), 0xA5, np.uint8)
    buf[0, :, :W] = prev
    buf[1, :, :W] = cur
    return buf[:, :, :W]


class _DevBuf:
    """device memory of `words` 32-bit words with GUARD more behind them"""

    def __init__(self, ctx, words, init=None):
        self.ctx, self.words = ctx, int(words)
        self.ptr = ctx.malloc(4 * (self.words + GUARD))
        host = np.full(self.words + GUARD, GUARD_WORD, np.uint32)
        if init is not None:
            host[:self.words] = np.ascontiguousarray(init).view(np.uint32).ravel()
        ctx.memcpy_h2d(self.ptr, host)

    def read(self, dtype):
        host = np.zeros(self.words + GUARD, np.uint32)
        self.ctx.memcpy_d2h(host, self.ptr)
        assert (host[self.words:] == GUARD_WORD).all(), "guard words behind a device buffer were overwritten"
        return host[:self.words].view(dtype)

    def free(self):
        self.ctx.free(self.ptr)


def _host_forms(ctx, view, prev_slots, want_slots, L=oc.LEVELS, w=oc.RADIUS, K=oc.ITERS):
    """-> [(records[:count], count, slots or None)] of the one-pair call and of the batch call on the two frames"""
    stride = view.strides[1]
    if prev_slots is None:
        one = ctx.klt_flow(view[0], view[1], L, w, K, want_slots=want_slots, stride=stride)
        bat = ctx.klt_flow_batch(view, L, w, K, 0, want_slots=want_slots)
    else:
        one = ctx.klt_flow_from(view[0], view[1], L, w, K, prev_slots, want_slots=want_slots, stride=stride)
        bat = ctx.klt_flow_batch_from(view, L, w, K, 0, prev_slots, want_slots=want_slots)
    ent, slots = one if want_slots else (one, None)
    count = int(bat[1][0])
    return [(ent, len(ent), slots), (bat[0][0, :count], count, bat[2][0] if want_slots else None)]


def _dev_forms(ctx, view, prev_slots, want_slots, L=oc.LEVELS, w=oc.RADIUS, K=oc.ITERS):
    """the same through the device-pointer forms, every output between guard words"""
    _, H, W = view.shape
    buf = view.base if view.base is not None else view
    stride, pitch = buf.shape[2], buf.shape[1] * buf.shape[2]
    ns = ctx.klt_slot_count(W, H)
    d = ctx.malloc(buf.size)
    ctx.memcpy_h2d(d, buf)
    b_prev = _DevBuf(ctx, 6 * ns, prev_slots) if prev_slots is not None else None
    out = []
    try:
        for batch in (False, True):
            b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns)
            d_slots = b_slots.ptr if want_slots else None
            if batch and b_prev:
                ctx.klt_flow_batch_from_dev(d, 2, W, H, stride, pitch, 0, L, w, K, b_rec.ptr, b_cnt.ptr, d_slots, b_prev.ptr)
            elif batch:
                ctx.klt_flow_batch_dev(d, 2, W, H, stride, pitch, 0, L, w, K, b_rec.ptr, b_cnt.ptr, d_slots)
            elif b_prev:
                ctx.klt_flow_from_dev(d, d + pitch, W, H, stride, L, w, K, b_prev.ptr, b_rec.ptr, b_cnt.ptr, d_slots)
            else:
                ctx.klt_flow_dev(d, d + pitch, W, H, stride, L, w, K, b_rec.ptr, b_cnt.ptr, d_slots)
            ctx.sync()
            count = int(b_cnt.read(np.uint32)[0])
            assert count <= ns
            slots = b_slots.read(np.int32).reshape(ns, 6).copy()
            if not want_slots:
                assert (slots.view(np.uint32) == GUARD_WORD).all(), "raw slots were written though nobody asked for them"
            out.append((b_rec.read(np.float32).reshape(ns, 4)[:count].copy(), count, slots if want_slots else None))
            for b in (b_rec, b_cnt, b_slots):
                b.free()
            if b_prev:
                assert (b_prev.read(np.int32).reshape(ns, 6) == prev_slots).all(), "the previous pair's slots were written"
    finally:
        if b_prev:
            b_prev.free()
        ctx.free(d)
    return out


def _same(one, bat, what):
    assert one[1] == bat[1], f"{what}: the one-pair call kept {one[1]}, the batch of two frames {bat[1]}"
    assert (_bits(one[0]) == _bits(bat[0])).all(), f"{what}: records differ"
    if one[2] is not None:
        assert (one[2] == bat[2]).all(), f"{what}: raw slots differ"


def _row(ctx, name, cell, pad=0, want_slots=True):
    """both forms, host and device pointers, from zero and from a prev_slots -> the device's tallies [(kept, status 5, status 6)]"""
    prev, cur = oc.pair()
    view = _frames(prev, cur, pad)
    tallies = []
    try:
        _settings(ctx, name, cell)
        ns = ctx.klt_slot_count(oc.W, oc.H)
        # what the `_from` rows start from: this pair's own answer under the same settings, the one-pair call's
        _, prev_slots = ctx.klt_flow(prev, cur, oc.LEVELS, oc.RADIUS, oc.ITERS, want_slots=True)
        for start in (None, prev_slots):
            for forms in (_host_forms, _dev_forms):
                one, bat = forms(ctx, view, start, want_slots)
                what = f"{name} cell {cell} pad {pad} {'from slots' if start is not None else 'from zero'} {forms.__name__}"
                _same(one, bat, what)
                assert 0 < one[1] < ns, f"{what}: {one[1]} of {ns} slots kept"
                if want_slots:
                    tally = oc.tally(one[2])
                    assert tally[0] == one[1] and oc.bounds_hold(name, cell, tally, ns), f"{what}: (kept, status 5, status 6) = {tally}"
                    tallies.append(tally)
    finally:
        _defaults(ctx)
    return tallies


@pytest.mark.parametrize("name,cell", oc.ROWS)
def test_two_frames_through_the_batch_forms_equal_the_one_pair_forms(ctx, name, cell):
    _row(ctx, name, cell)


def test_with_rows_padded_by_13_bytes(ctx):
    _row(ctx, *oc.PADDED_ROW, pad=oc.PAD)


def test_without_raw_slots(ctx):
    """No slots come back, so no status can be tallied: this row asserts 0 < kept < slots alone, and its setting's status bound (at least
    one status 5) is carried by the parametrised row of the same setting, which runs with slots."""
    _row(ctx, *oc.NO_SLOTS_ROW, want_slots=False)


def test_a_pair_above_the_small_compaction_through_the_batch_entry(ctx):
    from ofps_amd import synth
    big = oc.LARGE
    fr = synth.luma_sequence(2, big["W"], big["H"], big["seed"])
    try:
        _settings(ctx, "plain", big["cell"], min_score=1, score_radius=1)
        assert ctx.klt_slot_count(big["W"], big["H"]) == big["slots"]
        one, bat = _dev_forms(ctx, _frames(fr[0], fr[1]), None, True, big["levels"], big["radius"], big["iters"])
        assert one[1] > big["kept_above"] and bat[1] > big["kept_above"], (one[1], bat[1])
        _same(one, bat, "2048 x 1032")
    finally:
        _defaults(ctx)
