"""-m gpu: a refused push leaves its stream where it was, and a batch buffer that grows under a live ticket keeps the stream's newest frame.

Every form of ofps_hip_push_frame_async and ofps_hip_push_frames_async is run once with two tickets in flight and nothing refused, then again
with refused calls between the accepted ones: a third push with two tickets uncollected, a bad argument (stride < W), and a setting the frame
has no room for -- for hip_klt levels 5 on 128 x 96 (96 >> 4 = 6 < 8), for the filtered hip_sad forms a contrast gate of 257 pixels, one more
than a 16 x 16 block holds (sad_gate.hip: sad_gate_check, asked by SadFilter::plan; the setter takes any value >= 0).  Both runs enqueue the
same launches, so every frame's have_vectors, n_vectors, island, quaternion bytes and record bits must be equal.  The batched forms are cut
1 + 2 + 3, so the batch buffers grow twice and the second time with a ticket in flight (the previous frame is parked); the filtered hip_sad form
and the chained hip_klt form are also compared with the same cut collected one ticket at a time.

Frames: the six 128 x 96 frames of klt_batch_cases.SMALL at SMALL_SETS[1] (cell 8: 192 slots; the restatement keeps 177 / 76 / 162 / 87 / 75) for
hip_klt; the four 320 x 192 frames of sad_gate_cases for hip_sad (240 blocks, of which the gate alone drops the flat right-hand side: at most
13 of the 20 block columns pass; tests/test_sad_batch_filter_cpu.py pins kept counts strictly between 0 and 240 for these frames), for the
batched forms followed by frames 2 and 1 again to make six.  No compared item is trivially equal: every
item with vectors of a filtered or hip_klt form has 0 < n_vectors < capacity, asserted on what the device returned; the plain hip_sad forms
always return one record per block, and their records are asserted not to be all alike."""
import ctypes as C

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import klt_batch_cases as bc
import sad_gate_cases as gc

pytestmark = pytest.mark.gpu

EINVAL = -1
CUT = (1, 2, 3)
KLT_SET = bc.SMALL_SETS[1]
CRITERIA = dict(gate=1, limit=1, median=2)
BAD_GATE = gc.BLOCK * gc.BLOCK + 1
SAD_PRM = dict(block=gc.BLOCK, search_range=gc.RANGE, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1], **gc.FRAME_DETECTOR)
KLT_PRM = dict(min_size=0.05, subdivide=2)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _sad_frames(n):
    f = gc.frames()
    return np.ascontiguousarray(f[[0, 1, 2, 3, 2, 1][:n]])


class Form:
    """one form of a stream: its frames, its settings, what it may be refused for"""

    def __init__(self, name, batched, klt=False, filtered=False, chained=False):
        self.name, self.batched, self.klt, self.filtered, self.chained = name, batched, klt, filtered, chained
        self.frames = np.ascontiguousarray(bc.sequence(bc.SMALL)) if klt else _sad_frames(6 if batched else 4)
        self.prm = KLT_PRM if klt else SAD_PRM
        self.seed = 77 if klt else gc.SEED

    def apply(self, ctx):
        ctx.reset_frames()
        crit = CRITERIA if self.filtered else dict(gate=0, limit=0, median=0)
        ctx.set_sad_gate(crit["gate"]); ctx.set_sad_consistency(crit["limit"]); ctx.set_sad_median(crit["median"])
        ctx.set_sad_batch_filter(int(self.filtered and self.batched))
        if self.klt:
            cell, r, min_score, min_eig, R, L, w, K = KLT_SET
            ctx.set_klt(cell, r, min_score, min_eig, R)
            ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
            ctx.set_klt_prediction(int(self.chained)); ctx.set_klt_batch_prediction(int(self.chained))

    def restore(self, ctx):
        ctx.reset_frames()
        ctx.set_sad_gate(0); ctx.set_sad_consistency(0); ctx.set_sad_median(0); ctx.set_sad_batch_filter(0)
        ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)
        ctx.set_klt(); ctx.set_klt_prediction(0); ctx.set_klt_batch_prediction(0)

    def capacity(self, ctx):
        H, W = self.frames.shape[1:]
        return ctx.klt_slot_count(W, H, KLT_SET[0]) if self.klt else gc.NBLK

    # ---- pushes and waits: (ticket, entries, frames kept alive) and the per-frame tuples that are compared
    def push(self, ctx, start, size):
        ent = np.zeros((size, self.capacity(ctx), 4), np.float32)
        if self.batched:
            batch = np.ascontiguousarray(self.frames[start:start + size])
            return ctx.push_frames_async(batch, seed=self.seed + start, out_entries=ent, **self.prm), ent, batch
        return ctx.push_frame_async(self.frames[start], seed=self.seed + start, out_entries=ent[0], **self.prm), ent, None

    def wait(self, ctx, pushed):
        t, ent, _ = pushed
        res = ctx.frames_wait(t) if self.batched else [ctx.frame_wait(t)]
        return [(r["have_vectors"], r["n_vectors"], r["motion"], r["quat"].tobytes(), ent[j][:r["n_vectors"]].tobytes() if r["have_vectors"] else b"")
                for j, r in enumerate(res)]

    # ---- the refusals, each by its code and a word of its text
    def _refused(self, call, word):
        with pytest.raises(OfpsHipError) as e:
            call()
        assert e.value.code == EINVAL and word in str(e.value), (self.name, word, str(e.value))

    def refuse_third(self, ctx, start, size):
        self._refused(lambda: self.push(ctx, start, size), "has not been collected")

    def refuse_others(self, ctx, start, size):
        H, W = self.frames.shape[1:]
        prm = ctx._frame_params(gc.BLOCK, gc.RANGE, True, 0.05, 2, 0.003, True, 16 / 9, 22.0, False, 200, 0.05, 1000, 0)
        ptr, t = self.frames[start:].ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(0)
        if self.batched:
            self._refused(lambda: ctx._check(ctx._lib.ofps_hip_push_frames_async(ctx._h, ptr, size, W, H, W - 1, W * H, C.byref(prm), None, C.byref(t))), "bad geometry")
        else:
            self._refused(lambda: ctx._check(ctx._lib.ofps_hip_push_frame_async(ctx._h, ptr, W, H, W - 1, C.byref(prm), None, None, C.byref(t))), "bad geometry")
        if self.klt:
            _, _, _, _, _, L, w, K = KLT_SET
            ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, 5, w, K)
            self._refused(lambda: self.push(ctx, start, size), "levels")
            ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
        elif self.filtered:
            ctx.set_sad_gate(BAD_GATE)
            self._refused(lambda: self.push(ctx, start, size), "contrast gate")
            ctx.set_sad_gate(CRITERIA["gate"])

    def run(self, ctx, mode):
        """mode: "serial" one ticket at a time, "inflight" two, "refused" two with the refused calls between them"""
        self.apply(ctx)
        try:
            sizes = CUT if self.batched else (1,) * len(self.frames)
            starts = [sum(sizes[:k]) for k in range(len(sizes))]
            out, pending = [], []
            for k, (start, size) in enumerate(zip(starts, sizes)):
                if len(pending) == (1 if mode == "serial" else 2):
                    if mode == "refused" and k == 2:
                        self.refuse_third(ctx, start, size)
                    out += self.wait(ctx, pending.pop(0))
                    if mode == "refused":
                        self.refuse_others(ctx, start, size)
                pending.append(self.push(ctx, start, size))
            while pending:
                out += self.wait(ctx, pending.pop(0))
            return out
        finally:
            self.restore(ctx)

    def check_not_trivial(self, ctx, out):
        cap = self.capacity(ctx)
        assert [o[0] for o in out] == [False] + [True] * (len(self.frames) - 1), self.name
        for j, (have, n, motion, quat, rec) in enumerate(out[1:], 1):
            if self.klt or self.filtered:
                assert 0 < n < cap, (self.name, j, n, cap)
            else:
                assert n == cap and len(np.unique(np.frombuffer(rec, np.uint32).reshape(cap, 4)[:, 2:], axis=0)) > 1, (self.name, j)
        if self.klt and not self.chained:
            assert tuple(o[1] for o in out[1:]) == bc.SMALL_KEPT[KLT_SET], self.name


FORMS = {f.name: f for f in (Form("frame plain", False), Form("frame filtered", False, filtered=True), Form("batch plain", True),
                             Form("batch filtered", True, filtered=True), Form("batch klt", True, klt=True),
                             Form("batch klt chained", True, klt=True, chained=True))}
_inflight = {}


def _reference(ctx, form):
    """the form's stream with two tickets in flight and nothing refused: run once, shared, checked for substance"""
    if form.name not in _inflight:
        out = form.run(ctx, "inflight")
        form.check_not_trivial(ctx, out)
        _inflight[form.name] = out
    return _inflight[form.name]


@pytest.mark.parametrize("name", list(FORMS))
def test_a_refused_push_leaves_the_stream_where_it_was(ctx, name):
    form = FORMS[name]
    want = _reference(ctx, form)
    got = form.run(ctx, "refused")
    assert len(got) == len(want) == len(form.frames)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, "frame", j, g[:3], w[:3])


@pytest.mark.parametrize("name", ["batch filtered", "batch klt chained"])
def test_a_buffer_that_grows_under_a_live_ticket_keeps_the_previous_frame(ctx, name):
    form = FORMS[name]
    want = form.run(ctx, "serial")
    form.check_not_trivial(ctx, want)
    got = _reference(ctx, form)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, "frame", j, g[:3], w[:3])
