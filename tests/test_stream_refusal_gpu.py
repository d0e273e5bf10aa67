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
always return one record per block, and their records are asserted not to be all alike.

The dense decoders' stream (ofps_hip_lk_push_frame[_fused]_async) under the same two runs: hip_lk down-sampled, reduced and through the plain
push, hip_flow with OFPS_HIP_FLOW_USE_PREVIOUS, and hip_klt (OFPS_HIP_FLOW_SPARSE) without and with klt_prediction.  Frames: dense_fused_cases'
texture, halfflat, move0, move1, movehalf, halfflat at 480 x 270 with LK = (1, 2, 1) -- tests/test_dense_fused_cpu.py pins the oracle's counts
149 / 312 / 311 / 169 / 149 of 312 at cap (24, 24) and 6179 / 12600 / 12600 / 6853 / 6179 of 12600 reduced at cap (150, 150) -- and
klt_batch_cases.SMALL at SMALL_SETS[1] for hip_klt.  Refused between the accepted pushes: the third push, stride W - 1, flags bit 31, levels 9
(LK), radius 8 (Farneback: winsize 17), levels 5 on 128 x 96 (hip_klt), OFPS_HIP_FLOW_USE_PREVIOUS without Farneback, a camera of 180 degrees
and OFPS_HIP_LK_FULLRES_RECORDS (fused), a frame of another size and other Farneback levels with a ticket pending.  Per frame have_vectors,
n_vectors, grid, island, field bits, quaternion bytes and record bits must be equal; hip_flow and predicted hip_klt are also compared with one
ticket at a time, where the upload runs on the compute stream and the mask / the prepare-ahead behind, not beside, the other ticket's flow."""
import ctypes as C

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import dense_fused_cases as fc
import klt_batch_cases as bc
import sad_gate_cases as gc

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
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
    def _refused(self, call, word, code=EINVAL):
        with pytest.raises(OfpsHipError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (self.name, word, e.value.code, str(e.value))

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


DENSE_KINDS = ("texture", "halfflat", "move0", "move1", "movehalf", "halfflat")
DENSE_TAIL = dict(detector=True, estimator=True, aspect=fc.CAM[0], fov_y_deg=fc.CAM[1], use_ransac=False, num_iters=fc.RANSAC_ITERS,
                  inlier_deg=fc.INLIER_DEG, num_samples=1000)


class DenseForm(Form):
    """one form of the dense decoders' stream: ofps_hip_lk_push_frame_fused_async, or (fused=False) ofps_hip_lk_push_frame_async"""
    batched = False

    def __init__(self, name, fused=True, cap=(24, 24), reduced=False, farneback=False, sparse=False, predicted=False):
        self.name, self.fused, self.farneback, self.sparse, self.predicted = name, fused, farneback, sparse, predicted
        if sparse:
            self.frames = np.ascontiguousarray(bc.sequence(bc.SMALL))
            self.other = fc.frame("texture")                                    # a frame of another size
            self.kw = dict(levels=KLT_SET[5], radius=KLT_SET[6], iters=KLT_SET[7], sparse=True)
            self.tail = dict(DENSE_TAIL, **KLT_PRM)
        else:
            self.frames = np.ascontiguousarray(np.stack([fc.frame(k) for k in DENSE_KINDS]))
            self.other = np.ascontiguousarray(bc.sequence(bc.SMALL)[0])
            L, w, K = fc.FB if farneback else fc.LK
            self.kw = dict(levels=L, radius=w, iters=K, max_w=cap[0], max_h=cap[1], contrast_mask=True, reduced=reduced, farneback=farneback,
                           use_previous=farneback)
            self.tail = dict(DENSE_TAIL, **fc.DETECTOR)
        if not fused:
            self.tail = {}
        self.seed = 77 if sparse else fc.SEED

    def apply(self, ctx):
        ctx.lk_reset()
        if self.sparse:
            ctx.set_klt(*KLT_SET[:5])
            ctx.set_klt_prediction(int(self.predicted))

    def restore(self, ctx):
        ctx.lk_reset()
        ctx.set_klt(); ctx.set_klt_prediction(0)

    def capacity(self, ctx):
        H, W = self.frames.shape[1:]
        if self.sparse:
            return ctx.klt_slot_count(W, H, KLT_SET[0])
        gw, gh = ctx.cv_grid(W, H, self.kw["max_w"], self.kw["max_h"])
        return gw * gh

    def _push(self, ctx, frame, seed, **change):
        kw = {**self.kw, **self.tail, **change}
        if self.fused:
            return ctx.lk_push_frame_fused_async(frame, seed=seed, **kw)
        return ctx.lk_push_frame_async(frame, **kw)

    def push(self, ctx, start, size):
        return self._push(ctx, self.frames[start], self.seed + start), None, None

    def wait(self, ctx, pushed):
        if self.fused:
            r = ctx.lk_frame_fused_wait(pushed[0])
            area, field = (None, b"") if r["motion"] is None else (r["motion"][0], r["motion"][1].tobytes())
            return [(r["have_vectors"], r["n_vectors"], area, r["quat"].tobytes(), r["entries"].tobytes() if r["have_vectors"] else b"", r["grid"], field)]
        got = ctx.lk_frame_wait(pushed[0])
        return [(False, 0, None, b"", b"", None, b"")] if got is None else [(True, len(got[0]), None, b"", got[0].tobytes(), got[1], b"")]

    def refuse_others(self, ctx, start, size):
        """with one ticket pending"""
        frame = self.frames[start]
        H, W = frame.shape
        flags = ctx._lk_flags(self.kw.get("contrast_mask", False), False, self.farneback, self.kw.get("use_previous", False), self.kw.get("reduced", False), 0, self.sparse)
        prm = ctx._frame_params(0, 0, True, 0.05, 3, 0.003, True, fc.CAM[0], fc.CAM[1], False, 200, 0.05, 1000, 0)
        ptr, t = frame.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(0)
        geometry = (self.kw["levels"], self.kw["radius"], self.kw["iters"], self.kw.get("max_w", 150), self.kw.get("max_h", 150))

        def raw(stride, flags):
            if self.fused:
                return ctx._check(ctx._lib.ofps_hip_lk_push_frame_fused_async(ctx._h, ptr, W, H, stride, *geometry, flags, C.byref(prm), C.byref(t)))
            return ctx._check(ctx._lib.ofps_hip_lk_push_frame_async(ctx._h, ptr, W, H, stride, *geometry, flags, C.byref(t)))
        self._refused(lambda: raw(W - 1, flags), "stride")
        self._refused(lambda: raw(W, flags | (1 << 31)), "unknown flags")
        if self.sparse:
            self._refused(lambda: self._push(ctx, frame, 0, levels=5), "levels")                 # 96 >> 4 = 6 < 8
        elif self.farneback:
            self._refused(lambda: self._push(ctx, frame, 0, radius=8), "winsize 17", EUNSUPPORTED)
        else:
            self._refused(lambda: self._push(ctx, frame, 0, levels=9), "out of range")
        if not self.farneback:
            self._refused(lambda: self._push(ctx, frame, 0, use_previous=True), "OFPS_HIP_FLOW_USE_PREVIOUS")
        if self.fused:
            self._refused(lambda: self._push(ctx, frame, 0, fov_y_deg=180.0), "bad camera")
            if self.sparse:                                     # hip_klt's own refusal of the flag comes first
                self._refused(lambda: self._push(ctx, frame, 0, fullres_records=True), "OFPS_HIP_FLOW_SPARSE excludes")
            else:
                self._refused(lambda: self._push(ctx, frame, 0, fullres_records=True), "no fused form", EUNSUPPORTED)
        self._refused(lambda: self._push(ctx, self.other, 0), "geometry change")
        if self.farneback:
            self._refused(lambda: self._push(ctx, frame, 0, levels=self.kw["levels"] - 1), "Farneback parameters changed")

    def check_not_trivial(self, ctx, out):
        cap = self.capacity(ctx)
        assert [o[0] for o in out] == [False] + [True] * (len(self.frames) - 1), self.name
        counts = [o[1] for o in out[1:]]
        print(f"{self.name}: n = {counts} of {cap}, islands {[o[2] for o in out[1:]]}")
        assert all(n > 0 for n in counts), (self.name, counts)
        if self.sparse:
            assert all(0 < n < cap for n in counts), (self.name, counts, cap)
            if not self.predicted:
                assert tuple(counts) == bc.SMALL_KEPT[KLT_SET], (self.name, counts)
        else:
            assert sum(0 < n < cap for n in counts) >= 3, (self.name, counts, cap)
            if self.fused:
                assert out[3][2] is not None, (self.name, "move0 -> move1: no island")


FORMS = {f.name: f for f in (Form("frame plain", False), Form("frame filtered", False, filtered=True), Form("batch plain", True),
                             Form("batch filtered", True, filtered=True), Form("batch klt", True, klt=True),
                             Form("batch klt chained", True, klt=True, chained=True),
                             DenseForm("dense lk"), DenseForm("dense lk reduced", cap=(150, 150), reduced=True),
                             DenseForm("dense flow", farneback=True), DenseForm("dense lk plain", fused=False),
                             DenseForm("dense klt", sparse=True), DenseForm("dense klt predicted", sparse=True, predicted=True))}
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


@pytest.mark.parametrize("name", ["dense flow", "dense klt predicted"])
def test_a_dense_stream_one_ticket_at_a_time_equals_two_in_flight(ctx, name):
    """serial: the upload runs on the compute stream and the mask / prepare-ahead behind the other ticket's flow instead of beside it"""
    form = FORMS[name]
    want = form.run(ctx, "serial")
    form.check_not_trivial(ctx, want)
    got = _reference(ctx, form)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, "frame", j, g[:3], w[:3])
