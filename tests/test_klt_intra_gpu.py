"""hip_klt's intra test and scene-cut rule (include/ofps_hip.h N3i) on the GPU, bit for bit against the restatement
tests/indep_klt_intra.py: the two stage forms, the one-pair forms with and without slots, mean removal, the forward-backward check and
prediction, the batch form in both ref_modes and chained, the sparse fused form and the batched stream across a cut, the multi-device
workers, the compaction's large path, and the settings."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import indep_klt_intra as ii
import indep_klt_pred as ip
import klt_cases as kc
import klt_intra_cases as xc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
GUARD_WORD = 0x5A17C0DE
SEED = 77
IDENTITY = (1.0, 0.0, 0.0, 0.0)
QUAT_BOUND = 2e-6                                            # N3b's bound on the quaternion of the same records through two forms
L, w, K = xc.SET
TAIL = dict(detector=True, min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16, use_ransac=False)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    assert c.get_klt_intra() == 0 and c.get_klt_cut() == 0
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _reset(ctx):
    ctx.set_klt(); ctx.set_klt_fb(0); ctx.set_klt_mean_removal(0); ctx.set_klt_prediction(0); ctx.set_klt_batch_prediction(0)
    ctx.set_klt_intra(0); ctx.set_klt_cut(0)
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
        return host[:self.words].view(dtype).copy()

    def free(self):
        self.ctx.free(self.ptr)


def _dev_frame(ctx, img, pad):
    """-> (device pointer, stride) of a copy of img whose rows are W + pad bytes, the padding 0xA5"""
    view, stride = kc.padded(img, pad)
    d = ctx.malloc(view.base.size)
    ctx.memcpy_h2d(d, view.base)
    return d, stride


# ------------------------------------------------------------------------------------------------ 1: the stage forms
def _edge_points(W, H):
    """every corner, points on every edge and one step inside, and seeded interior points"""
    rng = np.random.default_rng(5)
    xs, ys = [0, 1, 6, W // 2, W - 8, W - 2, W - 1], [0, 1, 6, H // 2, H - 8, H - 2, H - 1]
    pts = [(x, y) for x in xs for y in ys]
    pts += list(zip(rng.integers(0, W, 70).tolist(), rng.integers(0, H, 70).tolist()))
    return np.array(pts, np.int32)


@pytest.mark.parametrize("radius", [1, 4, 7])
def test_activity_stage_forms_match_the_restatement(ctx, radius):
    img = kc.warp_pair(97, 65, (1.3, -0.6))[0]
    H, W = img.shape
    pts = _edge_points(W, H)
    assert len(pts) > 64 and len(pts) % 64 != 0 and len(pts) % 16 != 0          # more than one workgroup, ragged in the wave and in the slot group
    want = ii.activity(img, pts, radius)
    assert len(set(want.tolist())) > 50
    np.testing.assert_array_equal(ctx.klt_activity(img, pts, radius), want)
    view, stride = kc.padded(img, 13)
    np.testing.assert_array_equal(ctx.klt_activity(view, pts, radius, stride=stride), want)
    # the literals of the definition
    dot = np.zeros((8, 8), np.uint8); dot[4, 4] = 255
    corner = np.full((8, 8), 200, np.uint8); corner[:2, :2] = [[10, 20], [30, 40]]
    if radius == 1:
        assert ctx.klt_activity(dot, [[4, 4]], 1).tolist() == [451] and ctx.klt_activity(corner, [[0, 0]], 1).tolist() == [80]
    assert ctx.klt_activity(np.full((9, 11), 117, np.uint8), [[5, 4], [0, 0], [10, 8]], radius).tolist() == [0, 0, 0]
    # the _dev form: points outside the frame give A = 0 and touch nothing; the host form refuses them
    outside = np.array([[-1, 3], [W, 3], [3, -1], [3, H], [-2 ** 31, 5], [2 ** 31 - 1, 2 ** 31 - 1]], np.int32)
    both = np.concatenate([pts, outside])
    d_img, stride = _dev_frame(ctx, img, 7)
    b_pts, b_out = _DevBuf(ctx, 2 * len(both), both), _DevBuf(ctx, len(both))
    try:
        ctx.klt_activity_dev(d_img, W, H, stride, b_pts.ptr, len(both), radius, b_out.ptr)
        ctx.sync()
        np.testing.assert_array_equal(b_out.read(np.uint32), np.concatenate([want, np.zeros(len(outside), np.uint32)]))
    finally:
        b_pts.free(); b_out.free(); ctx.free(d_img)
    for p in outside[:4]:
        with pytest.raises(OfpsHipError):
            ctx.klt_activity(img, [p], radius)
    assert ctx.klt_activity(img, [[3, 3]], radius).tolist() == [int(ii.activity(img, [[3, 3]], radius)[0])]        # a valid call behind the refusals
    assert len(ctx.klt_activity(img, np.zeros((0, 2), np.int32), radius)) == 0


def test_verdict_stage_forms_match_the_restatement(ctx):
    st, cnt = ctx.klt_intra([[3, -4, 57728, 0], [3, -4, 57727, 0]], [451, 451], 8)
    assert st.tolist() == [6, 0] and cnt.tolist() == [2, 1]
    big = np.array([2 ** 31, 2 ** 32 - 1, 2 ** 31 + 5, 134217727, 134217728], np.uint32)
    quads = [[0, 0, 2 ** 31 - 1, 0]] * 5
    for q in (1, 255):
        st, cnt = ctx.klt_intra(quads, big, q)
        want = ii.verdict(quads, big.tolist(), q)
        assert st.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()
    assert ctx.klt_intra(quads, big, 1)[0].tolist() == [0, 0, 0, 6, 0]
    assert ctx.klt_intra([[0, 0, 0, 0]], [0], 255)[0].tolist() == [6]
    rng = np.random.default_rng(9)
    n = 1000                                                  # four workgroups, the last ragged
    quads = np.stack([rng.integers(-999, 999, n), rng.integers(-999, 999, n), rng.integers(0, 60000, n), rng.integers(0, 8, n)], 1).astype(np.int32)
    act = rng.integers(0, 400, n).astype(np.uint32)
    seen_cut = set()
    for q, P in ((8, 0), (8, 50), (3, 50), (255, 1), (1, 100), (40, 37)):
        want_st, want_cnt, cut = ii.verdict(quads, act.tolist(), q, P)
        st, cnt = ctx.klt_intra(quads, act, q, P)
        np.testing.assert_array_equal(st, want_st, err_msg=f"q {q} P {P}")
        assert cnt.tolist() == want_cnt.tolist(), (q, P)
        seen_cut.add(cut)
    assert seen_cut == {False, True}
    # the cut rule's equality, by hand: 5 intra of 10 at P = 50 is a cut, 4 of 10 is not; no candidate is a cut
    ten = [[1, 1, 10 ** 6, 0]] * 5 + [[1, 1, 1, 0]] * 5
    assert ctx.klt_intra(ten, [100] * 10, 8, 50)[0].tolist() == [6] * 5 + [7] * 5
    assert ctx.klt_intra(ten[1:] + [[1, 1, 1, 0]], [100] * 10, 8, 50)[0].tolist() == [6] * 4 + [0] * 6
    st, cnt = ctx.klt_intra([[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3]], [7, 7, 7], 8, 1)
    assert st.tolist() == [1, 2, 3] and cnt.tolist() == [0, 0]
    # the _dev form, with and without counters
    want_st, want_cnt, _ = ii.verdict(quads, act.tolist(), 3, 50)
    b_q, b_a = _DevBuf(ctx, 4 * n, quads), _DevBuf(ctx, n, act)
    b_st, b_cnt = _DevBuf(ctx, n), _DevBuf(ctx, 2)
    try:
        ctx.klt_intra_dev(b_q.ptr, b_a.ptr, n, 3, 50, b_st.ptr, b_cnt.ptr)
        ctx.sync()
        np.testing.assert_array_equal(b_st.read(np.int32), want_st)
        assert b_cnt.read(np.uint32).tolist() == want_cnt.tolist()
        ctx.klt_intra_dev(b_q.ptr, b_a.ptr, n, 3, 50, b_st.ptr, None)
        ctx.sync()
        np.testing.assert_array_equal(b_st.read(np.int32), want_st)
    finally:
        for b in (b_q, b_a, b_st, b_cnt):
            b.free()
    for q, P in ((0, 0), (256, 0), (-1, 0), (8, 101), (8, -1)):
        with pytest.raises(OfpsHipError):
            ctx.klt_intra(quads, act, q, P)
    assert ctx.klt_intra(quads[:1], act[:1], 8)[0].tolist() == ii.verdict(quads[:1], act[:1].tolist(), 8)[0].tolist()


# ------------------------------------------------------------------------------------------------ 2: the one-pair forms
# (name, cell, L, w, K, mean removal, F, q, P): every q is chosen so that the pair has intra and kept tracks, which the test asserts of the
# restatement before it looks at the device; w = 7 at cell 8: the windows overlap and clamp at every edge
PAIRS = {"warp96": lambda: kc.warp_pair(96, 64, (1.3, -0.6)), "warp97": lambda: kc.warp_pair(97, 65, (1.3, -0.6)), "repaint": xc.repaint_pair,
         "cut": xc.cut_pair}
FLOW_CASES = [("repaint", 16, 2, 4, 10, False, 0, 8, 0), ("repaint", 16, 2, 4, 10, False, 0, 8, 25), ("repaint", 16, 2, 4, 10, True, 0, 8, 0),
              ("repaint", 16, 2, 4, 10, False, 64, 8, 25), ("repaint", 16, 2, 4, 10, True, 64, 8, 0), ("cut", 16, 2, 4, 10, False, 0, 8, 50),
              ("warp97", 8, 2, 7, 10, False, 0, 3, 0), ("warp96", 8, 1, 1, 3, False, 0, 3, 0), ("warp97", 16, 2, 4, 10, False, 0, 3, 90),
              ("warp97", 16, 2, 4, 10, False, 0, 3, 40)]


@functools.lru_cache(maxsize=None)
def _expect(case):
    name, cell, Lc, wc, Kc, zm, F, q, P = case
    prev, cur = PAIRS[name]()
    raw = ip.flow_from(prev, cur, Lc, wc, Kc, None, cell=cell, mean_removal=zm, fb_limit=F)
    return raw, ii.apply(raw, prev, wc, q, P)


@pytest.mark.parametrize("case", FLOW_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_flow_forms_match_the_restatement(ctx, case):
    name, cell, Lc, wc, Kc, zm, F, q, P = case
    prev, cur = PAIRS[name]()
    H, W = prev.shape
    raw, want = _expect(case)
    n_cand, n_intra = want["counts"].tolist()
    print(case, "candidates", n_cand, "intra", n_intra, "cut", want["cut"], "kept", want["count"], "of", raw["count"])
    assert 0 < n_intra and (n_intra < n_cand or name == "cut")
    # with the forward-backward check on, the check has dropped the repainted tracks already (status 5): they still count as intra
    # candidates, so the cut rule at 25 percent fires on them, and without it the test changes nothing
    if F and not P:
        assert want["slots"].tobytes() == raw["slots"].tobytes() and (raw["slots"][:, 5] == 5).any()
    else:
        assert want["slots"].tobytes() != raw["slots"].tobytes() and want["count"] < raw["count"]
    ctx.set_klt(cell); ctx.set_klt_mean_removal(int(zm)); ctx.set_klt_fb(F)
    try:
        # the stages: the unfiltered slots and quads, the activities, the verdict and its counters
        ctx.set_klt_intra(0); ctx.set_klt_cut(P)              # P alone has no effect
        rec0, slots0 = ctx.klt_flow(prev, cur, Lc, wc, Kc, want_slots=True)
        np.testing.assert_array_equal(slots0, raw["slots"])
        assert _bits(rec0).tobytes() == _bits(raw["records"]).tobytes()
        has = slots0[:, 0] >= 0
        quads = np.zeros((len(slots0), 4), np.int32); quads[:, 3] = 1
        quads[has] = ctx.klt_track(prev, cur, slots0[has, :2], Lc, wc, Kc)
        np.testing.assert_array_equal(quads[:, 2], raw["residuals"])
        np.testing.assert_array_equal(quads[:, 3], raw["slots"][:, 5])
        act = np.zeros(len(slots0), np.uint32)
        act[has] = ctx.klt_activity(prev, slots0[has, :2], wc)
        cand = np.isin(slots0[:, 5], ii.CANDIDATES)
        np.testing.assert_array_equal(act[cand], want["activity"][cand])
        st, cnt = ctx.klt_intra(quads, act, q, P)
        np.testing.assert_array_equal(st, want["slots"][:, 5])
        assert cnt.tolist() == [n_cand, n_intra]
        # the decoder: host form with slots
        ctx.set_klt_intra(q)
        rec, slots = ctx.klt_flow(prev, cur, Lc, wc, Kc, want_slots=True)
        np.testing.assert_array_equal(slots, want["slots"])
        assert len(rec) == want["count"] and _bits(rec).tobytes() == _bits(want["records"]).tobytes()
        assert len(ctx.klt_flow(prev, cur, Lc, wc, Kc)) == want["count"]
        # the _dev form on padded rows, without slots (flags alone) and with them
        d_prev, stride = _dev_frame(ctx, prev, 13)
        d_cur, _ = _dev_frame(ctx, cur, 13)
        ns = ctx.klt_slot_count(W, H)
        try:
            for want_slots in (False, True):
                b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns) if want_slots else None
                try:
                    ctx.klt_flow_dev(d_prev, d_cur, W, H, stride, Lc, wc, Kc, b_rec.ptr, b_cnt.ptr, b_slots.ptr if b_slots else None)
                    ctx.sync()
                    assert int(b_cnt.read(np.uint32)[0]) == want["count"]
                    got = b_rec.read(np.float32).reshape(-1, 4)[:want["count"]]
                    assert _bits(got).tobytes() == _bits(want["records"]).tobytes()
                    if b_slots:
                        np.testing.assert_array_equal(b_slots.read(np.int32).reshape(-1, 6), want["slots"])
                finally:
                    for b in (b_rec, b_cnt, b_slots):
                        if b:
                            b.free()
        finally:
            ctx.free(d_prev); ctx.free(d_cur)
    finally:
        _reset(ctx)


@functools.lru_cache(maxsize=None)
def _cut_chain(q=xc.Q, P=50, **kw):
    return ii.flow_chain(xc.cut_sequence(), L, w, K, q, P, **kw)


def test_flow_from_with_prediction_across_the_cut(ctx):
    fr = xc.cut_sequence()
    want = _cut_chain()
    assert want[1]["cut"] and np.abs(want[1]["guesses"]).sum() > 0 and not want[2]["guesses"].any() and want[2]["count"] > 40
    ctx.set_klt_intra(xc.Q); ctx.set_klt_cut(50)
    try:
        prev_slots = None
        for k in range(3):
            rec, slots = ctx.klt_flow_from(fr[k], fr[k + 1], L, w, K, prev_slots, want_slots=True)
            np.testing.assert_array_equal(slots, want[k]["slots"], err_msg=f"pair {k}")
            assert _bits(rec).tobytes() == _bits(want[k]["records"]).tobytes(), k
            prev_slots = slots
        assert (want[1]["slots"][:, 5] != 0).all()            # (every candidate of the cut pair is intra itself: status 6, none left for 7)
    finally:
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ 3: the batch forms
@functools.lru_cache(maxsize=None)
def _batch_frames(ref_mode):
    if ref_mode:
        return xc.key_sequence()
    fr = xc.cut_sequence().copy()                             # (clean, cut, repaint): the last frame of the new scene with a repainted rectangle
    r0, r1, c0, c1 = xc.REPAINT
    fr[3, r0:r1, c0:c1] = xc.other(fr.shape[2], fr.shape[1])[r0:r1, c0:c1]
    return fr


@pytest.mark.parametrize("ref_mode", [0, 1], ids=["chain", "key"])
def test_batch_of_clean_cut_and_repaint(ctx, ref_mode):
    fr = _batch_frames(ref_mode)
    want = ii.flow_batch(fr, L, w, K, ref_mode, xc.Q, 50)
    cuts = [a["cut"] for a in want]
    print("ref_mode", ref_mode, "counters", [a["counts"].tolist() for a in want], "cut", cuts, "kept", [a["count"] for a in want])
    assert cuts == [False, True, False] and want[0]["counts"][1] == 0 and 0 < want[2]["counts"][1] < want[2]["counts"][0]
    ctx.set_klt_intra(xc.Q); ctx.set_klt_cut(50)
    try:
        for want_slots in (True, False):
            got = ctx.klt_flow_batch(fr, L, w, K, ref_mode, want_slots=want_slots)
            rec, counts = got[0], got[1]
            for k, a in enumerate(want):
                assert int(counts[k]) == a["count"], (k, int(counts[k]), a["count"])
                assert _bits(rec[k][:a["count"]]).tobytes() == _bits(a["records"]).tobytes(), k
                if want_slots:
                    np.testing.assert_array_equal(got[2][k], a["slots"], err_msg=f"item {k}")
        # the chained batch: item 2 starts from zero behind the cut, as the restatement's chain does
        chained = ii.flow_batch(fr, L, w, K, ref_mode, xc.Q, 50, chained=True)
        assert np.abs(chained[1]["guesses"]).sum() > 0 and not chained[2]["guesses"].any()
        for want_slots in (True, False):
            got = ctx.klt_flow_batch_from(fr, L, w, K, ref_mode, None, want_slots=want_slots)
            for k, a in enumerate(chained):
                assert int(got[1][k]) == a["count"], k
                assert _bits(got[0][k][:a["count"]]).tobytes() == _bits(a["records"]).tobytes(), k
                if want_slots:
                    np.testing.assert_array_equal(got[2][k], a["slots"], err_msg=f"chained item {k}")
    finally:
        _reset(ctx)


def test_chained_batch_equals_the_sparse_stream_across_the_cut(ctx):
    fr = xc.cut_sequence()
    want = _cut_chain()
    ctx.set_klt_intra(xc.Q); ctx.set_klt_cut(50); ctx.set_klt_prediction(1); ctx.set_klt_batch_prediction(1)
    try:
        rec, counts = ctx.klt_flow_batch(fr, L, w, K, 0)[:2]
        ctx.lk_reset()
        stream = [ctx.lk_push_frame(np.ascontiguousarray(f), L, w, K, sparse=True) for f in fr]
        assert stream[0] is None
        for k, a in enumerate(want):
            ent = stream[k + 1][0]
            assert int(counts[k]) == a["count"] == len(ent), (k, int(counts[k]), a["count"], len(ent))
            assert _bits(rec[k][:a["count"]]).tobytes() == _bits(a["records"]).tobytes() == _bits(ent).tobytes(), k
    finally:
        ctx.lk_reset(); _reset(ctx)


# ------------------------------------------------------------------------------------------------ 4: the fused sparse form
@pytest.mark.parametrize("ahead", [False, True], ids=["sync", "async"])
def test_fused_sparse_form_across_the_cut(ctx, ahead):
    fr = [np.ascontiguousarray(f) for f in xc.cut_sequence()]
    want = _cut_chain()
    ctx.set_klt_intra(xc.Q); ctx.set_klt_cut(50); ctx.set_klt_prediction(1)

    def run(frames):
        ctx.lk_reset()
        if not ahead:
            return [ctx.lk_push_frame_fused(f, L, w, K, sparse=True, seed=SEED, **TAIL) for f in frames]
        res, tickets = [], [ctx.lk_push_frame_fused_async(frames[0], L, w, K, sparse=True, seed=SEED, **TAIL)]
        for k in range(1, len(frames)):
            tickets.append(ctx.lk_push_frame_fused_async(frames[k], L, w, K, sparse=True, seed=SEED, **TAIL))
            res.append(ctx.lk_frame_fused_wait(tickets[k - 1]))
        res.append(ctx.lk_frame_fused_wait(tickets[-1]))
        return res

    try:
        got = run(fr)
        for k, a in enumerate(want):
            g = got[k + 1]
            assert g["have_vectors"] and g["n_vectors"] == a["count"], (k, g["n_vectors"], a["count"])
            assert _bits(g["entries"]).tobytes() == _bits(a["records"]).tobytes(), k
        cut = got[2]
        assert cut["n_vectors"] == 0 and cut["motion"] is None and cut["quat"].tolist() == list(IDENTITY)
        assert np.abs(got[1]["quat"] - IDENTITY).max() > 1e-5                   # the estimator ran on the clean pair
        fresh = run(fr[2:])                                    # the frame behind the cut: a freshly started stream's answer
        assert fresh[1]["n_vectors"] == got[3]["n_vectors"] > 40 and _bits(fresh[1]["entries"]).tobytes() == _bits(got[3]["entries"]).tobytes()
        assert np.abs(fresh[1]["quat"] - got[3]["quat"]).max() <= QUAT_BOUND
        assert (fresh[1]["motion"] is None) == (got[3]["motion"] is None)
        if got[3]["motion"] is not None:
            assert fresh[1]["motion"][0] == got[3]["motion"][0]
    finally:
        ctx.lk_reset(); _reset(ctx)


# ------------------------------------------------------------------------------------------------ 5: the batched stream
def _stream(c, frames, sizes):
    out, start, pending = [], 0, []

    def collect():
        t, ent = pending.pop(0)
        for j, r in enumerate(c.frames_wait(t)):
            out.append(dict(r, entries=ent[j][:r["n_vectors"]].copy()))

    for size in sizes:
        batch = np.ascontiguousarray(frames[start:start + size])
        ent = np.zeros((size, c.batch_record_capacity(batch.shape[2], batch.shape[1]), 4), np.float32)
        pending.append((c.push_frames_async(batch, seed=SEED + start, out_entries=ent, **TAIL), ent))
        if len(pending) == 2:
            collect()
        start += size
    while pending:
        collect()
    return out


def test_batched_stream_answers_do_not_depend_on_the_tickets(ctx):
    fr = xc.cut_sequence()
    want = _cut_chain()
    ctx.set_klt_intra(xc.Q); ctx.set_klt_cut(50); ctx.set_klt_prediction(1); ctx.set_klt_batch_prediction(1)
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
    try:
        runs = []
        for sizes in ((4,), (2, 2), (1, 1, 1, 1), (3, 1)):
            ctx.reset_frames()
            got = _stream(ctx, fr, sizes)
            assert not got[0]["have_vectors"] and got[0]["n_vectors"] == 0
            for k, a in enumerate(want):
                g = got[k + 1]
                assert g["have_vectors"] and g["n_vectors"] == a["count"], (sizes, k, g["n_vectors"], a["count"])
                assert _bits(g["entries"]).tobytes() == _bits(a["records"]).tobytes(), (sizes, k)
            assert got[2]["n_vectors"] == 0 and got[2]["motion"] is None and np.asarray(got[2]["quat"]).tolist() == list(IDENTITY)
            runs.append(got)
        for got in runs[1:]:
            for j, (g, r) in enumerate(zip(got, runs[0])):
                assert (g["motion"] is None) == (r["motion"] is None) and np.abs(np.asarray(g["quat"]) - np.asarray(r["quat"])).max() <= QUAT_BOUND, j
    finally:
        ctx.reset_frames(); _reset(ctx)


# ------------------------------------------------------------------------------------------------ 6: the multi-device workers
def test_multi_device_workers_read_both_variables():
    env = dict(os.environ, OFPS_HIP_BATCH_DECODER="1", OFPS_HIP_KLT_LEVELS=str(L), OFPS_HIP_KLT_RADIUS=str(w), OFPS_HIP_KLT_ITERS=str(K),
               OFPS_HIP_KLT_INTRA=str(xc.Q), OFPS_HIP_KLT_CUT="50", KLT_CHILD_SEED=str(SEED))
    for name in ("OFPS_HIP_KLT_MEAN_REMOVAL", "OFPS_HIP_KLT_FB", "OFPS_HIP_KLT_PREDICTION", "OFPS_HIP_KLT_BATCH_PREDICTION", "OFPS_HIP_KLT_CELL"):
        env.pop(name, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_klt_intra_child.py")], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["settings_seen"] == [xc.Q, 50]
    want = ii.flow_chain(xc.cut_sequence(), L, w, K, xc.Q, 50, predict_on=False)        # the workers never predict
    got = child["frames"]
    assert [g["have_vectors"] for g in got] == [False, True, True, True]
    for k, a in enumerate(want):
        assert got[k + 1]["n_vectors"] == a["count"], (k, got[k + 1]["n_vectors"], a["count"])
        assert got[k + 1]["entries"] == _bits(a["records"]).reshape(-1).tolist(), k
    assert want[1]["cut"] and got[2]["n_vectors"] == 0 and got[2]["motion"] is None
    assert np.array(got[2]["quat"], np.uint32).view(np.float32).tolist() == list(IDENTITY)       # (by value: a zero may carry a sign)


# ------------------------------------------------------------------------------------------------ 7: the compaction's large path
def test_large_path_keeps_exactly_the_verdicts_subset(ctx):
    """more than 32,768 slots: the expected values are the device's own stages (the unfiltered decoder, the track stage's residuals, the
    activity stage) under the NumPy verdict"""
    a, b = xc.repaint_pair()
    prev, cur = np.tile(a, (11, 16))[:1032], np.tile(b, (11, 16))[:1032]
    H, W = prev.shape
    ctx.set_klt(8)
    ns = ctx.klt_slot_count(W, H)
    assert (W, H) == (2048, 1032) and ns == 33024 > 32768
    Lb, wb, Kb, q = 1, 1, 10, xc.Q
    d_prev, stride = _dev_frame(ctx, prev, 0)
    d_cur, _ = _dev_frame(ctx, cur, 0)
    b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns)
    b_pts, b_quads, b_act = _DevBuf(ctx, 2 * ns), _DevBuf(ctx, 4 * ns), _DevBuf(ctx, ns)
    try:
        ctx.klt_flow_dev(d_prev, d_cur, W, H, stride, Lb, wb, Kb, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        n0 = int(b_cnt.read(np.uint32)[0])
        rec0, slots0 = b_rec.read(np.float32).reshape(-1, 4)[:n0], b_slots.read(np.int32).reshape(-1, 6)
        assert n0 == int((slots0[:, 5] == 0).sum())
        ctx.memcpy_h2d(b_pts.ptr, np.concatenate([np.ascontiguousarray(slots0[:, :2]).view(np.uint32).ravel(), np.full(GUARD, GUARD_WORD, np.uint32)]))
        ctx.klt_track_dev(d_prev, d_cur, W, H, stride, b_pts.ptr, ns, Lb, wb, Kb, b_quads.ptr)
        ctx.klt_activity_dev(d_prev, W, H, stride, b_pts.ptr, ns, wb, b_act.ptr)
        ctx.sync()
        quads, act = b_quads.read(np.int32).reshape(-1, 4), b_act.read(np.uint32)
        has = slots0[:, 0] >= 0
        np.testing.assert_array_equal(quads[has, 3], slots0[has, 5])
        quads[~has] = (0, 0, 0, 1)
        cand = np.isin(quads[:, 3], ii.CANDIDATES)
        intra = cand & (16 * quads[:, 2].astype(np.int64) >= q * 256 * act.astype(np.int64))
        print("large path: slots", ns, "kept unfiltered", n0, "candidates", int(cand.sum()), "intra", int(intra.sum()))
        assert 0 < intra.sum() < cand.sum()
        want_st = np.where(intra & (quads[:, 3] == 0), ii.ST_INTRA, quads[:, 3])
        keep_of_kept = ~intra[slots0[:, 5] == 0]              # which of the unfiltered records stay
        ctx.set_klt_intra(q)
        ctx.klt_flow_dev(d_prev, d_cur, W, H, stride, Lb, wb, Kb, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        ctx.sync()
        n1 = int(b_cnt.read(np.uint32)[0])
        assert n1 == int(keep_of_kept.sum()) < n0
        assert _bits(b_rec.read(np.float32).reshape(-1, 4)[:n1]).tobytes() == _bits(rec0[keep_of_kept]).tobytes()
        slots1 = b_slots.read(np.int32).reshape(-1, 6)
        np.testing.assert_array_equal(slots1[:, 5], want_st)
        np.testing.assert_array_equal(slots1[:, :5], slots0[:, :5])
    finally:
        for buf in (b_rec, b_cnt, b_slots, b_pts, b_quads, b_act):
            buf.free()
        ctx.free(d_prev); ctx.free(d_cur)
        _reset(ctx)


# ------------------------------------------------------------------------------------------------ 8: the settings
def test_setters_getters_options_and_q_zero(ctx):
    try:
        for bad in (-1, 256, 1000):
            ctx.set_klt_intra(9)
            with pytest.raises(OfpsHipError):
                ctx.set_klt_intra(bad)
            assert ctx.get_klt_intra() == 9                   # the setting stays as it was
            ctx.set_klt_intra(255); assert ctx.get_klt_intra() == 255
        for bad in (-1, 101):
            ctx.set_klt_cut(30)
            with pytest.raises(OfpsHipError):
                ctx.set_klt_cut(bad)
            assert ctx.get_klt_cut() == 30
            ctx.set_klt_cut(100); assert ctx.get_klt_cut() == 100
        ctx.set_klt_intra(0); ctx.set_klt_cut(0)
        ctx.set_option("OFPS_HIP_KLT_INTRA", "12"); ctx.set_option("OFPS_HIP_KLT_CUT", "40")
        assert (ctx.get_klt_intra(), ctx.get_klt_cut()) == (12, 40)
        for name, bad in (("OFPS_HIP_KLT_INTRA", "256"), ("OFPS_HIP_KLT_INTRA", "-1"), ("OFPS_HIP_KLT_INTRA", "8x"), ("OFPS_HIP_KLT_CUT", "101"),
                          ("OFPS_HIP_KLT_CUT", "1e1")):
            with pytest.raises(OfpsHipError):
                ctx.set_option(name, bad)
        assert (ctx.get_klt_intra(), ctx.get_klt_cut()) == (12, 40)
        ctx.set_option("OFPS_HIP_KLT_INTRA", None); ctx.set_option("OFPS_HIP_KLT_CUT", "")
        assert (ctx.get_klt_intra(), ctx.get_klt_cut()) == (0, 0)
        # q = 0, with and without P: today's slots and records
        prev, cur = xc.repaint_pair()
        raw = ip.flow_from(prev, cur, L, w, K)
        for P in (0, 50):
            ctx.set_klt_cut(P)
            rec, slots = ctx.klt_flow(prev, cur, L, w, K, want_slots=True)
            np.testing.assert_array_equal(slots, raw["slots"])
            assert _bits(rec).tobytes() == _bits(raw["records"]).tobytes()
        # the stage form ofps_hip_klt_track never applies the test
        ctx.set_klt_intra(1)
        pts = raw["slots"][raw["slots"][:, 0] >= 0, :2]
        assert set(ctx.klt_track(prev, cur, pts, L, w, K)[:, 3].tolist()) <= {0, 2, 3}
    finally:
        _reset(ctx)
