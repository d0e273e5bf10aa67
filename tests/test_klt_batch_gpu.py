"""-m gpu: hip_klt's batch form (include/ofps_hip.h N3b) through the C ABI.  ofps_hip_klt_flow_batch[_dev] against the restatement
tests/indep_klt.py item by item, bit for bit (chain and key mode, padded rows and frames, guard words, the second compaction round, the
smallest and a large batch against the one-pair forms); the batched stream with the decoder at KLT against six fused sparse calls of the
dense decoders' stream; refusals; the switch back at SAD against a context that never saw a klt call; options and environment variables; the
multi-device workers; the C++ host tool.  Every comparison is bit for bit but the quaternion's (2e-6, the batch-against-single bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import indep_klt as ik
import klt_batch_cases as bc
import klt_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
QUAT_BOUND = 2e-6
GUARD = 64
GUARD_WORD = 0x5A17C0DE
IDENTITY = np.array([1, 0, 0, 0], np.float32)
SEED = 77


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(ctx, params):
    cell, r, min_score, min_eig, R, L, w, K = params
    ctx.set_klt(cell, r, min_score, min_eig, R)
    return L, w, K


class _DevBuf:
    """device memory of `words` 32-bit words with GUARD more behind them"""

    def __init__(self, ctx, words):
        self.ctx, self.words = ctx, int(words)
        self.ptr = ctx.malloc(4 * (self.words + GUARD))
        ctx.memcpy_h2d(self.ptr, np.full(self.words + GUARD, GUARD_WORD, np.uint32))

    def read(self, dtype):
        host = np.zeros(self.words + GUARD, np.uint32)
        self.ctx.memcpy_d2h(host, self.ptr)
        assert (host[self.words:] == GUARD_WORD).all(), "guard words behind a device output were overwritten"
        return host[:self.words].view(dtype)

    def free(self):
        self.ctx.free(self.ptr)


def _upload(ctx, view):
    """a [n, H, W] view of a (possibly wider and taller) buffer -> (device pointer, stride, frame pitch)"""
    buf = view if view.flags["C_CONTIGUOUS"] else view.base              # the padded views are slices [:, :H, :W] of their buffer
    assert buf.ndim == 3 and buf.flags["C_CONTIGUOUS"] and buf.ctypes.data == view.ctypes.data
    ptr = ctx.malloc(buf.size)
    ctx.memcpy_h2d(ptr, buf)
    return ptr, buf.shape[2], buf.shape[1] * buf.shape[2]


def _batch_dev(ctx, view, ref_mode, L, w, K, want_slots=True):
    """-> (records [pairs, ns, 4], counts [pairs], slots [pairs, ns, 6] or the untouched words of the buffer nobody was given)"""
    n, H, W = view.shape
    pairs, ns = n - 1, ctx.klt_slot_count(W, H)
    d, stride, pitch = _upload(ctx, view)
    b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * pairs * ns), _DevBuf(ctx, pairs), _DevBuf(ctx, 6 * pairs * ns)
    try:
        ctx.klt_flow_batch_dev(d, n, W, H, stride, pitch, ref_mode, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr if want_slots else None)
        ctx.sync()
        slots = b_slots.read(np.int32).reshape(pairs, ns, 6) if want_slots else b_slots.read(np.uint32)
        return b_rec.read(np.float32).reshape(pairs, ns, 4), b_cnt.read(np.uint32).copy(), slots
    finally:
        for b in (b_rec, b_cnt, b_slots):
            b.free()
        ctx.free(d)


def _pairs_dev(ctx, view, ref_mode, L, w, K):
    """the merged one-pair device form on every pair of the sequence -> [(records[:count], count, slots)]"""
    n, H, W = view.shape
    ns = ctx.klt_slot_count(W, H)
    d, stride, pitch = _upload(ctx, view)
    out = []
    try:
        for k in range(n - 1):
            a, b = bc.pair_of(k, ref_mode)
            b_rec, b_cnt, b_slots = _DevBuf(ctx, 4 * ns), _DevBuf(ctx, 1), _DevBuf(ctx, 6 * ns)
            ctx.klt_flow_dev(d + a * pitch, d + b * pitch, W, H, stride, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
            ctx.sync()
            count = int(b_cnt.read(np.uint32)[0])
            out.append((b_rec.read(np.float32).reshape(ns, 4)[:count].copy(), count, b_slots.read(np.int32).reshape(ns, 6).copy()))
            for x in (b_rec, b_cnt, b_slots):
                x.free()
    finally:
        ctx.free(d)
    return out


def _check_items(got, want, what):
    """got: (records, counts, slots) of a batch form; want: per item (records[:count], count, slots)"""
    rec, counts, slots = got
    assert len(counts) == len(want), what
    for k, (wrec, wcount, wslots) in enumerate(want):
        assert int(counts[k]) == wcount, f"{what}: item {k} count {int(counts[k])} != {wcount}"
        np.testing.assert_array_equal(_bits(rec[k][:wcount]), _bits(wrec), err_msg=f"{what}: item {k} record bits")
        if slots is not None:
            np.testing.assert_array_equal(slots[k], wslots, err_msg=f"{what}: item {k} slots")


def _restated(spec, params, ref_mode=0):
    return [(e["records"], int(e["count"]), e["slots"]) for e in bc.expect(spec, params, ref_mode)]


# ------------------------------------------------------------------------------------------------ 1, 2: chain and key mode against the restatement
@pytest.mark.parametrize("params", bc.SMALL_SETS, ids=[str(i) for i in range(len(bc.SMALL_SETS))])
def test_batch_forms_match_the_restatement(ctx, params):
    fr = bc.sequence(bc.SMALL)
    want = _restated(bc.SMALL, params)
    assert tuple(w[1] for w in want) == bc.SMALL_KEPT[params]
    L, w, K = _set(ctx, params)
    try:
        _check_items(_batch_dev(ctx, fr, 0, L, w, K), want, f"dev {params}")
        _check_items(ctx.klt_flow_batch(fr, L, w, K, want_slots=True), want, f"host {params}")
        rec, counts, untouched = _batch_dev(ctx, fr, 0, L, w, K, want_slots=False)        # d_out_slots NULL: records and counts alone
        assert (untouched == GUARD_WORD).all()
        _check_items((rec, counts, None), want, f"dev, no slots {params}")
        _check_items(ctx.klt_flow_batch(fr, L, w, K) + (None,), want, f"host, no slots {params}")
    finally:
        ctx.set_klt()


@pytest.mark.parametrize("params", bc.KEY_SETS, ids=["0", "1"])
def test_key_mode_pairs_every_frame_with_frame_0(ctx, params):
    fr = bc.sequence(bc.SMALL)
    want = _restated(bc.SMALL, params, 1)
    L, w, K = _set(ctx, params)
    try:
        _check_items(_batch_dev(ctx, fr, 1, L, w, K), want, f"dev key {params}")
        _check_items(ctx.klt_flow_batch(fr, L, w, K, ref_mode=1, want_slots=True), want, f"host key {params}")
    finally:
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ 3: padded rows, frames further apart
@pytest.mark.parametrize("pad", [12, 13])
def test_padded_rows_and_a_larger_frame_pitch(ctx, pad):
    params = bc.SMALL_SETS[0]
    view = bc.padded_sequence(bc.SMALL, pad, 3)
    assert view.strides == ((96 + 3) * (128 + pad), 128 + pad, 1)
    L, w, K = _set(ctx, params)
    try:
        for ref_mode in (0, 1):
            want = _restated(bc.SMALL, params, ref_mode)
            _check_items(_batch_dev(ctx, view, ref_mode, L, w, K), want, f"dev pad {pad} ref_mode {ref_mode}")
            _check_items(ctx.klt_flow_batch(view, L, w, K, ref_mode=ref_mode, want_slots=True), want, f"host pad {pad} ref_mode {ref_mode}")
    finally:
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ 4: more than one round of the segmented compaction
def test_second_compaction_round(ctx):
    fr = bc.sequence(bc.BIG)
    try:
        L, w, K = _set(ctx, bc.BIG_SETS[0])
        assert ctx.klt_slot_count(384, 224) == 1344
        _check_items(_batch_dev(ctx, fr, 0, L, w, K), _restated(bc.BIG, bc.BIG_SETS[0]), "big, restatement")
        L, w, K = _set(ctx, bc.BIG_SETS[1])
        want = _pairs_dev(ctx, fr, 0, L, w, K)
        assert tuple(x[1] for x in want) == bc.BIG_KEPT[bc.BIG_SETS[1]]
        _check_items(_batch_dev(ctx, fr, 0, L, w, K), want, "big, one-pair form")
    finally:
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ 5: the smallest batch and a large one
def test_two_frames_equal_the_one_pair_call(ctx):
    fr = bc.sequence(bc.SMALL)[:2]
    L, w, K = _set(ctx, kc.DEFAULT_SET)
    ent, slots = ctx.klt_flow(fr[0], fr[1], L, w, K, want_slots=True)
    _check_items(ctx.klt_flow_batch(fr, L, w, K, want_slots=True), [(ent, len(ent), slots)], "n_frames 2")


def test_a_720p_batch_at_cell_8_equals_the_one_pair_form(ctx):
    from ofps_amd import synth
    fr = synth.luma_sequence(3, 1280, 720, 3)
    try:
        ctx.set_klt(8)
        assert ctx.klt_slot_count(1280, 720) == 14400
        for ref_mode in (0, 1):
            want = _pairs_dev(ctx, fr, ref_mode, 3, 4, 5)
            assert all(x[1] > 10000 for x in want)
            _check_items(_batch_dev(ctx, fr, ref_mode, 3, 4, 5), want, f"720p ref_mode {ref_mode}")
    finally:
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ 6: the single-context stream
def _single_stream(ctx, frames, L, w, K, **tail):
    """six fused sparse calls of the dense decoders' stream: the reference of the batched stream"""
    ctx.lk_reset()
    return [ctx.lk_push_frame_fused(np.ascontiguousarray(f), L, w, K, sparse=True, seed=SEED + j, **tail) for j, f in enumerate(frames)]


def _batched_stream(ctx, frames, sizes, L, w, K, in_flight=1, entries=True, **tail):
    """-> per frame dict(have_vectors, n_vectors, motion, quat[, islands], entries)"""
    n, H, W = frames.shape
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
    ctx.reset_frames()
    ns = ctx.batch_record_capacity(W, H)
    out, pending, start = [], [], 0
    def collect():
        t, ent, _ = pending.pop(0)             # (the third entry kept the ticket's frames alive until here)
        for j, r in enumerate(ctx.frames_wait(t)):
            r["entries"] = ent[j][:r["n_vectors"]].copy() if ent is not None else None
            out.append(r)
    for size in sizes:
        batch = np.ascontiguousarray(frames[start:start + size])
        ent = np.zeros((size, ns, 4), np.float32) if entries else None
        if len(pending) >= in_flight:
            collect()
        pending.append((ctx.push_frames_async(batch, seed=SEED + start, out_entries=ent, **tail), ent, batch))
        start += size
    while pending:
        collect()
    ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)
    return out


def _same_stream(got, want, what, entries=True):
    assert len(got) == len(want)
    for j, (g, s) in enumerate(zip(got, want)):
        where = f"{what}: frame {j}"
        assert g["have_vectors"] == s["have_vectors"], where
        assert g["n_vectors"] == s["n_vectors"], where
        if not s["have_vectors"]:
            continue
        if entries:
            np.testing.assert_array_equal(_bits(g["entries"]), _bits(s["entries"][:s["n_vectors"]]), err_msg=where + " record bits")
        assert (g["motion"] is None) == (s["motion"] is None), where
        if s["motion"] is not None:
            assert g["motion"][0] == s["motion"][0], where + " island area"
        print(where, "quaternion difference", float(np.abs(g["quat"] - s["quat"]).max()))
        assert np.abs(g["quat"] - s["quat"]).max() <= QUAT_BOUND, where
        if "islands" in s:
            gi, si = g["islands"], s["islands"]
            assert (gi["n_islands"], gi["n_components"], gi["dim"], gi["n_listed"]) == (si["n_islands"], si["n_components"], si["dim"], si["n_listed"]), where
            np.testing.assert_array_equal(gi["table"], si["table"], err_msg=where + " islands table")
            np.testing.assert_array_equal(gi["labels"], si["labels"], err_msg=where + " island labels")


@pytest.mark.parametrize("ransac", [False, True], ids=["lsq", "ransac"])
@pytest.mark.parametrize("sizes", [(3, 3), (1, 2, 3)], ids=["3+3", "1+2+3"])
def test_batched_stream_equals_six_fused_sparse_calls(ctx, sizes, ransac):
    fr = bc.sequence(bc.SMALL)
    L, w, K = _set(ctx, kc.DEFAULT_SET)
    tail = dict(use_ransac=ransac, target_motion=0.003)
    want = _single_stream(ctx, fr, L, w, K, **tail)
    assert [s["n_vectors"] for s in want[1:]] == list(bc.SMALL_KEPT[kc.DEFAULT_SET]) and not want[0]["have_vectors"]
    _same_stream(_batched_stream(ctx, fr, sizes, L, w, K, **tail), want, f"{sizes}")


def test_two_tickets_in_flight_and_no_record_buffer(ctx):
    fr = bc.sequence(bc.SMALL)
    L, w, K = _set(ctx, kc.DEFAULT_SET)
    want = _single_stream(ctx, fr, L, w, K)
    _same_stream(_batched_stream(ctx, fr, (3, 3), L, w, K, in_flight=2), want, "two tickets")
    _same_stream(_batched_stream(ctx, fr, (3, 3), L, w, K, in_flight=2, entries=False), want, "out_entries NULL", entries=False)


def test_stream_lists_islands_and_compensates(ctx):
    fr = bc.sequence(bc.SMALL)
    L, w, K = _set(ctx, kc.DEFAULT_SET)
    try:
        ctx.set_detect_islands(4)
        want = _single_stream(ctx, fr, L, w, K, target_motion=0.0005)
        assert all("islands" in s for s in want[1:])
        _same_stream(_batched_stream(ctx, fr, (3, 3), L, w, K, target_motion=0.0005), want, "islands K = 4")
        ctx.set_detect_islands(0)
        ctx.set_detect_compensation(1)
        want = _single_stream(ctx, fr, L, w, K, target_motion=0.0005)
        _same_stream(_batched_stream(ctx, fr, (1, 2, 3), L, w, K, target_motion=0.0005), want, "compensation mode 1")
    finally:
        ctx.set_detect_islands(0)
        ctx.set_detect_compensation(0)


@pytest.mark.parametrize("params", [bc.ALL_FLAT, bc.FEW], ids=["all-flat", "few"])
def test_stream_items_with_too_few_records(ctx, params):
    fr = bc.sequence(bc.SMALL)
    L, w, K = _set(ctx, params)
    try:
        want = _single_stream(ctx, fr, L, w, K)
        got = _batched_stream(ctx, fr, (3, 3), L, w, K)
        _same_stream(got, want, f"{params}")
        assert [g["n_vectors"] for g in got[1:]] == list(bc.SMALL_KEPT[params])
        if params == bc.ALL_FLAT:
            for g in got[1:]:
                assert g["have_vectors"] and g["n_vectors"] == 0 and g["motion"] is None
                np.testing.assert_array_equal(g["quat"], IDENTITY)
    finally:
        ctx.set_klt()


def test_geometry_change_restarts_the_stream(ctx):
    fr = bc.sequence(bc.SMALL)
    other = np.stack(kc.warp_pair(96, 64, (1.3, -0.6)))
    L, w, K = _set(ctx, kc.PARAM_SETS[0])
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
    try:
        ctx.reset_frames()
        a = ctx.frames_wait(ctx.push_frames_async(np.ascontiguousarray(fr[:3])))
        ent = np.zeros((2, ctx.batch_record_capacity(96, 64), 4), np.float32)
        b = ctx.frames_wait(ctx.push_frames_async(other, out_entries=ent))
        assert [r["have_vectors"] for r in a] == [False, True, True] and [r["have_vectors"] for r in b] == [False, True]
        assert [r["n_vectors"] for r in a[1:]] == list(bc.SMALL_KEPT[kc.PARAM_SETS[0]][:2])
        one = ctx.klt_flow(other[0], other[1], L, w, K)
        assert b[1]["n_vectors"] == len(one)
        np.testing.assert_array_equal(_bits(ent[1][:len(one)]), _bits(one))
        ctx.reset_frames()
        c = ctx.frames_wait(ctx.push_frames_async(other))
        assert [r["have_vectors"] for r in c] == [False, True]
    finally:
        ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)


# ------------------------------------------------------------------------------------------------ 7: refusals, each followed by a valid call
def test_refusals(ctx):
    fr = bc.sequence(bc.SMALL)
    params = kc.PARAM_SETS[0]
    want = _restated(bc.SMALL, params)
    L, w, K = _set(ctx, params)

    def valid():
        _check_items(ctx.klt_flow_batch(fr, L, w, K, want_slots=True), want, "valid call behind a refusal")

    def refused(call):
        with pytest.raises(OfpsHipError) as e:
            call()
        assert e.value.code == EINVAL
        valid()

    refused(lambda: ctx.klt_flow_batch(fr, 5, w, K))                                      # 96 >> 4 = 6 < 8
    with pytest.raises(OfpsHipError) as e:
        ctx.set_klt(12)
    assert e.value.code == EINVAL
    valid()
    refused(lambda: ctx.klt_flow_batch(fr, L, w, K, ref_mode=2))
    refused(lambda: ctx.klt_flow_batch(fr[:1], L, w, K))                                  # one frame is no pair
    d, stride, pitch = _upload(ctx, fr)
    b_rec, b_cnt = _DevBuf(ctx, 4 * 5 * 48), _DevBuf(ctx, 5)
    try:
        for bad in (dict(pitch=pitch - 1), dict(ref_mode=2), dict(L=5)):
            with pytest.raises(OfpsHipError) as e:
                ctx.klt_flow_batch_dev(d, 6, 128, 96, stride, bad.get("pitch", pitch), bad.get("ref_mode", 0), bad.get("L", L), w, K, b_rec.ptr, b_cnt.ptr)
            assert e.value.code == EINVAL, bad
        ctx.sync()
        assert (b_cnt.read(np.uint32) == GUARD_WORD).all(), "a refused call wrote counts"
        ctx.klt_flow_batch_dev(d, 6, 128, 96, stride, pitch, 0, L, w, K, b_rec.ptr, b_cnt.ptr)
        ctx.sync()
        assert tuple(b_cnt.read(np.uint32).tolist()) == bc.SMALL_KEPT[params]
    finally:
        b_rec.free(); b_cnt.free(); ctx.free(d)
    # the stream: settings the frame has no room for are refused at the push, before the upload; the decoder's own ranges at the setter
    for bad in ((2, 5, 7, 10), (1, 0, 7, 10), (1, 7, 7, 10), (1, 4, 8, 10), (1, 4, 7, 31)):
        with pytest.raises(OfpsHipError) as e:
            ctx.set_batch_decoder(*bad)
        assert e.value.code == EINVAL, bad
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, 5, w, K)
    try:
        ctx.reset_frames()
        with pytest.raises(OfpsHipError) as e:
            ctx.push_frames_async(np.ascontiguousarray(fr[:3]))
        assert e.value.code == EINVAL
        ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, w, K)
        res = ctx.frames_wait(ctx.push_frames_async(np.ascontiguousarray(fr[:3])))
        assert [r["n_vectors"] for r in res[1:]] == list(bc.SMALL_KEPT[params][:2])
    finally:
        ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)
        ctx.set_klt()


# ------------------------------------------------------------------------------------------------ 8: the switch back at SAD
def _sad_stream(c, fr):
    c.reset_frames()
    out = []
    for a in (0, 3):
        ent = np.zeros((3, 48, 4), np.float32)
        res = c.frames_wait(c.push_frames_async(np.ascontiguousarray(fr[a:a + 3]), seed=SEED + a, out_entries=ent))
        out.append((ent.tobytes(), [(r["have_vectors"], r["n_vectors"], r["motion"], r["quat"].tobytes()) for r in res]))
    return out


def test_decoder_back_at_sad_equals_a_fresh_context(ctx):
    from ofps_amd.runtime import HipContext
    fr = bc.sequence(bc.SMALL)
    L, w, K = _set(ctx, kc.DEFAULT_SET)
    _batched_stream(ctx, fr, (3, 3), L, w, K)                 # (leaves the decoder at SAD)
    assert ctx.get_batch_decoder()["decoder"] == ctx.BATCH_DECODER_SAD
    fresh = HipContext(0)
    try:
        assert fresh.get_batch_decoder() == dict(decoder=0, levels=4, radius=7, iters=10)
        assert _sad_stream(ctx, fr) == _sad_stream(fresh, fr)
    finally:
        fresh.close()
    prev, cur = kc.warp_pair(96, 64, (1.3, -0.6))
    for params in kc.PARAM_SETS:
        cell, r, min_score, min_eig, R, L, w, K = params
        exp = ik.flow(prev, cur, L, w, K, cell, r, min_score, min_eig, R)
        _set(ctx, params)
        ent, slots = ctx.klt_flow(prev, cur, L, w, K, want_slots=True)
        np.testing.assert_array_equal(slots, exp["slots"])
        np.testing.assert_array_equal(_bits(ent), _bits(exp["records"]))
    ctx.set_klt()


# ------------------------------------------------------------------------------------------------ 9: options
OPTION_CASES = [("OFPS_HIP_KLT_CELL", "cell", 32, ("12", "0")), ("OFPS_HIP_KLT_SCORE_RADIUS", "score_radius", 3, ("0", "4")),
                ("OFPS_HIP_KLT_MIN_SCORE", "min_score", 500, ("0", "-3")), ("OFPS_HIP_KLT_MIN_EIG", "min_eig", 77, ("0", "65536")),
                ("OFPS_HIP_KLT_MAX_RESIDUAL", "max_residual", 160, ("-1", "4081")), ("OFPS_HIP_BATCH_DECODER", "decoder", 1, ("2", "-1")),
                ("OFPS_HIP_KLT_LEVELS", "levels", 3, ("0", "7")), ("OFPS_HIP_KLT_RADIUS", "radius", 5, ("0", "8")),
                ("OFPS_HIP_KLT_ITERS", "iters", 12, ("0", "31"))]


def _settings(c):
    return {**c.get_klt(), **c.get_batch_decoder()}


def test_options_set_the_fields_the_getters_read(ctx):
    dflt = _settings(ctx)
    assert dflt == dict(cell=16, score_radius=2, min_score=1, min_eig=1, max_residual=0, decoder=0, levels=4, radius=7, iters=10)
    for name, key, value, bad in OPTION_CASES:
        ctx.set_option(name, value)
        assert _settings(ctx) == {**dflt, key: value}, name
        for b in bad:
            with pytest.raises(OfpsHipError) as e:
                ctx.set_option(name, b)
            assert e.value.code == EINVAL, (name, b)
            assert _settings(ctx)[key] == value, (name, b)
        ctx.set_option(name, None)
        assert _settings(ctx) == dflt, name


def test_environment_variables_are_read_at_init():
    env = dict(os.environ, **{name: str(value) for name, _, value, _ in OPTION_CASES})
    code = ("import json, sys; sys.path.insert(0, %r); from ofps_amd.runtime import HipContext; c = HipContext(0); "
            "print(json.dumps({**c.get_klt(), **c.get_batch_decoder()})); c.close()" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {key: value for _, key, value, _ in OPTION_CASES}


# ------------------------------------------------------------------------------------------------ 10: the multi-device workers
@pytest.mark.parametrize("ransac", [False, True], ids=["lsq", "ransac"])
def test_multi_device_workers_take_the_decoder_from_the_environment(ctx, ransac):
    params = kc.PARAM_SETS[0]
    cell, r, min_score, min_eig, R, L, w, K = params
    env = dict(os.environ, OFPS_HIP_BATCH_DECODER="1", OFPS_HIP_KLT_CELL=str(cell), OFPS_HIP_KLT_SCORE_RADIUS=str(r), OFPS_HIP_KLT_MIN_SCORE=str(min_score),
               OFPS_HIP_KLT_MIN_EIG=str(min_eig), OFPS_HIP_KLT_MAX_RESIDUAL=str(R), OFPS_HIP_KLT_LEVELS=str(L), OFPS_HIP_KLT_RADIUS=str(w),
               OFPS_HIP_KLT_ITERS=str(K), KLT_CHILD_SEED=str(SEED), KLT_CHILD_RANSAC="1" if ransac else "0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_klt_child.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["capacity"] == 48
    _set(ctx, params)
    try:
        want = _batched_stream(ctx, bc.sequence(bc.SMALL), (3, 3), L, w, K, use_ransac=ransac)
    finally:
        ctx.set_klt()
    got = child["frames"]
    assert [g["have_vectors"] for g in got] == [False] + [True] * 5
    assert [g["n_vectors"] for g in got[1:]] == list(bc.SMALL_KEPT[params])
    for k in range(1, 6):
        assert got[k]["n_vectors"] == want[k]["n_vectors"], k
        assert got[k]["entries"] == _bits(want[k]["entries"]).reshape(-1).tolist(), k
        assert got[k]["quat"] == _bits(want[k]["quat"]).tolist(), k
        assert got[k]["motion"] == (list(want[k]["motion"]) if want[k]["motion"] is not None else None), k


# ------------------------------------------------------------------------------------------------ 11: the C++ host tool
def test_host_tool_batched_stream_with_klt():
    from ofps_amd import build as hip_build
    tool = os.path.join(os.path.dirname(hip_build.__file__), "host", "ofps_hip_tool")
    if not os.path.exists(tool):
        hip_build.build_host()
    out = subprocess.run([tool, "stream-bench", "128", "96", "12", "batch", "3", "--klt"], check=True, capture_output=True, text=True, timeout=120).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r["mode"] == "read_ahead_batched" and r["decoder"] == "hip_klt" and r["batch"] == 3
    assert r["capacity"] == 48 and 0 < r["last_n_vectors"] <= 48
    out = subprocess.run([tool, "stream-bench", "128", "96", "12", "multi", "3", "0", "0", "--klt"], check=True, capture_output=True, text=True,
                         timeout=120).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r["mode"] == "multi_read_ahead_batched" and r["decoder"] == "hip_klt" and r["workers"] == 2
    assert r["capacity"] == 48 and 0 < r["last_n_vectors"] <= 48
