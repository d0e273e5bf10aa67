"""-m gpu: gate, consistency check and median test in the batched forms (include/ofps_hip.h N1b) on the cases of
tests/sad_batch_filter_cases.py.  Three references, none of them the code under test:
  the restatements (tests/sad_gate_cases.py, tests/sad_consistency_cases.py, tests/indep_sad_median.py on the CPU oracle's search);
  the one-pair device forms (ofps_hip_sad_flow_gated_dev / _checked_dev / _median_dev), item by item, bit for bit;
  n single ofps_hip_push_frame calls with the same settings for the batched stream: counts, records and island bit for bit, the
  quaternion to the 2e-6 the header states for batch against single.
Records, triples, counts and flags are integers or copies: every equality but the quaternion's is bit for bit.
tests/test_sad_batch_filter_cpu.py proves on the restatements that these inputs separate the items and the criteria."""
import numpy as np
import pytest

import sad_batch_filter_cases as bc
import sad_consistency_cases as cc
import sad_gate_cases as gc

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1, 0, 0, 0], np.float32)
EINVAL = -1
QUAT_BOUND = 2e-6                                        # include/ofps_hip.h: batch against single
GUARD = 64
CRIT_IDS = [bc.criteria_id(c) for c in bc.CRITERIA]
ALL3 = (bc.GATE, bc.LIMIT, bc.MEDIAN)


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
    DEFAULT = dict(median=0, limit=0, gate=0, scale=1, levels=1, predictors=0, prefilter=0, pruned=False, batch_filter=0, compensate=0)

    def __init__(self, ctx, **kw):
        self.ctx, self.v = ctx, dict(self.DEFAULT, **kw)

    def _apply(self, v):
        c = self.ctx
        c.set_sad_median(v["median"]); c.set_sad_consistency(v["limit"]); c.set_sad_gate(v["gate"]); c.set_sad_motion_scale(v["scale"])
        c.set_sad_levels(v["levels"]); c.set_sad_predictors(v["predictors"]); c.set_sad_prefilter(v["prefilter"])
        c.set_sad_mode(c.SAD_PRUNED if v["pruned"] else c.SAD_EXHAUSTIVE)
        c.set_sad_batch_filter(v["batch_filter"]); c.set_detect_compensation(v["compensate"])

    def __enter__(self):
        self._apply(self.v)

    def __exit__(self, *exc):
        self._apply(self.DEFAULT)


# --------------------------------------------------------------------------------------------------------------- the device form
def _filtered_dev(ctx, frames, ref_mode, B, R, crit, want_best=True, stride=None, pitch=None):
    """ofps_hip_sad_flow_filtered_dev on `frames` -> [(records[:n], triples[:n] or None, n)] per pair; 64 guard words behind each output"""
    import torch
    n_frames, H, W = frames.shape
    stride = W if stride is None else stride
    pitch = stride * H if pitch is None else pitch
    host = np.full((n_frames, pitch), 0xA5, np.uint8)                                   # padding bytes that are no frame's pixels
    for k in range(n_frames):
        host[k, :stride * H].reshape(H, stride)[:, :W] = frames[k]
    pairs, nblk = n_frames - 1, (W // B) * (H // B)
    d_frames = torch.from_numpy(host).cuda()
    d_ent = torch.full((pairs * nblk * 4 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    d_best = torch.full((pairs * nblk * 3 + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((pairs + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_flow_filtered_dev(d_frames.data_ptr(), n_frames, W, H, stride, pitch, ref_mode, B, R, crit[0], crit[1], crit[2], d_ent.data_ptr(),
                              d_best.data_ptr() if want_best else None, d_cnt.data_ptr())
    ctx.sync()
    ent, best, cnt = d_ent.cpu().numpy(), d_best.cpu().numpy(), d_cnt.cpu().numpy()
    assert (ent[pairs * nblk * 4:] == -7.0).all() and (best[pairs * nblk * 3:] == -7).all() and (cnt[pairs:] == -7).all(), "guard words"
    if not want_best:
        assert (best == -7).all(), "d_out_best NULL: nothing may be written"
    ent, best = ent[:pairs * nblk * 4].reshape(pairs, nblk, 4), best[:pairs * nblk * 3].reshape(pairs, nblk, 3)
    out = []
    for k in range(pairs):
        n = int(cnt[k])
        assert 0 <= n <= nblk, (k, n)
        out.append((ent[k, :n].copy(), best[k, :n].copy() if want_best else None, n))
    return out


def _one_pair_dev(ctx, prev, cur, B, R, crit):
    """the one-pair device form the definition names, with the same three values -> (records[:n], triples[:n], n)"""
    import torch
    H, W = prev.shape
    nblk = (W // B) * (H // B)
    d_prev, d_cur = torch.from_numpy(np.array(prev)).cuda(), torch.from_numpy(np.array(cur)).cuda()
    d_ent = torch.zeros((nblk, 4), dtype=torch.float32, device="cuda")
    d_best = torch.zeros((nblk, 3), dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gate, limit, median = crit
    a = (d_prev.data_ptr(), d_cur.data_ptr(), W, H, W, B, R)
    o = (d_ent.data_ptr(), d_best.data_ptr(), d_cnt.data_ptr())
    if median:
        ctx.sad_flow_median_dev(*a, gate, limit, median, *o)
    elif limit:
        ctx.sad_flow_checked_dev(*a, gate, limit, *o)
    else:
        ctx.sad_flow_gated_dev(*a, gate, *o)
    ctx.sync()
    n = int(d_cnt.cpu().numpy()[0])
    return d_ent.cpu().numpy()[:n], d_best.cpu().numpy()[:n], n


def _check_against_restatement(got, frames, ref_mode, B, R, crit, what):
    for k, ((p, c), (ent, best, n)) in enumerate(zip(bc.pairs_of(frames, ref_mode), got)):
        ent0, F = bc.vectors(p, c, B, R)
        keep = bc.keep_of(p, c, B, R, *crit)
        w = f"{what} item {k}"
        assert n == int(keep.sum()), w
        np.testing.assert_array_equal(_bits(ent), _bits(ent0[keep]), err_msg=w + ": records")
        if best is not None:
            np.testing.assert_array_equal(best, F[keep], err_msg=w + ": triples")


def _check_against_one_pair(ctx, got, frames, ref_mode, B, R, crit, what):
    for k, ((p, c), (ent, best, n)) in enumerate(zip(bc.pairs_of(frames, ref_mode), got)):
        e1, b1, n1 = _one_pair_dev(ctx, p, c, B, R, crit)
        w = f"{what} item {k}"
        assert n == n1, w
        np.testing.assert_array_equal(_bits(ent), _bits(e1), err_msg=w + ": records")
        if best is not None:
            np.testing.assert_array_equal(best, b1, err_msg=w + ": triples")


@pytest.mark.parametrize("ref_mode", (0, 1))
@pytest.mark.parametrize("crit", bc.CRITERIA, ids=CRIT_IDS)
def test_filtered_dev_against_restatement_and_one_pair_form(ctx, crit, ref_mode):
    """gc.frames(): 320 x 192, block 16, range 8, 3 pairs; d_out_best given and NULL; a padded stride with frame_pitch > stride * H"""
    f = gc.frames()
    what = f"{bc.criteria_id(crit)} ref_mode {ref_mode}"
    got = _filtered_dev(ctx, f, ref_mode, gc.BLOCK, gc.RANGE, crit)
    _check_against_restatement(got, f, ref_mode, gc.BLOCK, gc.RANGE, crit, what)
    _check_against_one_pair(ctx, got, f, ref_mode, gc.BLOCK, gc.RANGE, crit, what)
    if not ref_mode and crit == (0, bc.LIMIT, 0):
        assert [n for _, _, n in got] == [cc.FRAMES_KEPT[k] for k in (1, 2, 3)]
    no_best = _filtered_dev(ctx, f, ref_mode, gc.BLOCK, gc.RANGE, crit, want_best=False)
    padded = _filtered_dev(ctx, f, ref_mode, gc.BLOCK, gc.RANGE, crit, stride=gc.FRAME_W + 64, pitch=(gc.FRAME_W + 64) * gc.FRAME_H + 4096)
    for k in range(3):
        assert no_best[k][2] == padded[k][2] == got[k][2]
        np.testing.assert_array_equal(_bits(no_best[k][0]), _bits(got[k][0]), err_msg=f"{what} item {k}: records without d_out_best")
        np.testing.assert_array_equal(_bits(padded[k][0]), _bits(got[k][0]), err_msg=f"{what} item {k}: records, padded frames")
        np.testing.assert_array_equal(padded[k][1], got[k][1], err_msg=f"{what} item {k}: triples, padded frames")


def test_filtered_dev_with_two_frames_is_the_one_pair_form(ctx):
    f = gc.frames()[:2]
    got = _filtered_dev(ctx, f, 0, gc.BLOCK, gc.RANGE, ALL3)
    _check_against_restatement(got, f, 0, gc.BLOCK, gc.RANGE, ALL3, "two frames")
    _check_against_one_pair(ctx, got, f, 0, gc.BLOCK, gc.RANGE, ALL3, "two frames")


MODES = {  # settings of the search, range
    "scale4": (dict(scale=4), gc.RANGE),
    "levels2-predictors": (dict(levels=2, predictors=1), gc.RANGE),
    "prefilter4": (dict(prefilter=4), gc.RANGE),
    "pruned": (dict(pruned=True), 16),                   # the pruned kernel's geometry: block 16, range 16
    "scale4-levels2": (dict(scale=4, levels=2), gc.RANGE),
    # mean removal's output is itself a pair of frame sets the level loop lays out (tests/test_sad_batch_filter_cpu.py: the kept counts)
    "prefilter4-levels2": (dict(prefilter=4, levels=2), gc.RANGE),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_composition_through_the_context(ctx, mode):
    """everything else of the context applies as to any search: item by item against the one-pair call in the same mode, both ref_modes"""
    kw, R = MODES[mode]
    f = gc.frames()
    with _settings(ctx, **kw):
        for ref_mode in (0, 1):
            got = _filtered_dev(ctx, f, ref_mode, gc.BLOCK, R, ALL3)
            _check_against_one_pair(ctx, got, f, ref_mode, gc.BLOCK, R, ALL3, f"{mode} ref_mode {ref_mode}")
            assert all(0 < n < gc.NBLK for _, _, n in got)
        got = _filtered_dev(ctx, f, 0, gc.BLOCK, R, (0, 0, bc.MEDIAN))
        _check_against_one_pair(ctx, got, f, 0, gc.BLOCK, R, (0, 0, bc.MEDIAN), f"{mode} median alone")
        if kw.get("scale") == 4:                         # the triples are the quarter-pel ones, the verdicts the integer winners'
            with _settings(ctx, **dict(kw, scale=1)):
                integer = _filtered_dev(ctx, f, 0, gc.BLOCK, R, (0, 0, bc.MEDIAN))
            assert [n for _, _, n in integer] == [n for _, _, n in got]
            assert any(not np.array_equal(a[1], b[1]) for a, b in zip(integer, got))


@pytest.mark.parametrize("crit", bc.CRITERIA, ids=CRIT_IDS)
def test_compaction_over_scan_rounds(ctx, crit):
    """41 x 33 = 1,353 blocks: two scan rounds, the second partial, no multiple of 64; every item another count under every combination.
    The batched compaction has one path for every nblk."""
    f = bc.scan_frames()
    got = _filtered_dev(ctx, f, 0, bc.SCAN_B, bc.SCAN_R, crit)
    _check_against_restatement(got, f, 0, bc.SCAN_B, bc.SCAN_R, crit, bc.criteria_id(crit))
    assert len({n for _, _, n in got}) == len(got)


def test_compaction_over_four_scan_rounds(ctx):
    """63 x 49 = 3,087 blocks: four rounds, the last partial"""
    f = bc.scan3_frames()
    for crit in (ALL3, (bc.GATE, 0, 0)):
        got = _filtered_dev(ctx, f, 0, bc.SCAN_B, bc.SCAN_R, crit)
        _check_against_restatement(got, f, 0, bc.SCAN_B, bc.SCAN_R, crit, bc.criteria_id(crit))
        _check_against_one_pair(ctx, got, f, 0, bc.SCAN_B, bc.SCAN_R, crit, bc.criteria_id(crit))


def test_mixed_batch_with_none_two_some_and_all_kept(ctx):
    f = bc.mixed_frames()
    crit = (gc.TWO_BLOCK_GATE, 0, 0)
    got = _filtered_dev(ctx, f, 0, gc.BLOCK, gc.RANGE, crit)
    _check_against_restatement(got, f, 0, gc.BLOCK, gc.RANGE, crit, "mixed")
    counts = [n for _, _, n in got]
    assert counts[0] == 0 and counts[1] == bc.MIXED_KEPT_2 and 2 < counts[2] < gc.NBLK and counts[3] == gc.NBLK


def test_errors_are_refused_before_anything_is_enqueued(ctx):
    import torch
    from ofps_amd.runtime import OfpsHipError
    W, H, B, R = 96, 64, 8, 8
    d = torch.zeros(4 * W * H, dtype=torch.int32, device="cuda")                        # real device memory behind every pointer: these calls must
    torch.cuda.synchronize()                                                            # be refused before anything is enqueued, but are not trusted to
    p = d.data_ptr()
    ok = dict(d_frames=p, n_frames=3, W=W, H=H, stride=W, frame_pitch=W * H, ref_mode=0, block=B, search_range=R, min_pixels=1, limit=1, median=2,
              d_out_entries=p, d_out_best=None, d_out_counts=p)
    bad = [dict(min_pixels=0, limit=0, median=0),        # all three criteria off
           dict(min_pixels=B * B + 1), dict(min_pixels=-1), dict(limit=130), dict(limit=-1), dict(median=256), dict(median=-1),
           dict(n_frames=1), dict(n_frames=0), dict(d_out_entries=0), dict(d_out_counts=0), dict(d_frames=0),
           dict(ref_mode=2), dict(frame_pitch=W * H - 1), dict(stride=W - 1), dict(block=65)]
    for kw in bad:
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow_filtered_dev(**dict(ok, **kw))
        assert ei.value.code == EINVAL, kw
    ctx.sync()
    assert (d.cpu().numpy() == 0).all()


def test_setter_getter_and_option(ctx):
    from ofps_amd import _lib
    from ofps_amd.runtime import OfpsHipError
    lib = _lib.load()
    assert ctx.get_sad_batch_filter() == 0
    for bad in (-1, 2, 77):
        assert lib.ofps_hip_set_sad_batch_filter(ctx._h, bad) == EINVAL and ctx.get_sad_batch_filter() == 0
        assert str(bad) in lib.ofps_hip_last_error(ctx._h).decode()                     # the value is in the message
    for ok in (1, 0):
        ctx.set_sad_batch_filter(ok)
        assert ctx.get_sad_batch_filter() == ok
    ctx.set_option("OFPS_HIP_SAD_BATCH_FILTER", 1)        # the option table sets the same field
    assert ctx.get_sad_batch_filter() == 1
    for bad in (-1, 2, "yes"):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_BATCH_FILTER", bad)
        assert ei.value.code == EINVAL and ctx.get_sad_batch_filter() == 1 and str(bad) in str(ei.value)
    ctx.set_option("OFPS_HIP_SAD_BATCH_FILTER", None)
    assert ctx.get_sad_batch_filter() == 0
    assert lib.ofps_hip_get_sad_batch_filter(None) == EINVAL and lib.ofps_hip_set_sad_batch_filter(None, 1) == EINVAL


# --------------------------------------------------------------------------------------------------------------- the batched stream
def _prm(use_ransac, seed, B=gc.BLOCK, R=gc.RANGE, cam=gc.FRAME_CAM, detector=True, estimator=True):
    return dict(block=B, search_range=R, detector=detector, estimator=estimator, aspect=cam[0], fov_y_deg=cam[1], use_ransac=use_ransac, seed=seed,
                **gc.FRAME_DETECTOR, **gc.FRAME_RANSAC)


def _singles(ctx, frames, seeds, use_ransac, **kw):
    """one ofps_hip_push_frame per frame on a fresh single-frame stream, frame j seeded seeds[j]"""
    ctx.reset_frames()
    out = [ctx.push_frame(f, want_entries=True, **_prm(use_ransac, s, **kw)) for f, s in zip(frames, seeds)]
    ctx.reset_frames()
    return out


def _batches(ctx, frames, sizes, seed0s, use_ransac, **kw):
    """`frames` pushed as tickets of `sizes` frames on a fresh batched stream, every ticket pushed before the previous one is collected
    (two in flight) -> per frame dict(have, n, entries, quat, motion)"""
    nblk = (frames.shape[2] // kw.get("B", gc.BLOCK)) * (frames.shape[1] // kw.get("B", gc.BLOCK))
    ctx.reset_frames()
    bufs, ents, tickets, out = [], [], [], []
    at = 0

    def collect(k):
        res = ctx.frames_wait(tickets[k])
        for j, r in enumerate(res):
            n = r["n_vectors"]
            out.append(dict(have=r["have_vectors"], n=n, entries=ents[k][j, :n].copy() if r["have_vectors"] else None, quat=r["quat"], motion=r["motion"]))

    try:
        for k, (size, seed0) in enumerate(zip(sizes, seed0s)):
            if k >= 2:
                collect(k - 2)
            buf = ctx.pinned_array((size,) + frames.shape[1:], np.uint8)
            ent = ctx.pinned_array((size, nblk, 4))
            ent[:] = np.nan
            np.copyto(buf, frames[at:at + size])
            at += size
            bufs.append(buf); ents.append(ent)
            tickets.append(ctx.push_frames_async(buf, out_entries=ent, **_prm(use_ransac, seed0, **kw)))
        for k in range(max(0, len(sizes) - 2), len(sizes)):
            collect(k)
    finally:
        ctx.reset_frames()
        for p in bufs + ents:
            ctx.free_pinned(p)
    return out


def _check_stream(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        m = f"{what} frame {j}"
        assert g["have"] == w["have_vectors"], m
        if not g["have"]:
            assert g["n"] == 0 and g["motion"] is None, m
            np.testing.assert_array_equal(g["quat"], IDENTITY, err_msg=m)
            continue
        assert g["n"] == w["n_vectors"], m
        np.testing.assert_array_equal(_bits(g["entries"]), _bits(w["entries"]), err_msg=m + ": records")
        assert (g["motion"] is None) == (w["motion"] is None), m
        if g["motion"] is not None:
            assert g["motion"][0] == w["motion"][0], m + ": island"
        err = float(np.abs(g["quat"] - w["quat"]).max())
        print(f"{m}: kept {g['n']}, quat {g['quat']} (|batch - single| {err:.3g}), area {gc.area_of(g['motion'])}")
        assert err <= QUAT_BOUND and np.isfinite(g["quat"]).all(), m


def _stream_frames():
    """the 4 frames, then 3 more: ticket 2's item 0 pairs with ticket 1's last frame"""
    f = gc.frames()
    return np.ascontiguousarray(np.concatenate([f, f[2::-1]]))


@pytest.mark.parametrize("use_ransac", (False, True), ids=["lsq", "ransac"])
@pytest.mark.parametrize("crit", bc.CRITERIA, ids=CRIT_IDS)
def test_batched_stream_equals_single_pushes(ctx, crit, use_ransac):
    f = _stream_frames()
    seeds = [gc.SEED + j for j in range(4)] + [gc.SEED + 40 + j for j in range(3)]      # item j of a ticket: seed0 + j
    with _settings(ctx, gate=crit[0], limit=crit[1], median=crit[2], batch_filter=1):
        want = _singles(ctx, f, seeds, use_ransac)
        got = _batches(ctx, f, (4, 3), (gc.SEED, gc.SEED + 40), use_ransac)
    what = f"{bc.criteria_id(crit)} {'ransac' if use_ransac else 'lsq'}"
    _check_stream(got, want, what)
    assert not got[0]["have"] and all(g["have"] for g in got[1:])
    for k in (1, 2, 3):                                  # ... and the restatement's kept sets for the first ticket
        keep = bc.keep_of(f[k - 1], f[k], gc.BLOCK, gc.RANGE, *crit)
        assert got[k]["n"] == int(keep.sum()), what
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(gc.frame_vectors(k)[0][keep]), err_msg=what)
    assert all(0 < g["n"] < gc.NBLK for g in got[1:])


def test_batched_stream_without_detector_and_estimator(ctx):
    """the counts travel in the ticket's block also when no stage asks for a read-back"""
    f = _stream_frames()
    with _settings(ctx, gate=bc.GATE, median=bc.MEDIAN, batch_filter=1):
        got = _batches(ctx, f, (4, 3), (0, 0), False, detector=False, estimator=False)
        want = _singles(ctx, f, [0] * 7, False, detector=False, estimator=False)
    _check_stream(got, want, "records only")


def test_mixed_batch_gives_identity_and_no_motion(ctx):
    f = np.ascontiguousarray(bc.mixed_frames()[:4])                                     # [textured, flat, two-block, textured]
    for use_ransac in (False, True):
        with _settings(ctx, gate=gc.TWO_BLOCK_GATE, batch_filter=1):
            got = _batches(ctx, f, (4,), (gc.SEED,), use_ransac)
            want = _singles(ctx, f, [gc.SEED + j for j in range(4)], use_ransac)
        _check_stream(got, want, "mixed")
        assert [g["n"] for g in got] == [0, 0, bc.MIXED_KEPT_2, int(gc.keep_flags(f[3], gc.BLOCK, gc.TWO_BLOCK_GATE).sum())]
        assert got[1]["have"] and got[1]["motion"] is None                              # none kept: vectors "had", no motion, identity
        np.testing.assert_array_equal(got[1]["quat"], IDENTITY)
        np.testing.assert_array_equal(got[2]["quat"], IDENTITY)                         # fewer than 3 kept: identity with either solver


def test_detect_compensation_mode_1(ctx):
    f = _stream_frames()
    seeds = [gc.SEED + j for j in range(4)] + [gc.SEED + 40 + j for j in range(3)]
    with _settings(ctx, gate=bc.GATE, median=bc.MEDIAN, batch_filter=1, compensate=1):
        want = _singles(ctx, f, seeds, False)
        got = _batches(ctx, f, (4, 3), (gc.SEED, gc.SEED + 40), False)
    _check_stream(got, want, "compensated")
    with _settings(ctx, gate=bc.GATE, median=bc.MEDIAN, batch_filter=1):
        raw = _batches(ctx, f, (4, 3), (gc.SEED, gc.SEED + 40), False)
    assert any(a["motion"] != b["motion"] for a, b in zip(got, raw)), "the detector answered as on the raw vectors"


def test_a_ticket_follows_the_settings_at_its_push(ctx):
    """ticket 1 pushed with the switch on, ticket 2 with it off, both in flight"""
    f = _stream_frames()
    nblk = gc.NBLK
    bufs = [ctx.pinned_array((n, gc.FRAME_H, gc.FRAME_W), np.uint8) for n in (4, 3)]
    ents = [ctx.pinned_array((n, nblk, 4)) for n in (4, 3)]
    np.copyto(bufs[0], f[:4]); np.copyto(bufs[1], f[4:])
    try:
        with _settings(ctx, limit=bc.LIMIT, batch_filter=1):
            ctx.reset_frames()
            t0 = ctx.push_frames_async(bufs[0], out_entries=ents[0], **_prm(False, 1))
            ctx.set_sad_batch_filter(0)
            t1 = ctx.push_frames_async(bufs[1], out_entries=ents[1], **_prm(False, 2))
            r0, r1 = ctx.frames_wait(t0), ctx.frames_wait(t1)
        assert [r["n_vectors"] for r in r0] == [0] + [cc.FRAMES_KEPT[k] for k in (1, 2, 3)]
        assert [r["n_vectors"] for r in r1] == [nblk] * 3
    finally:
        ctx.reset_frames()
        for p in bufs + ents:
            ctx.free_pinned(p)


def test_switch_0_after_switch_1_equals_a_fresh_context(ctx):
    from ofps_amd.runtime import HipContext
    f = _stream_frames()

    def run(c):
        c.set_sad_gate(bc.GATE); c.set_sad_median(bc.MEDIAN)
        try:
            return _batches(c, f, (4, 3), (gc.SEED, gc.SEED + 40), False)
        finally:
            c.set_sad_gate(0); c.set_sad_median(0)

    fresh = HipContext(0)
    try:
        ref = run(fresh)                                 # a context that never saw the switch
    finally:
        fresh.close()
    with _settings(ctx, batch_filter=1):
        on = run(ctx)
    assert ctx.get_sad_batch_filter() == 0
    again = run(ctx)
    assert [g["n"] for g in on[1:]] != [g["n"] for g in again[1:]]
    assert [g["n"] for g in again] == [0] + [gc.NBLK] * 6 == [g["n"] for g in ref]
    for a, r in zip(again[1:], ref[1:]):
        np.testing.assert_array_equal(_bits(a["entries"]), _bits(r["entries"]))
        np.testing.assert_array_equal(_bits(a["quat"]), _bits(r["quat"]))
        assert a["motion"] == r["motion"]


@pytest.mark.parametrize("use_ransac", (False, True), ids=["lsq", "ransac"])
def test_more_than_8192_blocks(ctx, use_ransac):
    """728 x 728, block 8 = 8,281 blocks, a batch of 3 behind a first frame: the estimator's launch-per-step solver with one count per item"""
    f = np.ascontiguousarray(bc.big_frames())
    kw = dict(B=bc.BIG_B, R=bc.BIG_R, cam=bc.BIG_CAM)
    seeds = [7] + [20 + j for j in range(3)]
    with _settings(ctx, gate=bc.GATE, median=bc.MEDIAN, batch_filter=1):
        want = _singles(ctx, f, seeds, use_ransac, **kw)
        got = _batches(ctx, f, (1, 3), (7, 20), use_ransac, **kw)
    _check_stream(got, want, "8281 blocks")
    counts = [g["n"] for g in got[1:]]
    assert counts == [int(bc.keep_of(f[k - 1], f[k], bc.BIG_B, bc.BIG_R, bc.GATE, 0, bc.MEDIAN).sum()) for k in (1, 2, 3)]
    assert len(set(counts)) == 3 and all(np.abs(g["quat"] - IDENTITY).max() > 0 for g in got[1:])


def test_multi_device_follows_the_switch_variable(monkeypatch):
    from ofps_amd.runtime import HipContext, MultiDevice
    f = np.ascontiguousarray(gc.frames())

    def multi():
        m = MultiDevice([0, 0])
        try:
            ent = np.full((4, gc.NBLK, 4), np.nan, np.float32)
            res = m.frames_wait(m.push_frames_async(f, out_entries=ent, **_prm(False, gc.SEED)))
            return res, ent
        finally:
            m.close()

    monkeypatch.setenv("OFPS_HIP_SAD_GATE", str(bc.GATE))                               # the workers read the environment at their own init
    res, ent = multi()                                                                  # without the switch variable: nblk records per frame
    assert [r["n_vectors"] for r in res] == [0] + [gc.NBLK] * 3
    for k in (1, 2, 3):
        np.testing.assert_array_equal(_bits(ent[k]), _bits(gc.frame_vectors(k)[0]))
    monkeypatch.setenv("OFPS_HIP_SAD_BATCH_FILTER", "1")
    res, ent = multi()
    one = HipContext(0)                                                                 # (reads the same environment)
    try:
        assert one.get_sad_batch_filter() == 1 and one.get_sad_gate() == bc.GATE
        want = _batches(one, f, (4,), (gc.SEED,), False)
    finally:
        one.close()
    assert not res[0]["have_vectors"] and res[0]["n_vectors"] == 0
    for k in (1, 2, 3):
        n = res[k]["n_vectors"]
        assert res[k]["have_vectors"] and n == want[k]["n"] == int(gc.frame_keep(k).sum()) < gc.NBLK
        np.testing.assert_array_equal(_bits(ent[k, :n]), _bits(want[k]["entries"]))
        assert res[k]["motion"] == want[k]["motion"]
        assert np.abs(res[k]["quat"] - want[k]["quat"]).max() <= QUAT_BOUND


# ------------------------------------------------------------------------- per-item device counts behind the densifier's two-pass sort
# 17 x 17 and 23 x 23 detector fields: more than 256 cells, so the densifier behind the batched tail is the general path with two digits,
# one launch over all items of the ticket, each item's count read from device memory.  (The other batched stream tests use gc.FRAME_DETECTOR:
# 9 x 9, the one-workgroup densifier.)
FINE_DETECTORS = {"side17": (dict(min_size=0.014, subdivide=2, target_motion=0.003), 17, (None, None, 9, 172)),
                  "side23": (dict(min_size=0.05, subdivide=5, target_motion=0.003), 23, (None, None, None, 191))}


@pytest.mark.parametrize("use_ransac", (False, True), ids=["lsq", "ransac"])
@pytest.mark.parametrize("detector", list(FINE_DETECTORS))
def test_batched_stream_with_device_counts_and_a_two_pass_detector_sort(ctx, monkeypatch, detector, use_ransac):
    """bc.mixed_frames() as ONE ticket of five under the gate that keeps none, two, some and all blocks: records, counts and island of the
    batched push against five single pushes, bit for bit, and the island against the oracle on the kept records.  The batched form returns
    the island's area and side only (ofps_hip_frame_result); the island FIELD is compared where the library returns one: the single push
    against the oracle."""
    import oracle
    det, side, areas = FINE_DETECTORS[detector]
    assert oracle.block_dim(det["min_size"], det["subdivide"]) == side and side * side > 256
    monkeypatch.setattr(gc, "FRAME_DETECTOR", det)       # _prm reads it at every call
    f = np.ascontiguousarray(bc.mixed_frames())
    seeds = [gc.SEED + j for j in range(len(f))]
    with _settings(ctx, gate=gc.TWO_BLOCK_GATE, batch_filter=1):
        ctx.reset_frames()
        want = [ctx.push_frame(fr, want_entries=True, want_field=True, **_prm(use_ransac, s)) for fr, s in zip(f, seeds)]
        ctx.reset_frames()
    # the same ticket unfiltered first: it leaves a whole sort of nblk records behind in every item's segment of the sorting scratch, so a stage
    # that looked past an item's count would find well-formed keys of another frame there, not (perhaps) zeros
    full = _batches(ctx, f, (len(f),), (gc.SEED,), use_ransac)
    with _settings(ctx, gate=gc.TWO_BLOCK_GATE, batch_filter=1):
        got = _batches(ctx, f, (len(f),), (gc.SEED,), use_ransac)
    what = f"{detector} {'ransac' if use_ransac else 'lsq'}"
    _check_stream(got, [dict(w, motion=None if w["motion"] is None else (w["motion"][0], side)) for w in want], what)
    assert not got[0]["have"] and [g["n"] for g in got[1:]] == [0, bc.MIXED_KEPT_2, 144, gc.NBLK]
    for k in range(1, len(f)):
        m = f"{what} frame {k}"
        isl = oracle.detect_motion(bc.vectors(f[k - 1], f[k], gc.BLOCK, gc.RANGE)[0], **det)
        assert full[k]["n"] == gc.NBLK and full[k]["motion"] == (None if isl is None else (isl[0], side)), m + ": unfiltered"
        keep = bc.keep_of(f[k - 1], f[k], gc.BLOCK, gc.RANGE, gc.TWO_BLOCK_GATE, 0, 0)
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(bc.vectors(f[k - 1], f[k], gc.BLOCK, gc.RANGE)[0][keep]), err_msg=m)
        isl = oracle.detect_motion(np.ascontiguousarray(got[k]["entries"]), **det)
        assert gc.area_of(isl) == (areas[k - 1] or 0), m
        assert got[k]["motion"] == (None if isl is None else (isl[0], side)), m + ": batched island"
        assert (want[k]["motion"] is None) == (isl is None), m
        if isl is not None:
            assert want[k]["motion"][0] == isl[0], m
            np.testing.assert_array_equal(_bits(want[k]["motion"][1]), _bits(isl[1]), err_msg=m + ": the single push's island field")
