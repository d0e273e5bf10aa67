"""-m gpu: hip_klt over its whole parameter, window and frame domain (include/ofps_hip.h N3, N3m, N3f, N3p, N3pb, N3b, N3i), through the C ABI,
bit for bit against the restatements tests/indep_klt*.py on the cases of tests/klt_domain_cases.py: every window radius 1..7 and every depth
1..6 through the plain kernels and through each compiled variant, all nine (cell, score radius) pairs, the smallest and the odd frames, the
settings at both ends of their ranges, 0/255 and many-equal-maxima content.  The host forms and the _dev forms, the latter with guard words
behind every output.  No tolerance anywhere.  Expectations are computed once per process and shared read-only."""
from functools import lru_cache

import numpy as np
import pytest

from ofps_amd._lib import OfpsHipError

import indep_klt as ik
import indep_klt_fb as ifb
import indep_klt_intra as ii
import indep_klt_pred as ip
import klt_cases as kc
import klt_domain_cases as dc

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64                                                # guard words behind every device output
GUARD_WORD = 0x5A17C0DE
BY_ID = {c.id: c for c in dc.FLOW_CASES}


@pytest.fixture(scope="module")
def shared_ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


@pytest.fixture
def ctx(shared_ctx):
    yield shared_ctx
    _defaults(shared_ctx)


def _defaults(ctx):
    ctx.set_klt(); ctx.set_klt_mean_removal(0); ctx.set_klt_fb(0); ctx.set_klt_intra(0); ctx.set_klt_cut(0)
    ctx.set_klt_prediction(0); ctx.set_klt_batch_prediction(0)
    ctx.lk_reset()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _kw(c):
    return dict(cell=c.cell, r=c.r, min_score=c.min_score, min_eig=c.min_eig, max_residual=c.R, mean_removal=c.zm, fb_limit=c.F)


@lru_cache(maxsize=None)
def _expect(c):
    prev, cur = dc.pair(c.frame)
    return ii.flow_from(prev, cur, c.L, c.w, c.K, None, c.q, c.P, **_kw(c))


def _set(ctx, c):
    ctx.set_klt(c.cell, c.r, c.min_score, c.min_eig, c.R)
    ctx.set_klt_mean_removal(int(c.zm)); ctx.set_klt_fb(c.F); ctx.set_klt_intra(c.q); ctx.set_klt_cut(c.P)


def _quads_of(exp):
    s = exp["slots"]
    have = s[:, 5] != ik.ST_NONE
    return s[have][:, :2], np.column_stack([s[have, 3], s[have, 4], exp["residuals"][have], s[have, 5]]).astype(np.int32)


def _counts(slots):
    return np.bincount(np.asarray(slots)[:, 5], minlength=8)


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


class _Dev:
    """device buffers of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs, self.raw = ctx, [], []

    def buf(self, words, fill=None):
        b = _DevBuf(self.ctx, max(int(words), 1), fill)
        self.bufs.append(b)
        return b

    def frame(self, img, pad=0):
        """one frame with `pad` poisoned bytes behind every row -> (pointer, stride)"""
        view, stride = kc.padded(img, pad)
        return self.bytes(view.base if view.base is not None else view), stride

    def bytes(self, arr):
        host = np.ascontiguousarray(arr)
        ptr = self.ctx.malloc(host.nbytes)
        self.ctx.memcpy_h2d(ptr, host)
        self.raw.append(ptr)
        return ptr

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        for b in self.bufs:
            b.free()
        for p in self.raw:
            self.ctx.free(p)


def _views(c):
    """the case's frames as the host forms take them: (prev, cur, stride or None)"""
    prev, cur = dc.pair(c.frame)
    if not c.pad:
        return prev, cur, None
    pv, stride = kc.padded(prev, c.pad)
    return pv, kc.padded(cur, c.pad)[0], stride


def _check_flow(ctx, c, exp=None):
    """every one-pair form of the case against the restatement's answer"""
    exp = _expect(c) if exp is None else exp
    prev, cur = dc.pair(c.frame)
    pv, cv, stride = _views(c)
    H, W = prev.shape
    _set(ctx, c)
    what = c.id
    ns = ctx.klt_slot_count(W, H)
    assert ns == len(exp["slots"]), what
    np.testing.assert_array_equal(ctx.klt_features(pv, stride=stride), exp["features"], err_msg=what + ": features")
    ent, slots = ctx.klt_flow(pv, cv, c.L, c.w, c.K, want_slots=True, stride=stride)
    np.testing.assert_array_equal(slots, exp["slots"], err_msg=what + ": slots")
    assert len(ent) == exp["count"], what
    np.testing.assert_array_equal(_bits(ent), _bits(exp["records"]), err_msg=what + ": record bits")
    pts, quads = _quads_of(exp)
    stage = c.q == 0                                          # the stage forms _track do not run N3i's verdict
    if stage:
        np.testing.assert_array_equal(ctx.klt_track(pv, cv, pts, c.L, c.w, c.K, stride=stride), quads, err_msg=what + ": quadruples")
    with _Dev(ctx) as d:
        dp, st = d.frame(prev, c.pad)
        dq, _ = d.frame(cur, c.pad)
        b_tri, b_rec, b_cnt, b_slots = d.buf(3 * ns), d.buf(4 * ns), d.buf(1), d.buf(6 * ns)
        b_pts, b_quad = d.buf(2 * len(pts), pts if len(pts) else None), d.buf(4 * len(pts))
        ctx.klt_features_dev(dp, W, H, st, b_tri.ptr)
        ctx.klt_flow_dev(dp, dq, W, H, st, c.L, c.w, c.K, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        if stage:
            ctx.klt_track_dev(dp, dq, W, H, st, b_pts.ptr, len(pts), c.L, c.w, c.K, b_quad.ptr)
        ctx.sync()
        np.testing.assert_array_equal(b_tri.read(np.int32).reshape(-1, 3)[:ns], exp["features"], err_msg=what + ": features_dev")
        np.testing.assert_array_equal(b_slots.read(np.int32).reshape(-1, 6)[:ns], exp["slots"], err_msg=what + ": flow_dev slots")
        count = int(b_cnt.read(np.uint32)[0])
        assert count == exp["count"], what
        np.testing.assert_array_equal(b_rec.read(np.uint32).reshape(-1, 4)[:count], _bits(exp["records"]), err_msg=what + ": flow_dev record bits")
        quad = b_quad.read(np.int32)
        if stage:
            np.testing.assert_array_equal(quad[:4 * len(pts)].reshape(-1, 4), quads, err_msg=what + ": track_dev")
    return slots


# ------------------------------------------------------------------------------------------------ B, C: the flow cases
@pytest.mark.parametrize("cid", [c.id for c in dc.FLOW_CASES])
def test_flow_case(ctx, cid):
    c = BY_ID[cid]
    slots = _check_flow(ctx, c)
    if len(slots) > 4 and cid not in dc.ALL_OR_NOTHING:       # the condition, on what the device returned
        kept = int((slots[:, 5] == 0).sum())
        assert 0 < kept < len(slots), (cid, _counts(slots))


def test_statuses_on_the_device(ctx):
    """the conditions of tests/test_klt_domain_cpu.py again, on what the device returns: every status occurs, 0 and 3 at every w and every L,
    5 at every w of the N3f sweep"""
    seen = set()
    per_w, per_L = {w: set() for w in dc.WS}, {L: set() for L in range(1, 7)}
    for c in [x for x in dc.B1 if x.frame == dc.WARP131] + dc.DEEP:
        _set(ctx, c)
        _, slots = ctx.klt_flow(*dc.pair(c.frame), c.L, c.w, c.K, want_slots=True)
        st = set(np.unique(slots[:, 5]).tolist())
        seen |= st; per_w[c.w] |= st; per_L[c.L] |= st
    assert all({0, 3} <= s for s in per_w.values()) and all({0, 3} <= s for s in per_L.values()), (per_w, per_L)
    fb_w = {w: False for w in dc.WS}
    for c in [x for x in dc.FB16_SWEEP if x.frame == dc.WARP131 and x.L == 1]:
        _set(ctx, c)
        _, slots = ctx.klt_flow(*dc.pair(c.frame), c.L, c.w, c.K, want_slots=True)
        fb_w[c.w] |= bool((slots[:, 5] == 5).any())
        seen |= set(np.unique(slots[:, 5]).tolist())
    assert all(fb_w.values()), fb_w
    for cid in dc.STATUS_WITNESSES:
        c = BY_ID[cid]
        _set(ctx, c)
        _, slots = ctx.klt_flow(*dc.pair(c.frame), c.L, c.w, c.K, want_slots=True)
        seen |= set(np.unique(slots[:, 5]).tolist())
    assert seen == set(range(8)), seen


def test_the_30th_iteration_and_the_clamp_are_reached(ctx):
    a, b = (_check_flow(ctx, BY_ID[k]) for k in ("K29", "K30"))
    assert int((a != b).any(1).sum()) == dc.K_PIN
    for cid, (kept, at_clamp) in dc.CLAMP_PIN.items():
        c = BY_ID[cid]
        s = _check_flow(ctx, c)
        k = s[:, 5] == 0
        assert (int(k.sum()), int(((np.abs(s[k, 3]) == 256 * c.w) | (np.abs(s[k, 4]) == 256 * c.w)).sum())) == (kept, at_clamp), cid


def test_min_eig_and_max_residual_at_values_from_the_restatement(ctx):
    for c in dc.EIG_MIXED:
        s = _check_flow(ctx, c)
        n = _counts(s)
        assert n[0] > 0 and n[2] > 0, (c.id, n)
    c, slot, R = dc.RESIDUAL_EXACT
    for r, status in ((R, 0), (R - 1, 4)):
        cr = c._replace(id=f"{c.id}-R{r}", R=r)
        exp = _expect(cr)
        assert int(exp["residuals"][slot]) == 16 * R * (2 * c.w + 1) ** 2 and int(exp["slots"][slot, 5]) == status
        s = _check_flow(ctx, cr, exp)
        assert int(s[slot, 5]) == status


@pytest.mark.parametrize("L,W,H", dc.TOO_SMALL)
def test_one_pixel_below_the_smallest_frame_is_refused(ctx, L, W, H):
    prev, cur = dc.pair(("warp", W, H, (1.3, -0.6)))
    ctx.set_klt(8, 1, 1, 1, 0)
    ns = ctx.klt_slot_count(W, H)
    for fn, args in ((ctx.klt_flow, (prev, cur, L, 4, 10)), (ctx.klt_track, (prev, cur, np.array([[5, 5]]), L, 4, 10)),
                     (ctx.klt_track_q, (prev, cur, np.array([[5, 5]]), L, 4, 10))):
        with pytest.raises(OfpsHipError) as e:
            fn(*args)
        assert e.value.code == EINVAL
    with _Dev(ctx) as d:                                      # the _dev form: refused before anything is computed
        dp, st = d.frame(prev)
        dq, _ = d.frame(cur)
        b_rec, b_cnt, b_slots = d.buf(4 * ns), d.buf(1), d.buf(6 * ns)
        with pytest.raises(OfpsHipError) as e:
            ctx.klt_flow_dev(dp, dq, W, H, st, L, 4, 10, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
        assert e.value.code == EINVAL
        ctx.sync()
        for b in (b_rec, b_cnt, b_slots):
            assert (b.read(np.uint32) == GUARD_WORD).all()
    ent = ctx.klt_flow(prev, cur, L - 1, 4, 10)               # one level less is legal on the same frame
    assert len(ent) > 0


# ------------------------------------------------------------------------------------------------ A: features
@lru_cache(maxsize=None)
def _features(c):
    return ik.features(dc.pair(c.frame)[0], c.cell, c.r, c.min_score)


def _check_features(ctx, c, want):
    prev = dc.pair(c.frame)[0]
    H, W = prev.shape
    ctx.set_klt(c.cell, c.r, c.min_score, 1, 0)
    ns = ctx.klt_slot_count(W, H)
    assert ns == len(want), c.id
    pv, stride = kc.padded(prev, c.pad) if c.pad else (prev, None)
    got = ctx.klt_features(pv, stride=stride)
    np.testing.assert_array_equal(got, want, err_msg=c.id + ": features")
    with _Dev(ctx) as d:
        dp, st = d.frame(prev, c.pad)
        b = d.buf(3 * ns)
        ctx.klt_features_dev(dp, W, H, st, b.ptr)
        ctx.sync()
        np.testing.assert_array_equal(b.read(np.int32).reshape(-1, 3)[:ns], want, err_msg=c.id + ": features_dev")
    return got


@pytest.mark.parametrize("cid", [c.id for c in dc.FEATURE_CASES])
def test_features(ctx, cid):
    c = next(x for x in dc.FEATURE_CASES if x.id == cid)
    got = _check_features(ctx, c, _features(c))
    if c in dc.GEOMETRY_CASES:
        nx, ny = ik.slot_grid(*dc.pair(c.frame)[0].shape[::-1], c.cell)
        j = int(cid.rsplit("j", 1)[1])
        last = got.reshape(ny, nx, 3)
        if j < c.r + 2:                                       # no admissible pixel in the last column and row of cells: status 1 from geometry
            assert (last[:, -1, 0] == -1).all() and (last[-1, :, 0] == -1).all() and (last[:-1, :-1, 0] >= 0).all()
        else:                                                 # exactly one admissible column / row: whatever is found there lies on it
            W, H = dc.pair(c.frame)[0].shape[::-1]
            col, row = last[:, -1], last[-1, :]
            assert (col[col[:, 0] >= 0][:, 0] == W - c.r - 2).all() and (row[row[:, 0] >= 0][:, 1] == H - c.r - 2).all()
            assert (col[:, 0] >= 0).any() and (row[:, 0] >= 0).any()


def test_tiny_frames_hold_a_feature_and_a_cell_without_one(ctx):
    kept = none = 0
    for c in dc.TINY_CASES:
        ctx.set_klt(c.cell, c.r, 1, 1, 0)
        f = ctx.klt_features(dc.pair(c.frame)[0])
        assert len(f) <= 2
        kept += int((f[:, 0] >= 0).sum()); none += int((f[:, 0] < 0).sum())
        if c.frame[1:] == (8, 8):
            assert (f[0, 0] >= 0) == (c.r < 3), c.id                   # r = 1, 2: a feature; r = 3: the frame is narrower than 2r + 3
    assert kept > 0 and none > 0


def test_ties_go_to_the_smallest_y_then_x(ctx):
    ctx.set_klt(8, 1, 1, 1, 0)
    f = ctx.klt_features(dc.pair(("ties", 64, 48))[0])
    assert f[:4].tolist() == [[2, 2, 2560000], [8, 2, 2560000], [16, 2, 2560000], [24, 2, 2560000]]


def test_min_score_equal_to_a_cells_best_score(ctx):
    c = dc.MINSCORE_AT
    base = _features(c)
    order = np.sort(base[:, 2])
    ms = int(order[len(order) // 2])                          # the median cell's best score, from the restatement's own list
    assert ms > 1
    for m in (ms, ms + 1):
        want = ik.features(dc.pair(c.frame)[0], c.cell, c.r, m)
        got = _check_features(ctx, c._replace(id=f"{c.id}-{m}", min_score=m), want)
        assert bool((got[:, 2] == ms).any()) == (m == ms)
        assert 0 < int((got[:, 0] >= 0).sum()) < len(got)


# ------------------------------------------------------------------------------------------------ B.5: caller-given points
def _point_pair():
    return dc.pair(dc.POINT_FRAME)


@lru_cache(maxsize=None)
def _point_expect(L, w, at_q):
    prev, cur = _point_pair()
    H, W = prev.shape
    if at_q:
        return ifb.track_points_q(prev, cur, np.concatenate([dc.q_positions(W, H), dc.q_outside(W, H)]), L, w, 10, 1, 64)
    return ik.track(prev, cur, np.concatenate([dc.frame_points(W, H), dc.px_outside(W, H)]), L, w, 10, 1, 64)


@pytest.mark.parametrize("L", dc.POINT_LS)
@pytest.mark.parametrize("w", dc.WS)
def test_track_on_corners_edges_and_centre(ctx, w, L):
    prev, cur = _point_pair()
    H, W = prev.shape
    ctx.set_klt(16, 2, 1, 1, 64)
    left = np.array([0, 0, 0, ik.ST_LEFT], np.int32)
    with _Dev(ctx) as d:
        dp, st = d.frame(prev)
        dq, _ = d.frame(cur)
        for at_q, inside, outside, host, dev in ((False, dc.frame_points(W, H), dc.px_outside(W, H), ctx.klt_track, ctx.klt_track_dev),
                                                 (True, dc.q_positions(W, H), dc.q_outside(W, H), ctx.klt_track_q, ctx.klt_track_q_dev)):
            want = _point_expect(L, w, at_q)
            n = len(inside)
            assert (want[n:] == left).all()
            np.testing.assert_array_equal(host(prev, cur, inside, L, w, 10), want[:n], err_msg=f"q={at_q}")
            for k in range(len(outside)):                     # the host forms refuse a point one beyond an end
                with pytest.raises(OfpsHipError) as e:
                    host(prev, cur, outside[k:k + 1], L, w, 10)
                assert e.value.code == EINVAL
            pts = np.concatenate([inside, outside])
            b_pts, b_quad = d.buf(2 * len(pts), pts), d.buf(4 * len(pts))
            dev(dp, dq, W, H, st, b_pts.ptr, len(pts), L, w, 10, b_quad.ptr)
            ctx.sync()
            np.testing.assert_array_equal(b_quad.read(np.int32).reshape(-1, 4), want, err_msg=f"q={at_q} _dev")
            np.testing.assert_array_equal(b_pts.read(np.int32).reshape(-1, 2), pts)


# ------------------------------------------------------------------------------------------------ C: N3p
def _guess_points(W, H):
    rng = np.random.default_rng(46)
    return np.concatenate([dc.frame_points(W, H), np.column_stack([rng.integers(8, W - 8, 19), rng.integers(8, H - 8, 19)])]).astype(np.int32)


@pytest.mark.parametrize("L,w,zm,F", [(1, 2, False, 0), (6, 2, False, 0), (1, 5, True, 0), (6, 5, False, 16), (6, 6, True, 16), (6, 3, False, 0)])
def test_track_from_guesses(ctx, L, w, zm, F):
    prev, cur = _point_pair()
    K = dc.GUESS_ITERS
    H, W = prev.shape
    pts = _guess_points(W, H)
    gs = dc.guess_list(len(pts))
    ctx.set_klt(16, 2, 1, 1, 0); ctx.set_klt_mean_removal(int(zm)); ctx.set_klt_fb(F)
    want = ip.track_from(prev, cur, pts, gs, L, w, K, 1, 0, zm, F)
    assert {0, 3} <= set(want[:, 3].tolist())
    np.testing.assert_array_equal(ctx.klt_track_from(prev, cur, pts, gs, L, w, K), want)
    beyond = gs.copy()
    beyond[::2, 0] = dc.GUESS_BEYOND; beyond[1::2, 1] = -dc.GUESS_BEYOND
    with pytest.raises(OfpsHipError) as e:                    # the host form refuses a guess beyond 2^23
        ctx.klt_track_from(prev, cur, pts, beyond, L, w, K)
    assert e.value.code == EINVAL
    want_beyond = ip.track_from(prev, cur, pts, beyond, L, w, K, 1, 0, zm, F)
    zeroed = ip.track_from(prev, cur, pts, np.zeros_like(gs), L, w, K, 1, 0, zm, F)
    np.testing.assert_array_equal(want_beyond, zeroed)        # in the _dev form it counts as (0, 0)
    assert (want != zeroed).any(1).sum() >= 3                 # and the guesses matter
    with _Dev(ctx) as d:
        dp, st = d.frame(prev)
        dq, _ = d.frame(cur)
        b_pts = d.buf(2 * len(pts), pts)
        for g, exp in ((gs, want), (beyond, want_beyond)):
            b_g, b_quad = d.buf(2 * len(pts), g), d.buf(4 * len(pts))
            ctx.klt_track_from_dev(dp, dq, W, H, st, b_pts.ptr, b_g.ptr, len(pts), L, w, K, b_quad.ptr)
            ctx.sync()
            np.testing.assert_array_equal(b_quad.read(np.int32).reshape(-1, 4), exp)


def _seq_kw(kw):
    k = dict(kw)
    L, w, K = k.pop("L"), k.pop("w"), k.pop("K")
    zm, F = k.pop("zm", False), k.pop("F", 0)
    return L, w, K, zm, F, k


@lru_cache(maxsize=None)
def _batch_expect(bid):
    b = next(x for x in dc.BATCH_CASES + dc.CHAIN_CASES if x.id == bid)
    L, w, K, zm, F, k = _seq_kw(b.kw)
    return tuple(ii.flow_batch(dc.sequence(b.seq), L, w, K, b.ref_mode, 0, 0, b.chained, None, cell=k["cell"], r=k["r"], mean_removal=zm, fb_limit=F))


@pytest.mark.parametrize("bid", [b.id for b in dc.CHAIN_CASES])
def test_flow_from_chained_over_three_frames(ctx, bid):
    b = next(x for x in dc.CHAIN_CASES if x.id == bid)
    L, w, K, zm, F, k = _seq_kw(b.kw)
    fr = dc.sequence(b.seq)
    H, W = fr.shape[1:]
    ctx.set_klt(k["cell"], k["r"], 1, 1, 0); ctx.set_klt_mean_removal(int(zm)); ctx.set_klt_fb(F)
    exp = _batch_expect(bid)
    ns = ctx.klt_slot_count(W, H)
    prev_slots = None
    with _Dev(ctx) as d:
        dfr = [d.frame(f)[0] for f in fr]
        d_prev = None
        for i, e in enumerate(exp):
            n = _counts(e["slots"])
            assert 0 < n[0] < ns and (i == 0 or np.any(e["guesses"])), (bid, i, n)
            ent, slots = ctx.klt_flow_from(fr[i], fr[i + 1], L, w, K, prev_slots)
            np.testing.assert_array_equal(slots, e["slots"], err_msg=f"{bid} pair {i}: slots")
            np.testing.assert_array_equal(_bits(ent), _bits(e["records"]), err_msg=f"{bid} pair {i}: records")
            b_rec, b_cnt, b_slots = d.buf(4 * ns), d.buf(1), d.buf(6 * ns)
            ctx.klt_flow_from_dev(dfr[i], dfr[i + 1], W, H, W, L, w, K, d_prev, b_rec.ptr, b_cnt.ptr, b_slots.ptr)
            ctx.sync()
            np.testing.assert_array_equal(b_slots.read(np.int32).reshape(-1, 6), e["slots"], err_msg=f"{bid} pair {i}: _dev slots")
            cnt = int(b_cnt.read(np.uint32)[0])
            assert cnt == e["count"]
            np.testing.assert_array_equal(b_rec.read(np.uint32).reshape(-1, 4)[:cnt], _bits(e["records"]))
            prev_slots, d_prev = slots, b_slots.ptr


# ------------------------------------------------------------------------------------------------ A.5, C: the batch forms
@pytest.mark.parametrize("bid", [b.id for b in dc.BATCH_CASES])
def test_batch(ctx, bid):
    b = next(x for x in dc.BATCH_CASES if x.id == bid)
    L, w, K, zm, F, k = _seq_kw(b.kw)
    fr = dc.sequence(b.seq)
    n, H, W = fr.shape
    pairs = n - 1
    ctx.set_klt(k["cell"], k["r"], 1, 1, 0); ctx.set_klt_mean_removal(int(zm)); ctx.set_klt_fb(F)
    exp = _batch_expect(bid)
    ns = ctx.klt_slot_count(W, H)
    pad, extra = (5, 3) if b.extra == "pitch" else (0, 0)
    buf = np.full((n, H + extra, W + pad), 0xA5, np.uint8)
    buf[:, :H, :W] = fr
    view = buf[:, :H, :W]
    stride, pitch = W + pad, (H + extra) * (W + pad)
    assert (pitch > stride * H) == (b.extra == "pitch")
    host = ctx.klt_flow_batch_from if b.chained else ctx.klt_flow_batch
    ent, counts, slots = host(view, L, w, K, b.ref_mode, want_slots=True)
    prev_slots = None
    for i, e in enumerate(exp):
        what = f"{bid} item {i}"
        nst = _counts(e["slots"])
        assert 0 < nst[0] < ns, (what, nst)
        np.testing.assert_array_equal(slots[i], e["slots"], err_msg=what + ": slots")
        assert int(counts[i]) == e["count"], what
        np.testing.assert_array_equal(_bits(ent[i, :counts[i]]), _bits(e["records"]), err_msg=what + ": records")
        a = fr[0] if b.ref_mode else fr[i]                    # and the one-pair call
        one_ent, one_slots = ctx.klt_flow_from(a, fr[i + 1], L, w, K, prev_slots if b.chained else None)
        np.testing.assert_array_equal(one_slots, slots[i], err_msg=what + ": the one-pair call's slots")
        np.testing.assert_array_equal(_bits(one_ent), _bits(ent[i, :counts[i]]), err_msg=what + ": the one-pair call's records")
        prev_slots = one_slots
    with _Dev(ctx) as d:
        dfr = d.bytes(buf)
        b_rec, b_cnt = d.buf(4 * ns * pairs), d.buf(pairs)
        b_slots = None if b.extra == "noslots" else d.buf(6 * ns * pairs)
        dev = ctx.klt_flow_batch_from_dev if b.chained else ctx.klt_flow_batch_dev
        dev(dfr, n, W, H, stride, pitch, b.ref_mode, L, w, K, b_rec.ptr, b_cnt.ptr, b_slots.ptr if b_slots else None)
        ctx.sync()
        dcnt = b_cnt.read(np.uint32)
        drec = b_rec.read(np.uint32).reshape(pairs, ns, 4)
        np.testing.assert_array_equal(dcnt, [e["count"] for e in exp])
        for i, e in enumerate(exp):
            np.testing.assert_array_equal(drec[i, :e["count"]], _bits(e["records"]), err_msg=f"{bid} item {i}: _dev records")
        if b_slots:
            np.testing.assert_array_equal(b_slots.read(np.int32).reshape(pairs, ns, 6), np.stack([e["slots"] for e in exp]))


# ------------------------------------------------------------------------------------------------ C: N3i's activity, the fused form
@pytest.mark.parametrize("w", dc.WS)
def test_activity(ctx, w):
    for spec in dc.ACTIVITY_FRAMES:
        img = dc.pair(spec)[0]
        H, W = img.shape
        pts = dc.activity_points(W, H)
        want = ii.activity(img, pts, w)
        assert (want == 0).all() == (spec[0] == "flat")
        np.testing.assert_array_equal(ctx.klt_activity(img, pts, w), want, err_msg=f"{spec} w={w}")
        allpts = np.concatenate([pts, dc.px_outside(W, H)])
        with _Dev(ctx) as d:
            for pad in (0, 13):
                dp, st = d.frame(img, pad)
                b_pts, b_act = d.buf(2 * len(allpts), allpts), d.buf(len(allpts))
                ctx.klt_activity_dev(dp, W, H, st, b_pts.ptr, len(allpts), w, b_act.ptr)
                ctx.sync()
                np.testing.assert_array_equal(b_act.read(np.uint32), ii.activity(img, allpts, w), err_msg=f"{spec} w={w} pad={pad} _dev")


def test_fused_sparse_form_at_five_levels(ctx):
    c = dc.FUSED
    prev, cur = dc.pair(c.frame)
    exp = _expect(c)
    _set(ctx, c)
    ctx.lk_reset()
    kw = dict(levels=c.L, radius=c.w, iters=c.K, sparse=True)
    first = ctx.lk_push_frame_fused(prev, **kw)
    assert not first["have_vectors"]
    r = ctx.lk_push_frame_fused(cur, **kw)
    want = ctx.klt_flow(prev, cur, c.L, c.w, c.K)
    assert r["have_vectors"] and r["n_vectors"] == len(want) == exp["count"] and 0 < exp["count"] < len(exp["slots"])
    np.testing.assert_array_equal(_bits(r["entries"]), _bits(want))
    np.testing.assert_array_equal(_bits(want), _bits(exp["records"]))


# ------------------------------------------------------------------------------------------------ D: both sides of every bound
def _refused(fn, *a, **k):
    with pytest.raises(OfpsHipError) as e:
        fn(*a, **k)
    assert e.value.code == EINVAL, e.value


def test_settings_at_both_sides_of_their_bounds(ctx):
    base = dict(cell=16, score_radius=2, min_score=1, min_eig=1, max_residual=0)
    names = dict(cell="cell", score_radius="r", min_score="min_score", min_eig="min_eig", max_residual="R")
    small = dc.flow("bound", dc.BINARY64, cell=16, r=2, L=2, w=3)
    for key, bad, good in dc.SET_KLT_BOUNDS:
        for v in bad:
            ctx.set_klt(8, 3, 7, 9, 160)
            _refused(ctx.set_klt, **dict(base, **{key: v}))
            assert ctx.get_klt() == dict(cell=8, score_radius=3, min_score=7, min_eig=9, max_residual=160), (key, v)
        for v in good:
            _check_flow(ctx, small._replace(id=f"bound-{key}-{v}", **{names[key]: v}))
    bad, good = dc.FB_BOUNDS
    for v in bad:
        ctx.set_klt_fb(7)
        _refused(ctx.set_klt_fb, v)
        assert ctx.get_klt_fb() == 7
    for v in good:
        _check_flow(ctx, small._replace(id=f"bound-F-{v}", F=v))


def test_call_arguments_at_both_sides_of_their_bounds(ctx):
    deep = dc.flow("bound", dc.BOUND_FRAME, cell=32, r=2, L=2, w=3, K=10)
    prev, cur = dc.pair(deep.frame)
    H, W = prev.shape
    pts, gs = np.array([[20, 20]]), np.array([[0, 0]])
    for key, bad, good in dc.CALL_BOUNDS:
        for v in bad:
            c = deep._replace(**{key: v})
            ctx.set_klt(32, 2, 1, 1, 0)
            for fn, a in ((ctx.klt_flow, (prev, cur)), (ctx.klt_flow_from, (prev, cur)), (ctx.klt_track, (prev, cur, pts)),
                          (ctx.klt_track_q, (prev, cur, pts))):
                _refused(fn, *a, c.L, c.w, c.K)
            _refused(ctx.klt_track_from, prev, cur, pts, gs, c.L, c.w, c.K)
            _refused(ctx.klt_flow_batch, np.stack([prev, cur]), c.L, c.w, c.K)
            if key == "w":
                _refused(ctx.klt_activity, prev, pts, v)
            assert ctx.get_klt() == dict(cell=32, score_radius=2, min_score=1, min_eig=1, max_residual=0)
        for v in good:
            _check_flow(ctx, deep._replace(id=f"bound-{key}-{v}", **{key: v}))
    # stride = W - 1: rows that overlap; refused before anything is read
    buf = np.zeros(H * W, np.uint8)
    narrow = np.lib.stride_tricks.as_strided(buf, (H, W), (W - 1, 1))
    ctx.set_klt(32, 2, 1, 1, 0)
    _refused(ctx.klt_features, narrow, stride=W - 1)
    _refused(ctx.klt_flow, narrow, narrow, 2, 3, 10, stride=W - 1)
    _refused(ctx.klt_track, narrow, narrow, pts, 2, 3, 10, stride=W - 1)
    _refused(ctx.klt_activity, narrow, pts, 3, stride=W - 1)
    with _Dev(ctx) as d:
        dp, _ = d.frame(prev)
        b_rec, b_cnt = d.buf(4 * 64), d.buf(1)
        _refused(ctx.klt_flow_dev, dp, dp, W, H, W - 1, 2, 3, 10, b_rec.ptr, b_cnt.ptr)
        ctx.sync()
        assert (b_rec.read(np.uint32) == GUARD_WORD).all() and (b_cnt.read(np.uint32) == GUARD_WORD).all()
    _check_flow(ctx, deep._replace(id="bound-stride-W"))      # stride = W: the restatement's answer
