"""-m gpu: hip_sad's median test (include/ofps_hip.h N1v) against the restatement tests/indep_sad_median.py on the cases of
tests/sad_median_cases.py.  Residuals, flags, records and winners are integers or copies: every equality is bit for bit.  The one exception
is the quaternion of the fused path's device-count form, held to the solver's documented parity with ofps_hip_almeida on the same records:
2e-6 (least squares).  tests/test_sad_median_cpu.py proves on the restatement that the inputs separate test-on from test-off.

Where a search runs in a mode the CPU oracle does not restate here (search levels with neighbour predictors, mean removal), the INTEGER
winners the verdicts are computed from are the library's own unfiltered winners in that mode -- tests/test_sad_pred_gpu.py and
tests/test_sad_prefilter_gpu.py hold those to their restatements -- and the verdicts are the restatement's of this test."""
import numpy as np
import pytest

import indep_sad_median as im
import sad_consistency_cases as cc
import sad_gate_cases as gc
import sad_median_cases as mc

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1, 0, 0, 0], np.float32)
EINVAL = -1
QUAT_BOUND = 2e-6                                        # least squares: the solver's documented parity
B, R = mc.SCENE_B, mc.SCENE_R


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
    DEFAULT = dict(median=0, limit=0, gate=0, scale=1, levels=1, predictors=0, prefilter=0, pruned=False)

    def __init__(self, ctx, **kw):
        self.ctx, self.v = ctx, dict(self.DEFAULT, **kw)

    def _apply(self, v):
        c = self.ctx
        c.set_sad_median(v["median"]); c.set_sad_consistency(v["limit"]); c.set_sad_gate(v["gate"]); c.set_sad_motion_scale(v["scale"])
        c.set_sad_levels(v["levels"]); c.set_sad_predictors(v["predictors"]); c.set_sad_prefilter(v["prefilter"])
        c.set_sad_mode(c.SAD_PRUNED if v["pruned"] else c.SAD_EXHAUSTIVE)

    def __enter__(self):
        self._apply(self.v)

    def __exit__(self, *exc):
        self._apply(self.DEFAULT)


# --------------------------------------------------------------------------------------------------------------- the test alone
def _check_alone(ctx, nbx, nby, best, kin, limits, what):
    W, H = mc.field_frame(nbx, nby)
    want_r2 = im.residual2(best, kin, nbx, nby)
    for limit in limits:
        w = f"{what} limit {limit}"
        r2, keep = ctx.sad_median(best, kin, W, H, mc.BLOCK, limit)
        assert r2.dtype == np.uint32 and keep.dtype == np.uint8 and len(r2) == len(keep) == nbx * nby, w
        np.testing.assert_array_equal(r2, want_r2, err_msg=w + ": residual")
        np.testing.assert_array_equal(keep, im.keep_flags(best, kin, nbx, nby, limit), err_msg=w + ": keep bytes")
    r2, none = ctx.sad_median(best, kin, W, H, mc.BLOCK, 2, want_keep=False)           # one output NULL, then the other
    assert none is None
    np.testing.assert_array_equal(r2, want_r2)
    none, keep = ctx.sad_median(best, kin, W, H, mc.BLOCK, 2, want_residual=False)
    assert none is None
    np.testing.assert_array_equal(keep, im.keep_flags(best, kin, nbx, nby, 2))


def _check_alone_dev(ctx, nbx, nby, best, kin, limits, what, block=mc.BLOCK, frame=None):
    """the _dev form: both outputs, residual only, keep only; 64 guard words / bytes behind both outputs"""
    import torch
    W, H = mc.field_frame(nbx, nby) if frame is None else frame
    n = nbx * nby
    d_best = torch.from_numpy(np.array(best, np.int32)).cuda()
    d_kin = None if kin is None else torch.from_numpy(np.array(kin, np.uint8)).cuda()
    p_kin = None if kin is None else d_kin.data_ptr()
    want_r2 = im.residual2(best, kin, nbx, nby)
    for limit in limits:
        want_keep = im.keep_flags(best, kin, nbx, nby, limit)
        for outs in ("both", "residual", "keep"):
            w = f"{what} limit {limit} {outs}"
            d_r2 = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
            d_keep = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.sad_median_dev(d_best.data_ptr(), p_kin, W, H, block, limit, d_r2.data_ptr() if outs != "keep" else None,
                               d_keep.data_ptr() if outs != "residual" else None)
            ctx.sync()
            r2, keep = d_r2.cpu().numpy(), d_keep.cpu().numpy()
            assert (r2[n:] == -1).all() and (keep[n:] == 7).all(), w + ": guard words"
            if outs != "keep":
                np.testing.assert_array_equal(r2[:n].view(np.uint32), want_r2, err_msg=w)
            else:
                assert (r2 == -1).all(), w
            if outs != "residual":
                np.testing.assert_array_equal(keep[:n], want_keep, err_msg=w)
            else:
                assert (keep == 7).all(), w


@pytest.mark.parametrize("name", list(mc.FIELDS))
def test_alone_on_the_derived_cases(ctx, name):
    nbx, nby, best, kin, want = mc.FIELDS[name]()
    limits = sorted(set(mc.LIMITS) | set(want))
    _check_alone(ctx, nbx, nby, best, kin, limits, name)
    _check_alone_dev(ctx, nbx, nby, best, kin, limits, name + " dev")
    W, H = mc.field_frame(nbx, nby)
    for limit, flags in want.items():                    # the flags the case derives from the definition, of the library itself
        np.testing.assert_array_equal(ctx.sad_median(best, kin, W, H, mc.BLOCK, limit)[1], flags, err_msg=f"{name} limit {limit}")
    if kin is not None:                                  # keep_in NULL is all ones: another answer on these cases
        _check_alone(ctx, nbx, nby, best, None, mc.LIMITS, name + " without keep_in")


@pytest.mark.parametrize("lattice,block,frame", [((25, 17), 8, (200, 136)), ((120, 67), 16, (1920, 1080))], ids=["25x17", "120x67"])
def test_alone_on_synthetic_lattices(ctx, lattice, block, frame):
    """25 x 17: two workgroups, the second partial; 120 x 67 = 8,040 blocks: 32 workgroups, the last one partial.  Triples only, no search"""
    nbx, nby = lattice
    assert (frame[0] // block, frame[1] // block) == lattice
    best, kin = mc.synthetic_field(nbx, nby)
    _check_alone_dev(ctx, nbx, nby, best, kin, mc.LIMITS, "synthetic", block, frame)
    _check_alone_dev(ctx, nbx, nby, best, None, (2,), "synthetic without keep_in", block, frame)
    r2, keep = ctx.sad_median(best, kin, frame[0], frame[1], block, 2)                  # the host form at this size
    np.testing.assert_array_equal(r2, im.residual2(best, kin, nbx, nby))
    np.testing.assert_array_equal(keep, im.keep_flags(best, kin, nbx, nby, 2))


def test_alone_on_winners_far_outside_any_search(ctx):
    """|d| = 508: a defined residual and flag whatever the triples hold"""
    best, kin = mc.synthetic_field(25, 17, seed=1, big=508)
    assert np.abs(best[:, :2]).max() == 508
    r2 = im.residual2(best, kin, 25, 17)
    assert r2.max() >= 2 * 508 - 2 * 8                   # an outlier against a median of small vectors
    _check_alone_dev(ctx, 25, 17, best, kin, (1, 2, 254, 255), "508", 8, (200, 136))
    best = np.array(best)
    best[::7, 0] = np.iinfo(np.int32).max; best[3::11, 1] = np.iinfo(np.int32).min       # the residual saturates, the flag follows it
    _check_alone_dev(ctx, 25, 17, best, kin, (255,), "int32 extremes", 8, (200, 136))


# --------------------------------------------------------------------------------------------------------------- the scene through the search
def _scene_keep_in(gate, limit):
    """the other criteria's flags of the scene, from their restatements -> u8 [nblk] or None"""
    prev, cur = mc.scene()
    kin = None
    if limit:
        kin = cc.keep_flags(mc.scene_vectors()[1], mc.scene_vectors(reverse=True)[1], mc.SCENE_W, mc.SCENE_H, B, limit)
    if gate:
        g = gc.keep_flags(cur, B, gate)
        kin = g if kin is None else kin & g
    return None if kin is None else kin.astype(np.uint8)


def test_sad_flow_follows_the_contexts_limit(ctx):
    prev, cur = mc.scene()
    ent0, F = mc.scene_vectors()
    e_plain, b_plain = ctx.sad_flow(prev, cur, B, R, want_best=True)                   # the unfiltered call IS the restatement's search
    np.testing.assert_array_equal(_bits(e_plain), _bits(ent0))
    np.testing.assert_array_equal(b_plain, F)
    for limit in mc.LIMITS:
        keep = mc.scene_keep(limit)
        with _settings(ctx, median=limit):
            assert ctx.get_sad_median() == limit
            ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
            ent_only = ctx.sad_flow(prev, cur, B, R)                                    # without out_best
        assert len(ent) == len(best) == int(keep.sum()), limit                          # *n_out
        np.testing.assert_array_equal(_bits(ent), _bits(mc.filtered(ent0, keep)), err_msg=f"limit {limit}: records")
        np.testing.assert_array_equal(best, mc.filtered(F, keep), err_msg=f"limit {limit}: out_best")
        np.testing.assert_array_equal(_bits(ent_only), _bits(ent))
    assert int(mc.scene_keep(mc.SCENE_LIMIT).sum()) < mc.SCENE_NBLK
    # with the other criteria on in the context as well: kept iff all keep it, the median over THEIR kept blocks
    for gate, limit in ((1, 0), (0, 1), (1, 1)):
        kin = _scene_keep_in(gate, limit)
        keep = im.keep_flags(F, kin, mc.SCENE_NBX, mc.SCENE_NBY, mc.SCENE_LIMIT)
        with _settings(ctx, median=mc.SCENE_LIMIT, gate=gate, limit=limit):
            ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
        np.testing.assert_array_equal(_bits(ent), _bits(mc.filtered(ent0, keep)), err_msg=f"gate {gate} check {limit}: records")
        np.testing.assert_array_equal(best, mc.filtered(F, keep), err_msg=f"gate {gate} check {limit}: out_best")


def _median_dev(ctx, prev, cur, gate, limit, median, want_best=True):
    import torch
    H, W = prev.shape
    nblk = (W // B) * (H // B)
    d_prev, d_cur = torch.from_numpy(np.array(prev)).cuda(), torch.from_numpy(np.array(cur)).cuda()
    d_ent = torch.zeros((nblk, 4), dtype=torch.float32, device="cuda")
    d_best = torch.zeros((nblk, 3), dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_flow_median_dev(d_prev.data_ptr(), d_cur.data_ptr(), W, H, W, B, R, gate, limit, median, d_ent.data_ptr(),
                            d_best.data_ptr() if want_best else None, d_cnt.data_ptr())
    ctx.sync()
    n = int(d_cnt.cpu().numpy()[0])
    return d_ent.cpu().numpy()[:n], d_best.cpu().numpy()[:n]


@pytest.mark.parametrize("gate,limit", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["alone", "gate1", "check1", "gate1-check1"])
def test_median_dev_form_with_explicit_values(ctx, gate, limit):
    prev, cur = mc.scene()
    ent0, F = mc.scene_vectors()
    kin = _scene_keep_in(gate, limit)
    keep = im.keep_flags(F, kin, mc.SCENE_NBX, mc.SCENE_NBY, mc.SCENE_LIMIT)
    assert ctx.get_sad_median() == 0 and ctx.get_sad_gate() == 0 and ctx.get_sad_consistency() == 0      # the device form takes its own values
    ent, best = _median_dev(ctx, prev, cur, gate, limit, mc.SCENE_LIMIT)
    assert len(ent) == int(keep.sum()) < mc.SCENE_NBLK
    np.testing.assert_array_equal(_bits(ent), _bits(mc.filtered(ent0, keep)))
    np.testing.assert_array_equal(best, mc.filtered(F, keep))
    ent, _ = _median_dev(ctx, prev, cur, gate, limit, mc.SCENE_LIMIT, want_best=False)
    np.testing.assert_array_equal(_bits(ent), _bits(mc.filtered(ent0, keep)))

MODES = {  # id: (settings of the search, the integer winners are the restatement's plain ones)
    "scale4": (dict(scale=4), True),
    "levels2-predictors": (dict(levels=2, predictors=1), False),
    "prefilter4": (dict(prefilter=4), False),
    "pruned": (dict(pruned=True), True),
    "scale4-levels2-check1": (dict(scale=4, levels=2, limit=1), False),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_scene_in_the_other_search_modes(ctx, mode):
    """the records are the mode's unfiltered ones (quarter-pel at scale 4), the verdicts the INTEGER winners', the triples the mode's compacted"""
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
    kin = cc.keep_flags(F, G, mc.SCENE_W, mc.SCENE_H, B, check).astype(np.uint8) if check else None
    keep = im.keep_flags(F, kin, mc.SCENE_NBX, mc.SCENE_NBY, mc.SCENE_LIMIT)
    assert 0 < int(keep.sum()) < mc.SCENE_NBLK
    with _settings(ctx, median=mc.SCENE_LIMIT, **kw):
        ent, best = ctx.sad_flow(prev, cur, B, R, want_best=True)
        ent_dev, best_dev = _median_dev(ctx, prev, cur, 0, check, mc.SCENE_LIMIT)
    for e, b, what in ((ent, best, "sad_flow"), (ent_dev, best_dev, "median_dev")):
        assert len(e) == int(keep.sum()), f"{mode} {what}"
        np.testing.assert_array_equal(_bits(e), _bits(mc.filtered(e_ref, keep)), err_msg=f"{mode} {what}: records")
        np.testing.assert_array_equal(b, mc.filtered(b_ref, keep), err_msg=f"{mode} {what}: triples")
    if kw.get("scale") == 4:
        assert not np.array_equal(b_ref, F)              # quarter-pel triples went to the caller, integer winners to the test


# --------------------------------------------------------------------------------------------------------------- the fused path
def _prm(seed, use_ransac=False):
    return dict(block=B, search_range=R, detector=True, estimator=True, aspect=mc.SCENE_CAM[0], fov_y_deg=mc.SCENE_CAM[1], use_ransac=use_ransac,
                seed=seed, **mc.SCENE_DETECTOR, **mc.SCENE_RANSAC)


def _check_ticket(ctx, got, ent0, keep, seed, what):
    assert got["have"] and got["n"] == int(keep.sum()) == len(got["entries"]), what
    np.testing.assert_array_equal(_bits(got["entries"]), _bits(mc.filtered(ent0, keep)), err_msg=what + ": records")
    q = ctx.almeida(got["entries"], *mc.SCENE_CAM, use_ransac=False, seed=seed, **mc.SCENE_RANSAC)[0]
    want = ctx.detect(got["entries"], **mc.SCENE_DETECTOR)
    err = float(np.abs(got["quat"] - q).max())
    print(f"{what}: kept {got['n']}, quat {got['quat']} (|fused - almeida| {err:.3g}), area {gc.area_of(got['motion'])}")
    assert err <= QUAT_BOUND and np.isfinite(got["quat"]).all(), what
    assert (got["motion"] is None) == (want is None), what
    if want is not None:
        assert got["motion"][0] == want[0], what
        np.testing.assert_array_equal(_bits(got["motion"][1]), _bits(want[1]), err_msg=what + ": field")


def test_fused_ticket(ctx):
    prev, cur = mc.scene()
    with _settings(ctx):
        ctx.reset_frames()
        ctx.push_frame(prev, **_prm(mc.SCENE_SEED))
        plain = ctx.push_frame(cur, want_entries=True, want_field=True, **_prm(mc.SCENE_SEED + 1))
    with _settings(ctx, median=mc.SCENE_LIMIT):
        ctx.reset_frames()
        r0 = ctx.push_frame(prev, want_entries=True, **_prm(mc.SCENE_SEED))
        assert not r0["have_vectors"] and r0["motion"] is None
        np.testing.assert_array_equal(r0["quat"], IDENTITY)
        r = ctx.push_frame(cur, want_entries=True, want_field=True, **_prm(mc.SCENE_SEED + 1))
    ctx.reset_frames()
    assert plain["n_vectors"] == mc.SCENE_NBLK
    got = dict(have=r["have_vectors"], n=r["n_vectors"], entries=r["entries"], quat=r["quat"], motion=r["motion"])
    _check_ticket(ctx, got, mc.scene_vectors()[0], mc.scene_keep(), mc.SCENE_SEED + 1, "fused ticket")
    assert np.abs(r["quat"] - plain["quat"]).max() > 1e-5, "the estimator answered as without the test"


def test_fused_async_pair_of_tickets(ctx):
    """frames prev, cur, prev with two tickets in flight: the pairs (prev, cur) and (cur, prev)"""
    prev, cur = mc.scene()
    frames = (prev, cur, prev)
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
        with _settings(ctx, median=mc.SCENE_LIMIT, gate=1):
            ctx.reset_frames()
            for k in range(3):
                if k >= 2:
                    collect(k - 2)
                np.copyto(pins[k], frames[k])
                tickets.append(ctx.push_frame_async(pins[k], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(mc.SCENE_SEED + k)))
            collect(1)
            collect(2)
    finally:
        ctx.reset_frames()
        for p in pins + ents + flds:
            ctx.free_pinned(p)
    assert not out[0]["have"]
    for k, reverse in ((1, False), (2, True)):
        ent0, F = mc.scene_vectors(reverse)
        kin = gc.keep_flags(frames[k], B, 1).astype(np.uint8)                           # the gate reads the pair's CURRENT frame
        keep = im.keep_flags(F, kin, mc.SCENE_NBX, mc.SCENE_NBY, mc.SCENE_LIMIT)
        _check_ticket(ctx, out[k], ent0, keep, mc.SCENE_SEED + k, f"async ticket {k}")


def test_fewer_than_three_kept_records_give_the_identity(ctx):
    prev, cur, ent0, F = mc.sparse_pair()
    keep = im.keep_flags(F, None, mc.SPARSE_W // B, mc.SPARSE_H // B, 1)
    assert int(keep.sum()) == mc.SPARSE_KEPT < 3
    with _settings(ctx, median=1):
        ctx.reset_frames()
        ctx.push_frame(prev, **_prm(1))
        r = ctx.push_frame(cur, want_entries=True, want_field=True, **_prm(2))
        ent = ctx.sad_flow(prev, cur, B, R)
    ctx.reset_frames()
    assert r["have_vectors"] and r["n_vectors"] == mc.SPARSE_KEPT
    np.testing.assert_array_equal(_bits(r["entries"]), _bits(mc.filtered(ent0, keep)))
    np.testing.assert_array_equal(_bits(ent), _bits(mc.filtered(ent0, keep)))
    np.testing.assert_array_equal(r["quat"], IDENTITY)
    want = ctx.detect(r["entries"], **mc.SCENE_DETECTOR)
    assert (r["motion"] is None) == (want is None)


def test_limit_0_after_limit_2_equals_a_fresh_context(ctx):
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
    with _settings(ctx, median=mc.SCENE_LIMIT):
        on, on_sad = run(ctx)
    assert on["n_vectors"] == len(on_sad[0]) == int(mc.scene_keep().sum())
    assert ctx.get_sad_median() == 0
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


# --------------------------------------------------------------------------------------------------------------- errors, options, scope
def test_bad_limits_and_the_option(ctx):
    import torch
    from ofps_amd import _lib
    from ofps_amd.runtime import OfpsHipError
    lib = _lib.load()
    assert ctx.get_sad_median() == 0
    for bad in (-1, 256, 1 << 20):
        assert lib.ofps_hip_set_sad_median(ctx._h, bad) == EINVAL and ctx.get_sad_median() == 0
        assert str(bad) in lib.ofps_hip_last_error(ctx._h).decode()                     # the value is in the message
    for ok in (255, 1, 0):
        ctx.set_sad_median(ok)
        assert ctx.get_sad_median() == ok
    nbx, nby, best, _, _ = mc.quad_field()
    W, H = mc.field_frame(nbx, nby)
    for bad in (0, -1, 256):                             # the standalone forms: limit in [1, 255]
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_median(best, None, W, H, mc.BLOCK, bad)
        assert ei.value.code == EINVAL
    d = torch.zeros(96 * 64, dtype=torch.int32, device="cuda")                          # real device memory behind every pointer: these calls must
    torch.cuda.synchronize()                                                            # be refused before anything is enqueued, but are not trusted to
    p = d.data_ptr()
    for args in ((p, None, W, H, 65, 1, p, None),        # block outside [1, 64]
                 (0, None, W, H, 8, 1, p, None),         # null winners
                 (p, p + 4096, W, H, 8, 1, None, p + 4096)):     # the outgoing flags alias the incoming ones
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_median_dev(*args)
        assert ei.value.code == EINVAL, args
    for mp, limit, med in ((0, 0, 0), (0, 0, 256), (0, 0, -1), (-1, 0, 1), (65, 0, 1), (0, -1, 1), (0, 130, 1)):
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow_median_dev(p, p, 96, 64, 96, 8, 8, mp, limit, med, p, None, p)
        assert ei.value.code == EINVAL, (mp, limit, med)
    ctx.sync()
    ctx.set_option("OFPS_HIP_SAD_MEDIAN", 3)             # the option table sets the same field
    assert ctx.get_sad_median() == 3
    for bad in (-3, 256):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_MEDIAN", bad)
        assert ei.value.code == EINVAL and ctx.get_sad_median() == 3 and str(bad) in str(ei.value)
    ctx.set_option("OFPS_HIP_SAD_MEDIAN", None)
    assert ctx.get_sad_median() == 0


def test_batched_form_ignores_the_limit(ctx):
    import torch
    prev, cur = mc.scene()
    try:
        ctx.set_sad_median(mc.SCENE_LIMIT)
        d = torch.from_numpy(np.stack([prev, cur])).cuda()
        d_ent = torch.zeros((mc.SCENE_NBLK, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.sad_flow_dev(d.data_ptr(), 2, mc.SCENE_W, mc.SCENE_H, mc.SCENE_W, mc.SCENE_W * mc.SCENE_H, 0, B, R, d_ent.data_ptr())
        ctx.sync()
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()), _bits(mc.scene_vectors()[0]))          # nblk records
    finally:
        ctx.set_sad_median(0)


def test_plugin_property():
    from ofps_amd.plugins import HipSadDecoder
    prev, cur = mc.scene()
    dec = HipSadDecoder(iter([prev, cur, prev]))
    try:
        names = [p[0] for p in dec.props()]
        assert ("Median test", "usize", 0, 0, 255) in dec.props()
        assert names.index("Contrast gate") + 1 == names.index("Median test")
        assert dec.set_prop("Block size", B) and dec.set_prop("Search range", R)
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True and len(field) == mc.SCENE_NBLK
        assert dec.set_prop("Median test", mc.SCENE_LIMIT)
        field = []
        assert dec.process_frame(field) is True and dec.ctx.get_sad_median() == mc.SCENE_LIMIT
        keep = mc.scene_keep(reverse=True)
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(mc.filtered(mc.scene_vectors(reverse=True)[0], keep)))
    finally:
        dec.ctx.close()
