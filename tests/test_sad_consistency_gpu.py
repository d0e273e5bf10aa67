"""-m gpu: hip_sad's forward-backward consistency check (include/ofps_hip.h N1c) against the restatement of
tests/sad_consistency_cases.py.  Residuals, flags, records and winners are integers or copies: every equality is bit for bit.  The one
exception is the quaternion of the fused path's device-count form, held to the solver's documented parity with ofps_hip_almeida on the
same records: 2e-6 (least squares), 1e-4 (RANSAC).  tests/test_sad_consistency_cpu.py proves on the oracle that the inputs separate
check-on from check-off.

The kernel's optional AND input has no entry point of its own (ofps_hip_sad_consistency[_dev] take the two winner arrays only): it is
exercised, aliased with the output as the library uses it, by every case below that has the contrast gate on as well."""
import ctypes as C

import numpy as np
import pytest

import sad_consistency_cases as cc
import sad_gate_cases as gc

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1, 0, 0, 0], np.float32)
EINVAL = -1
QUAT_BOUND = {False: 2e-6, True: 1e-4}                   # by use_ransac


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

    def __init__(self, ctx, limit=0, gate=0, scale=1, comp=0, pruned=False):
        self.ctx, self.v = ctx, (limit, gate, scale, comp, pruned)

    def __enter__(self):
        limit, gate, scale, comp, pruned = self.v
        self.ctx.set_sad_consistency(limit); self.ctx.set_sad_gate(gate); self.ctx.set_sad_motion_scale(scale)
        self.ctx.set_detect_compensation(comp); self.ctx.set_sad_mode(self.ctx.SAD_PRUNED if pruned else self.ctx.SAD_EXHAUSTIVE)

    def __exit__(self, *exc):
        self.ctx.set_sad_consistency(0); self.ctx.set_sad_gate(0); self.ctx.set_sad_motion_scale(1)
        self.ctx.set_detect_compensation(0); self.ctx.set_sad_mode(self.ctx.SAD_EXHAUSTIVE)


# --------------------------------------------------------------------------------------------------------------- the kernel alone
def _check_kernel(ctx, W, H, B, F, G, limits=(1, 2, cc.LIMIT_MAX)):
    want = cc.residual(F, G, W, H, B)
    for limit in limits:
        w = f"{W}x{H} block {B} limit {limit}"
        res, keep = ctx.sad_consistency(F, G, W, H, B, limit)
        assert res.dtype == np.uint32 and keep.dtype == np.uint8 and len(res) == len(keep) == len(want), w
        np.testing.assert_array_equal(res, want, err_msg=w + ": residual")
        np.testing.assert_array_equal(keep, (want < limit).astype(np.uint8), err_msg=w + ": keep bytes")
    res, none = ctx.sad_consistency(F, G, W, H, B, 2, want_keep=False)                  # one output NULL, then the other
    assert none is None
    np.testing.assert_array_equal(res, want)
    none, keep = ctx.sad_consistency(F, G, W, H, B, 2, want_residual=False)
    assert none is None
    np.testing.assert_array_equal(keep, (want < 2).astype(np.uint8))


@pytest.mark.parametrize("block", cc.KERNEL_BLOCKS)
@pytest.mark.parametrize("lattice", cc.KERNEL_LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_on_synthetic_winners(ctx, lattice, block):
    for seed in (0, 3):                                  # another assignment of edges and corners to blocks
        W, H, F, G = cc.synthetic_winners(*lattice, block, seed=seed)
        _check_kernel(ctx, W, H, block, F, G)


def test_kernel_clamps_centres_in_the_ragged_margin(ctx):
    W, H, B, F, G, want = cc.ragged_winners()
    _check_kernel(ctx, W, H, B, F, G, limits=(1, 16, 17))
    res, keep = ctx.sad_consistency(F, G, W, H, B, 16)
    np.testing.assert_array_equal(res, want)
    np.testing.assert_array_equal(keep, [0, 1])          # residual 16 == limit: dropped
    W, H, F, G = cc.synthetic_winners(W // B, H // B, B, W, H)
    _check_kernel(ctx, W, H, B, F, G)


def test_kernel_dev_form_writes_nblk_outputs_and_no_more(ctx):
    import torch
    W, H, F, G = cc.synthetic_winners(65, 1, 8)
    n = len(F)
    d_f, d_g = torch.from_numpy(F.copy()).cuda(), torch.from_numpy(G.copy()).cuda()
    d_res = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")                 # 64 guard words / bytes behind the outputs
    d_keep = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.sad_consistency_dev(d_f.data_ptr(), d_g.data_ptr(), W, H, 8, 1, d_res.data_ptr(), d_keep.data_ptr())
    ctx.sync()
    want = cc.residual(F, G, W, H, 8)
    np.testing.assert_array_equal(d_res.cpu().numpy()[:n].view(np.uint32), want)
    np.testing.assert_array_equal(d_keep.cpu().numpy()[:n], (want < 1).astype(np.uint8))
    assert (d_res.cpu().numpy()[n:] == -1).all() and (d_keep.cpu().numpy()[n:] == 7).all()


# --------------------------------------------------------------------------------------------------------------- ofps_hip_sad_flow, checked
def _sad_flow(ctx, prev, cur, block, rng, stride=None):
    """ofps_hip_sad_flow with an explicit row stride (the runtime's wrapper always passes dense frames) -> (records, triples)"""
    H, W = prev.shape
    if stride is None:
        return ctx.sad_flow(prev, cur, block, rng, want_best=True)
    bufs = []
    for f in (prev, cur):
        b = np.full((H, stride), 255, np.uint8)          # whatever lies in the padding must not be read as luma
        b[:, :W] = f
        bufs.append(b)
    nb = (W // block) * (H // block)
    ent, best, n_out = np.zeros((nb, 4), np.float32), np.zeros((nb, 3), np.int32), C.c_size_t(0)
    u8 = C.POINTER(C.c_uint8)
    ctx._check(ctx._lib.ofps_hip_sad_flow(ctx._h, bufs[0].ctypes.data_as(u8), bufs[1].ctypes.data_as(u8), W, H, stride, block, rng,
                                          ent.ctypes.data_as(C.POINTER(C.c_float)), best.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out)))
    return ent[:n_out.value], best[:n_out.value]


PAIR_CASES = {  # id: (pair, block, range, stride, pinned count at LIMIT or None)
    "half_flat-8": ("half_flat", 8, gc.PAIR_RANGE, None, cc.HALF_FLAT_KEPT[8]),
    "half_flat-16": ("half_flat", 16, gc.PAIR_RANGE, None, cc.HALF_FLAT_KEPT[16]),
    "frames1": ("frames1", gc.BLOCK, gc.RANGE, None, cc.FRAMES_KEPT[1]),
    "frames2": ("frames2", gc.BLOCK, gc.RANGE, None, cc.FRAMES_KEPT[2]),
    "frames3": ("frames3", gc.BLOCK, gc.RANGE, None, cc.FRAMES_KEPT[3]),
    "half_flat-8-stride160": ("half_flat", 8, gc.PAIR_RANGE, 160, cc.HALF_FLAT_KEPT[8]),
    "generic-12": ("generic", cc.GENERIC_BLOCK, cc.GENERIC_RANGE, None, None),
}


@pytest.mark.parametrize("case", list(PAIR_CASES))
def test_checked_sad_flow_is_the_filtered_unchecked_output(ctx, case):
    name, block, rng, stride, pinned = PAIR_CASES[case]
    prev, cur, ent0, F, G = cc.pair_vectors(name, block, rng)
    H, W = cur.shape
    keep = cc.keep_flags(F, G, W, H, block, cc.LIMIT)
    if pinned is not None:
        assert int(keep.sum()) == pinned
    e_plain, b_plain = _sad_flow(ctx, prev, cur, block, rng, stride)                    # the unchecked call IS the oracle's output
    np.testing.assert_array_equal(_bits(e_plain), _bits(ent0))
    np.testing.assert_array_equal(b_plain, F)
    with _settings(ctx, limit=cc.LIMIT):
        ent, best = _sad_flow(ctx, prev, cur, block, rng, stride)
    assert len(ent) == len(best) == int(keep.sum()) < len(ent0), case                   # *n_out
    np.testing.assert_array_equal(_bits(ent), _bits(cc.check_filter(ent0, keep)), err_msg=case + ": records")
    np.testing.assert_array_equal(best, cc.check_filter(F, keep), err_msg=case + ": out_best")
    # other limits: 2, and the one that keeps every block
    with _settings(ctx, limit=2):
        ent2 = _sad_flow(ctx, prev, cur, block, rng, stride)[0]
    np.testing.assert_array_equal(_bits(ent2), _bits(cc.check_filter(ent0, cc.keep_flags(F, G, W, H, block, 2))), err_msg=case + ": limit 2")
    with _settings(ctx, limit=2 * rng + 1):
        ent_all = _sad_flow(ctx, prev, cur, block, rng, stride)[0]
    np.testing.assert_array_equal(_bits(ent_all), _bits(ent0), err_msg=case + ": limit 2 * range + 1 keeps all")
    # motion scale 4: the unchecked quarter-pel records and triples, filtered by the same INTEGER flags
    with _settings(ctx, scale=4):
        e4, b4 = _sad_flow(ctx, prev, cur, block, rng, stride)
    with _settings(ctx, limit=cc.LIMIT, scale=4):
        ent, best = _sad_flow(ctx, prev, cur, block, rng, stride)
    np.testing.assert_array_equal(_bits(ent), _bits(cc.check_filter(e4, keep)), err_msg=case + ": scale 4 records")
    np.testing.assert_array_equal(best, cc.check_filter(b4, keep), err_msg=case + ": scale 4 out_best")
    # with the contrast gate as well: kept iff both keep it
    both = keep & gc.keep_flags(cur, block, 1)
    for scale, e_ref, b_ref in ((1, ent0, F), (4, e4, b4)):
        with _settings(ctx, limit=cc.LIMIT, gate=1, scale=scale):
            ent, best = _sad_flow(ctx, prev, cur, block, rng, stride)
        assert len(ent) == int(both.sum())
        np.testing.assert_array_equal(_bits(ent), _bits(cc.check_filter(e_ref, both)), err_msg=f"{case}: gate 1, scale {scale}: records")
        np.testing.assert_array_equal(best, cc.check_filter(b_ref, both), err_msg=f"{case}: gate 1, scale {scale}: out_best")
    if name == "half_flat":
        assert int(both.sum()) == cc.HALF_FLAT_KEPT_WITH_GATE[block]


@pytest.mark.parametrize("scale", [1, 4])
def test_checked_sad_flow_in_pruned_mode(ctx, scale):
    prev, cur, ent0, F, G = cc.pair_vectors("pruned", cc.PRUNED_BLOCK, cc.PRUNED_RANGE)
    H, W = cur.shape
    keep = cc.keep_flags(F, G, W, H, cc.PRUNED_BLOCK, cc.LIMIT)
    with _settings(ctx, scale=scale, pruned=True):
        e_ref, b_ref = _sad_flow(ctx, prev, cur, cc.PRUNED_BLOCK, cc.PRUNED_RANGE)
    if scale == 1:
        np.testing.assert_array_equal(b_ref, F)
    with _settings(ctx, limit=cc.LIMIT, scale=scale, pruned=True):
        ent, best = _sad_flow(ctx, prev, cur, cc.PRUNED_BLOCK, cc.PRUNED_RANGE)
    assert len(ent) == int(keep.sum())
    np.testing.assert_array_equal(_bits(ent), _bits(cc.check_filter(e_ref, keep)))
    np.testing.assert_array_equal(best, cc.check_filter(b_ref, keep))


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("min_pixels", [0, 1])
def test_checked_dev_form(ctx, min_pixels, scale):
    import torch
    block = 8
    prev, cur, ent0, F, G = cc.pair_vectors("half_flat", block)
    nblk = len(F)
    keep = cc.keep_flags(F, G, gc.PAIR_W, gc.PAIR_H, block, cc.LIMIT)
    if min_pixels:
        keep = keep & gc.keep_flags(cur, block, min_pixels)
    with _settings(ctx, scale=scale):
        e_ref, b_ref = ctx.sad_flow(prev, cur, block, gc.PAIR_RANGE, want_best=True)
        d_prev, d_cur = torch.from_numpy(prev.copy()).cuda(), torch.from_numpy(cur.copy()).cuda()
        d_ent = torch.zeros((nblk, 4), dtype=torch.float32, device="cuda")
        d_best = torch.zeros((nblk, 3), dtype=torch.int32, device="cuda")
        d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ctx.get_sad_consistency() == 0 and ctx.get_sad_gate() == 0              # the device form takes its own values
        ctx.sad_flow_checked_dev(d_prev.data_ptr(), d_cur.data_ptr(), gc.PAIR_W, gc.PAIR_H, gc.PAIR_W, block, gc.PAIR_RANGE, min_pixels, cc.LIMIT,
                                 d_ent.data_ptr(), d_best.data_ptr(), d_cnt.data_ptr())
        ctx.sync()
        n = int(d_cnt.cpu().numpy()[0])
        assert n == int(keep.sum()) == (cc.HALF_FLAT_KEPT_WITH_GATE if min_pixels else cc.HALF_FLAT_KEPT)[block]
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()[:n]), _bits(cc.check_filter(e_ref, keep)))
        np.testing.assert_array_equal(d_best.cpu().numpy()[:n], cc.check_filter(b_ref, keep))
        d_cnt.fill_(-1); d_ent.zero_()
        torch.cuda.synchronize()
        ctx.sad_flow_checked_dev(d_prev.data_ptr(), d_cur.data_ptr(), gc.PAIR_W, gc.PAIR_H, gc.PAIR_W, block, gc.PAIR_RANGE, min_pixels, cc.LIMIT,
                                 d_ent.data_ptr(), None, d_cnt.data_ptr())             # without out_best
        ctx.sync()
        assert int(d_cnt.cpu().numpy()[0]) == n
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()[:n]), _bits(cc.check_filter(e_ref, keep)))


# --------------------------------------------------------------------------------------------------------------- the fused path
def _prm(use_ransac, seed, detector=True, estimator=True):
    return dict(block=gc.BLOCK, search_range=gc.RANGE, detector=detector, estimator=estimator, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1],
                use_ransac=use_ransac, seed=seed, **gc.FRAME_DETECTOR, **gc.FRAME_RANSAC)


def _sync_stream(ctx, use_ransac, frames=None, limits=None):
    """limits[k]: the context's limit when frame k is pushed (None: leave it alone)"""
    ctx.reset_frames()
    f = gc.frames() if frames is None else frames
    out = []
    for k in range(len(f)):
        if limits is not None:
            ctx.set_sad_consistency(limits[k])
        r = ctx.push_frame(f[k], want_entries=True, want_field=True, **_prm(use_ransac, gc.SEED + k))
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=r["entries"], quat=r["quat"], motion=r["motion"]))
    return out


def _async_stream(ctx, use_ransac, frames=None, limits=None):
    """two tickets in flight"""
    assert frames is None
    ctx.reset_frames()
    f = gc.frames()
    dim = ctx.block_dim(gc.FRAME_DETECTOR["min_size"], gc.FRAME_DETECTOR["subdivide"])
    pins = [ctx.pinned_frame(gc.FRAME_H, gc.FRAME_W) for _ in range(3)]
    ents = [ctx.pinned_array((gc.NBLK, 4)) for _ in range(2)]
    flds = [ctx.pinned_array((dim, dim, 2)) for _ in range(2)]
    out, tickets = [], []

    def collect(k):
        r = ctx.frame_wait(tickets[k])
        m = None if r["motion"] is None else (r["motion"][0], flds[k % 2].copy())
        out.append(dict(have=r["have_vectors"], n=r["n_vectors"], entries=ents[k % 2][:r["n_vectors"]].copy() if r["have_vectors"] else None,
                        quat=r["quat"], motion=m))

    for k in range(gc.N_FRAMES):
        if k >= 2:
            collect(k - 2)
        if limits is not None:
            ctx.set_sad_consistency(limits[k])
        np.copyto(pins[k % 3], f[k])
        tickets.append(ctx.push_frame_async(pins[k % 3], out_entries=ents[k % 2], out_field=flds[k % 2], **_prm(use_ransac, gc.SEED + k)))
    collect(gc.N_FRAMES - 2)
    collect(gc.N_FRAMES - 1)
    for p in pins + ents + flds:
        ctx.free_pinned(p)
    return out


RUN = {"sync": _sync_stream, "async": _async_stream}


def _same_motion(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a[0] == b[0], what
        np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what + ": field")


def _check_fused(ctx, ref, got, use_ransac, comp, gate, scale, what):
    """ref: the unchecked, ungated stream at the same motion scale; got: the checked one"""
    assert not got[0]["have"] and got[0]["motion"] is None
    np.testing.assert_array_equal(got[0]["quat"], IDENTITY)
    for k in range(1, gc.N_FRAMES):
        w = f"{what} frame {k}"
        keep = cc.frame_keep(k, cc.LIMIT, gate)
        literal = (cc.FRAMES_KEPT_WITH_GATE if gate else cc.FRAMES_KEPT)[k]
        assert got[k]["have"] and got[k]["n"] == literal == int(keep.sum()) == len(got[k]["entries"]), w
        assert ref[k]["n"] == gc.NBLK, w
        if scale == 1:
            np.testing.assert_array_equal(_bits(ref[k]["entries"]), _bits(gc.frame_vectors(k)[0]), err_msg=w + ": the unchecked records")
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(cc.check_filter(ref[k]["entries"], keep)), err_msg=w + ": records")
        q = ctx.almeida(got[k]["entries"], *gc.FRAME_CAM, use_ransac=use_ransac, seed=gc.SEED + k, **gc.FRAME_RANSAC)[0]
        det_in = ctx.compensate(got[k]["entries"], *gc.FRAME_CAM, got[k]["quat"]) if comp else got[k]["entries"]
        want = ctx.detect(det_in, **gc.FRAME_DETECTOR)
        err = float(np.abs(got[k]["quat"] - q).max())
        a1, a0 = gc.area_of(got[k]["motion"]), gc.area_of(ref[k]["motion"])
        print(f"{w}: kept {got[k]['n']}, quat {got[k]['quat']} (|fused - almeida| {err:.3g}), area unchecked {a0}, checked {a1}, detect {gc.area_of(want)}")
        assert err <= QUAT_BOUND[use_ransac], w
        assert np.isfinite(got[k]["quat"]).all(), w
        _same_motion(got[k]["motion"], want, w)
        if not use_ransac:
            assert np.abs(got[k]["quat"] - ref[k]["quat"]).max() > 1e-4, w + ": the estimator answered as without the check"
        if not comp:
            assert a1 != a0, w + ": the detector answered as without the check"


FUSED_CASES = {  # id: (form, use_ransac, comp, gate, scale)
    "sync-lsq": ("sync", False, 0, 0, 1), "sync-ransac": ("sync", True, 0, 0, 1),
    "async-lsq": ("async", False, 0, 0, 1), "async-ransac": ("async", True, 0, 0, 1),
    "sync-lsq-comp1": ("sync", False, 1, 0, 1), "async-lsq-comp1": ("async", False, 1, 0, 1),
    "sync-lsq-gate": ("sync", False, 0, gc.GATE, 1), "async-ransac-gate": ("async", True, 0, gc.GATE, 1),
    "sync-lsq-scale4": ("sync", False, 0, 0, 4), "async-lsq-scale4-gate-comp1": ("async", False, 1, gc.GATE, 4),
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_fused_checked_stream(ctx, case):
    form, use_ransac, comp, gate, scale = FUSED_CASES[case]
    assert ctx.get_sad_consistency() == 0 and ctx.get_sad_gate() == 0
    with _settings(ctx, scale=scale, comp=comp):
        ref = RUN[form](ctx, use_ransac)
    with _settings(ctx, limit=cc.LIMIT, gate=gate, scale=scale, comp=comp):
        assert ctx.get_sad_consistency() == cc.LIMIT
        got = RUN[form](ctx, use_ransac)
    assert len(got) == gc.N_FRAMES
    _check_fused(ctx, ref, got, use_ransac, comp, gate, scale, case)


def test_limit_switch_between_tickets_in_flight(ctx):
    """frames 0, 1 pushed at limit 1, frame 2 at 0, frame 3 at 2, two tickets in flight: a ticket follows the limit of its push"""
    try:
        ref0 = _async_stream(ctx, False, limits=[0, 0, 0, 0])
        ref1 = _async_stream(ctx, False, limits=[1, 1, 1, 1])
        ref2 = _async_stream(ctx, False, limits=[2, 2, 2, 2])
        got = _async_stream(ctx, False, limits=[1, 1, 0, 2])
    finally:
        ctx.set_sad_consistency(0)
    for k, want in ((1, ref1), (2, ref0), (3, ref2)):
        assert got[k]["n"] == want[k]["n"]
        np.testing.assert_array_equal(_bits(got[k]["entries"]), _bits(want[k]["entries"]))
        np.testing.assert_array_equal(_bits(got[k]["quat"]), _bits(want[k]["quat"]))
        _same_motion(got[k]["motion"], want[k]["motion"], f"frame {k}")
    assert got[1]["n"] == cc.FRAMES_KEPT[1] and got[2]["n"] == gc.NBLK
    assert got[3]["n"] == int(cc.frame_keep(3, 2).sum()) > cc.FRAMES_KEPT[3]


@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
def test_flat_frame_twice(ctx, use_ransac):
    """a clean flat pair round-trips exactly: the check alone keeps all 240 (that is the contrast gate's job: with it, none -> identity, no motion)"""
    flat = gc.flat_frame()
    with _settings(ctx, limit=cc.LIMIT):
        got = _sync_stream(ctx, use_ransac, frames=[flat, flat])
    assert got[1]["have"] and got[1]["n"] == gc.NBLK
    with _settings(ctx):
        plain = _sync_stream(ctx, use_ransac, frames=[flat, flat])
    np.testing.assert_array_equal(_bits(got[1]["entries"]), _bits(plain[1]["entries"]))
    for comp in (0, 1):
        with _settings(ctx, limit=cc.LIMIT, gate=gc.GATE, comp=comp):
            got = _sync_stream(ctx, use_ransac, frames=[flat, flat])
        assert got[1]["have"] and got[1]["n"] == 0 and got[1]["entries"].shape == (0, 4) and got[1]["motion"] is None, comp
        np.testing.assert_array_equal(got[1]["quat"], IDENTITY)


def test_limit_0_after_limit_1_equals_a_fresh_context(ctx):
    from ofps_amd.runtime import HipContext
    prev, cur = gc.half_flat_pair()
    fresh = HipContext(0)
    try:
        ref = _sync_stream(fresh, False)                                   # a context that never saw the check
        ref_sad = fresh.sad_flow(prev, cur, 8, gc.PAIR_RANGE, want_best=True)
    finally:
        fresh.close()
    with _settings(ctx, limit=cc.LIMIT):
        checked = _sync_stream(ctx, False)
        assert len(ctx.sad_flow(prev, cur, 8, gc.PAIR_RANGE)) == cc.HALF_FLAT_KEPT[8]
    assert checked[1]["n"] == cc.FRAMES_KEPT[1]
    assert ctx.get_sad_consistency() == 0
    again = _sync_stream(ctx, False)
    again_sad = ctx.sad_flow(prev, cur, 8, gc.PAIR_RANGE, want_best=True)
    np.testing.assert_array_equal(_bits(again_sad[0]), _bits(ref_sad[0]))
    np.testing.assert_array_equal(again_sad[1], ref_sad[1])
    for k in range(1, gc.N_FRAMES):
        assert again[k]["n"] == gc.NBLK
        np.testing.assert_array_equal(_bits(again[k]["entries"]), _bits(ref[k]["entries"]))
        np.testing.assert_array_equal(_bits(again[k]["quat"]), _bits(ref[k]["quat"]))
        _same_motion(again[k]["motion"], ref[k]["motion"], f"limit 0 again, frame {k}")


# --------------------------------------------------------------------------------------------------------------- errors, options, scope
def test_bad_limits_and_the_option(ctx):
    from ofps_amd import _lib
    from ofps_amd.runtime import OfpsHipError
    lib = _lib.load()
    assert ctx.get_sad_consistency() == 0
    for bad in (-1, 130, 1 << 20):
        assert lib.ofps_hip_set_sad_consistency(ctx._h, bad) == EINVAL and ctx.get_sad_consistency() == 0
    for ok in (129, 1, 0):
        ctx.set_sad_consistency(ok)
        assert ctx.get_sad_consistency() == ok
    W, H, F, G = cc.synthetic_winners(3, 2, 8)
    for bad in (0, -1, 130):                             # the standalone forms: limit in [1, 129]
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_consistency(F, G, W, H, 8, bad)
        assert ei.value.code == EINVAL
    import torch
    d = torch.zeros(96 * 64, dtype=torch.int32, device="cuda")                          # real device memory behind every pointer: these calls must
    torch.cuda.synchronize()                                                            # be refused before anything is enqueued, but are not trusted to
    p = d.data_ptr()
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_consistency_dev(p, p, W, H, 65, 1, p, None)                             # block outside [1, 64]
    assert ei.value.code == EINVAL
    with pytest.raises(OfpsHipError) as ei:
        ctx.sad_consistency_dev(0, 0, W, H, 8, 1, p, None)                              # null winners
    assert ei.value.code == EINVAL
    for mp, limit in ((0, 0), (0, 130), (-1, 1), (65, 1)):                              # checked_dev: limit in [1, 129]; min_pixels 0 or in [1, B * B]
        with pytest.raises(OfpsHipError) as ei:
            ctx.sad_flow_checked_dev(p, p, 96, 64, 96, 8, 8, mp, limit, p, None, p)
        assert ei.value.code == EINVAL, (mp, limit)
    ctx.sync()
    ctx.set_option("OFPS_HIP_SAD_CONSISTENCY", 3)        # the option table sets the same field
    assert ctx.get_sad_consistency() == 3
    for bad in (-3, 130):
        with pytest.raises(OfpsHipError) as ei:
            ctx.set_option("OFPS_HIP_SAD_CONSISTENCY", bad)
        assert ei.value.code == EINVAL and ctx.get_sad_consistency() == 3
    ctx.set_option("OFPS_HIP_SAD_CONSISTENCY", None)
    assert ctx.get_sad_consistency() == 0


def test_batched_forms_ignore_the_limit(ctx):
    import torch
    f = gc.frames()
    try:
        ctx.set_sad_consistency(cc.LIMIT)
        ctx.reset_frames()
        buf = ctx.pinned_array((3, gc.FRAME_H, gc.FRAME_W), np.uint8)
        ents = ctx.pinned_array((3, gc.NBLK, 4))
        np.copyto(buf, f[:3])
        res = ctx.frames_wait(ctx.push_frames_async(buf, out_entries=ents, **_prm(False, gc.SEED)))
        assert [r["n_vectors"] for r in res] == [0, gc.NBLK, gc.NBLK]
        for k in (1, 2):
            np.testing.assert_array_equal(_bits(ents[k]), _bits(gc.frame_vectors(k)[0]))
        ctx.free_pinned(buf); ctx.free_pinned(ents)
        d = torch.from_numpy(f[:2].copy()).cuda()
        d_ent = torch.zeros((gc.NBLK, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.sad_flow_dev(d.data_ptr(), 2, gc.FRAME_W, gc.FRAME_H, gc.FRAME_W, gc.FRAME_W * gc.FRAME_H, 0, gc.BLOCK, gc.RANGE, d_ent.data_ptr())
        ctx.sync()
        np.testing.assert_array_equal(_bits(d_ent.cpu().numpy()), _bits(gc.frame_vectors(1)[0]))
    finally:
        ctx.set_sad_consistency(0)
        ctx.reset_frames()


def test_plugin_property(ctx):
    from ofps_amd.plugins import HipSadDecoder
    f = gc.frames()
    dec = HipSadDecoder(iter(f))
    try:
        assert ("Consistency check", "usize", 0, 0, 129) in dec.props()
        assert dec.set_prop("Search range", gc.RANGE)      # the decoder's default is 16; the cases' oracle vectors are range 8
        field = []
        assert dec.process_frame(field) is False
        assert dec.process_frame(field) is True and len(field) == gc.NBLK
        assert dec.set_prop("Consistency check", cc.LIMIT)
        field = []
        assert dec.process_frame(field) is True and len(field) == cc.FRAMES_KEPT[2]
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(cc.check_filter(gc.frame_vectors(2)[0], cc.frame_keep(2))))
        assert dec.set_prop("Contrast gate", gc.GATE)       # applied per frame, like the gate, and together with it
        field = []
        assert dec.process_frame(field) is True and len(field) == cc.FRAMES_KEPT_WITH_GATE[3]
        np.testing.assert_array_equal(_bits(np.array(field)), _bits(cc.check_filter(gc.frame_vectors(3)[0], cc.frame_keep(3, cc.LIMIT, gc.GATE))))
    finally:
        dec.ctx.close()
