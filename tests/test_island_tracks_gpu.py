"""-m gpu: the island tracks (include/ofps_hip.h A5t; ofps_amd/csrc/detect_tracks.hip) through the C ABI, on the cases of
tests/island_track_cases.py against the plain-Python restatement tests/indep_island_tracks.py (proved on the CPU by
tests/test_island_tracks_cpu.py).  Rows below `rows`, track_counts and the state bytes: everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
import detect_islands_cases as ic
import indep_detect_islands as isl_indep
import indep_island_tracks as indep
import island_track_cases as tc

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = 64
I32P = C.POINTER(C.c_int32)
F32P = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------------- ofps_hip_detect_tracks
def _tracks_raw(ctx, frames, prm, K, T, reach, G, state=None, want_labels=True):
    """ofps_hip_detect_tracks itself, guard words behind every output -> ([(counts, table, labels, track_counts, rows), ...], state bytes)"""
    e = np.ascontiguousarray(np.stack([np.asarray(f, np.float32).reshape(-1, 4) for f in frames]))
    batch, n = e.shape[0], e.shape[1]
    d = ctx.block_dim(prm["min_size"], prm["subdivide"])
    nbytes = ctx.island_tracker_bytes(d, T)
    assert nbytes == indep.state_size(d, T)
    st = np.full(nbytes + GUARD, 0x5A, np.uint8)
    st[:nbytes] = np.frombuffer(state, np.uint8) if state is not None else 0
    counts = np.full(4 * batch + GUARD, -7, np.int32)
    table = np.full(8 * K * batch + GUARD, -7, np.int32)
    labels = np.full(d * d * batch + GUARD, 0x7777, np.uint16)
    tcounts = np.full(4 * batch + GUARD, -7, np.int32)
    rows = np.full(8 * T * batch + GUARD, -7, np.int32)
    ctx._check(ctx._lib.ofps_hip_detect_tracks(ctx._h, e.ctypes.data_as(F32P), n, batch, prm["min_size"], prm["subdivide"], prm["target_motion"], K, T,
                                               reach, G, C.c_void_p(st.ctypes.data), counts.ctypes.data_as(I32P), table.ctypes.data_as(I32P),
                                               C.c_void_p(labels.ctypes.data) if want_labels else None, tcounts.ctypes.data_as(I32P),
                                               rows.ctypes.data_as(I32P)))
    assert (st[nbytes:] == 0x5A).all() and (counts[4 * batch:] == -7).all() and (table[8 * K * batch:] == -7).all() and \
        (labels[d * d * batch:] == 0x7777).all() and (tcounts[4 * batch:] == -7).all() and (rows[8 * T * batch:] == -7).all(), "guard words"
    if not want_labels:
        assert (labels == 0x7777).all()
    out = [(counts[4 * j:4 * j + 4].copy(), table[8 * K * j:8 * K * (j + 1)].reshape(K, 8).copy(), labels[d * d * j:d * d * (j + 1)].reshape(d, d).copy(),
            tcounts[4 * j:4 * j + 4].copy(), rows[8 * T * j:8 * T * (j + 1)].reshape(T, 8).copy()) for j in range(batch)]
    return out, st[:nbytes].tobytes()


def _same(got, want, what, labels=True):
    """frames of (counts, table, labels, track_counts, rows): rows below n_listed / rows only"""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        at = f"{what}: frame {k}"
        assert g[0].tolist() == w[0].tolist(), at
        n = int(w[0][3])
        np.testing.assert_array_equal(g[1][:n], w[1][:n], err_msg=at + ": table")
        if labels:
            np.testing.assert_array_equal(g[2], w[2], err_msg=at + ": labels")
        assert g[3].tolist() == w[3].tolist(), at + f": track_counts {g[3].tolist()} != {w[3].tolist()}"
        r = int(w[3][0])
        np.testing.assert_array_equal(g[4][:r], w[4][:r], err_msg=at + ": tracks")


def _same_state(got, want, what):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    assert len(g) == len(w), what
    bad = np.flatnonzero(g != w)
    assert not len(bad), f"{what}: state bytes differ at {bad[:8].tolist()} ({len(bad)} in all)"


def _against_the_restatement(ctx, frames, prm, K, T, reach, G, what):
    want, want_state = tc.reference(tuple(frames), prm, K, T, reach, G)
    got, state = _tracks_raw(ctx, frames, prm, K, T, reach, G)
    _same(got, want, what)
    _same_state(state, want_state, what)
    return got, state


@pytest.mark.parametrize("h", tc.HAND, ids=lambda h: h.name)
def test_hand_derived_sequences(ctx, h):
    got, _ = _against_the_restatement(ctx, tc.hand_frames(h), tc.PRM8, tc.K8, h.T, h.reach, h.G, h.name)
    for k, (g, want) in enumerate(zip(got, h.want)):
        assert g[3][0] == len(want) and [tuple(int(v) for v in r[:4]) for r in g[4][:len(want)]] == want, (h.name, k)


# sides up to 17: every (reach, G); the large sides cost the restatement a flood fill of up to 25,600 cells per frame: the corners and the middle
@pytest.mark.parametrize("d,reach,G", [(d, r, g) for d in tc.RANDOM_SIDES_GPU for r, g in (tc.REACH_GAP if d <= 17 else ((0, 0), (1, 1), (4, 3)))])
def test_random_sequences(ctx, d, reach, G):
    frames, prm = tc.random_sequence(d), tc.params_of(d)
    assert ctx.block_dim(prm["min_size"], prm["subdivide"]) == d
    got, _ = _against_the_restatement(ctx, frames, prm, tc.RANDOM_K, tc.RANDOM_T, reach, G, f"random {d} reach {reach} gap {G}")
    if d >= 14:
        assert max(int(g[3][1]) for g in got) >= 2 and max(int(g[4][:g[3][0], 3].max(initial=0)) for g in got) >= 2, "something was followed"


def test_cut_independence_and_a_state_of_zeros(ctx):
    d, reach, G = 17, 1, 1
    frames, prm = tc.random_sequence(d), tc.params_of(d)
    K, T = tc.RANDOM_K, tc.RANDOM_T
    whole, state = _against_the_restatement(ctx, frames, prm, K, T, reach, G, "one call")
    st, got = None, []
    for e in frames:
        o, st = _tracks_raw(ctx, [e], prm, K, T, reach, G, st)
        got += o
    _same(got, whole, "12 calls")
    _same_state(st, state, "12 calls")
    a, st = _tracks_raw(ctx, frames[:5], prm, K, T, reach, G)
    b, st = _tracks_raw(ctx, frames[5:], prm, K, T, reach, G, st)
    _same(a + b, whole, "5 + 7")
    _same_state(st, state, "5 + 7")
    # labels are optional
    c, st = _tracks_raw(ctx, frames, prm, K, T, reach, G, want_labels=False)
    _same(c, whole, "no labels", labels=False)
    _same_state(st, state, "no labels")


# ------------------------------------------------------------------------------------------------------------------------ side 160 and T = 256
PRM160 = dc.params(ic.pair_area1(160))


def test_lattice_160_with_256_slots_and_with_one(ctx):
    # 6,400 tied islands of one cell, twice: the first 256 ranks (the first 256 seeds) are followed, the rest are not
    e = dc.entries(160, dc.lattice(160))
    for T in (256, 1):
        got, _ = _against_the_restatement(ctx, [e, e], PRM160, 6400, T, 0, 0, f"lattice T={T}")
        assert got[0][0][3] == 6400 and got[1][3].tolist() == [T, T, T, 2]
        assert got[1][4][:T, 0].tolist() == list(range(1, T + 1)) and (got[1][4][:T, 3] == 2).all()


def test_one_island_over_its_own_footprint_at_reach_4(ctx):
    # the atomics' worst case: every cell of the grid counts its whole window against one owner
    e = dc.entries(160, dc.all_on(160), motion=(0.02, -0.01))
    got, _ = _against_the_restatement(ctx, [e, e], PRM160, 4, 4, 4, 0, "full grid")
    assert got[1][3].tolist() == [1, 1, 1, 2] and got[1][4][0, :4].tolist() == [1, 0, 2, 2]
    mx, my = indep.sums_of(got[1][4][:1])
    assert int(mx[0]) == 25600 * indep.q(0.02) and int(my[0]) == 25600 * indep.q(-0.01)


@pytest.mark.parametrize("G", (0, 255))
def test_full_grid_alternating_with_an_empty_one(ctx, G):
    full, empty = dc.entries(160, dc.all_on(160)), dc.entries(160, [])
    got, state = _against_the_restatement(ctx, [full, empty, full, empty], PRM160, 4, 4, 0, G, f"alternating G={G}")
    assert got[2][4][0, :4].tolist() == ([2, 0, 1, 1] if G == 0 else [1, 0, 3, 2])
    assert got[3][3].tolist() == ([0, 0, 0, 4] if G == 0 else [0, 0, 1, 4])
    if G == 0:
        assert not any(state[16:]), "freed slots and cleared cells are zero bytes"


def test_256_slots_and_300_islands(ctx):
    d = 64
    prm = dc.params(ic.pair_area1(d))
    cells = dc.lattice(d)[:300]
    moved = [(x + 1, y) for x, y in cells]
    frames = [dc.entries(d, cells), dc.entries(d, moved), dc.entries(d, cells[40:])]
    got, _ = _against_the_restatement(ctx, frames, prm, 512, 256, 1, 1, "300 islands")
    assert got[0][0][3] == 300 and got[0][3].tolist() == [256, 256, 256, 1]
    assert got[2][0][3] == 260 and got[2][3][0] == 256


# ---------------------------------------------------------------------------------------------------------- ofps_hip_track_islands_dev, batched
def _dev_inputs(frames, prm, K):
    """the restatement's island lists as the device form's inputs"""
    per = []
    for e in frames:
        isl = isl_indep.islands(e, **prm)
        counts, table, labels, _ = isl_indep.listed(isl, K)
        tab = np.zeros((K, 8), np.int32)
        tab[:len(table)] = table
        per.append((counts, tab, labels, isl.field))
    return per


@pytest.mark.parametrize("with_cells", (True, False), ids=("cells", "null-cells"))
def test_track_islands_dev_batches(ctx, with_cells):
    import torch
    d, reach, G = 17, 1, 1
    frames, prm = tc.random_sequence(d), tc.params_of(d)
    K, T = tc.RANDOM_K, tc.RANDOM_T
    want, want_state = tc.reference(frames, prm, K, T, reach, G, with_cells)
    per = _dev_inputs(frames, prm, K)
    nbytes = indep.state_size(d, T)

    def run(cuts):
        d_state = torch.zeros(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        d_state[nbytes:] = 0x5A
        got, at = [], 0
        for b in cuts:
            items = per[at:at + b]
            at += b
            d_cnt = torch.from_numpy(np.concatenate([p[0] for p in items])).cuda()
            d_tab = torch.from_numpy(np.concatenate([p[1].reshape(-1) for p in items])).cuda()
            d_lab = torch.from_numpy(np.concatenate([p[2].reshape(-1) for p in items]).view(np.int16)).cuda()
            d_fld = torch.from_numpy(np.concatenate([p[3].reshape(-1) for p in items])).cuda()
            d_tc = torch.full((4 * b + GUARD,), -7, dtype=torch.int32, device="cuda")
            d_rows = torch.full((8 * T * b + GUARD,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.track_islands_dev(d_cnt.data_ptr(), d_tab.data_ptr(), d_lab.data_ptr(), d_fld.data_ptr() if with_cells else None, d, K, b, T, reach, G,
                                  d_state.data_ptr(), d_tc.data_ptr(), d_rows.data_ptr())
            ctx.sync()
            tcn, rows = d_tc.cpu().numpy(), d_rows.cpu().numpy()
            assert (tcn[4 * b:] == -7).all() and (rows[8 * T * b:] == -7).all(), "guard words"
            for j in range(b):
                got.append((items[j][0], items[j][1], items[j][2], tcn[4 * j:4 * j + 4], rows[8 * T * j:8 * T * (j + 1)].reshape(T, 8)))
        st = d_state.cpu().numpy()
        assert (st[nbytes:] == 0x5A).all(), "guard bytes behind the state"
        return got, st[:nbytes].tobytes()

    for cuts in ((12,), (1,) * 12, (2,) * 6, (5, 7)):
        got, st = run(cuts)
        _same(got, want, f"_dev cut {cuts}")
        _same_state(st, want_state, f"_dev cut {cuts}")
    if not with_cells:
        assert all(not g[4][:, 4:].any() for g in want), "no field, no motion sums"


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    import torch
    from ofps_amd.runtime import OfpsHipError
    h = tc.HAND_BY_NAME["B"]
    frames = tc.hand_frames(h)

    def refused(call, word):
        with pytest.raises(OfpsHipError) as ei:
            call()
        assert ei.value.code == EINVAL and word in str(ei.value), str(ei.value)

    for T, reach, G, K, word in ((0, 0, 0, 8, "max_tracks"), (257, 0, 0, 8, "max_tracks"), (4, -1, 0, 8, "reach"), (4, 5, 0, 8, "reach"), (4, 0, -1, 8, "max_gap"),
                                 (4, 0, 256, 8, "max_gap"), (4, 0, 0, 0, "max_islands"), (4, 0, 0, 6401, "max_islands")):
        refused(lambda: ctx.detect_tracks(frames, max_islands=K, max_tracks=T, reach=reach, max_gap=G, **tc.PRM8), word)
    refused(lambda: ctx.detect_tracks(frames, dc.SIDE_161[0], dc.SIDE_161[1], dc.TARGET), "161")
    z = np.zeros(64, np.int32)
    lib = ctx._lib
    assert lib.ofps_hip_detect_tracks(ctx._h, frames[0].ctypes.data_as(F32P), 64, 1, tc.PRM8["min_size"], 1, tc.PRM8["target_motion"], 8, 4, 0, 0, None,
                                      z.ctypes.data_as(I32P), z.ctypes.data_as(I32P), None, z.ctypes.data_as(I32P), z.ctypes.data_as(I32P)) == EINVAL
    # the device form: every range, dim, a null state -- before anything is enqueued
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    ok = dict(dim=8, max_islands=8, batch=1, max_tracks=4, reach=0, max_gap=0)
    for key, bad, word in (("dim", 0, "dim"), ("dim", 161, "dim"), ("max_tracks", 0, "max_tracks"), ("max_tracks", 257, "max_tracks"), ("reach", 5, "reach"),
                           ("reach", -1, "reach"), ("max_gap", 256, "max_gap"), ("max_gap", -1, "max_gap"), ("max_islands", 0, "max_islands"),
                           ("batch", 0, "batch")):
        a = dict(ok, **{key: bad})
        refused(lambda: ctx.track_islands_dev(p, p, p, None, a["dim"], a["max_islands"], a["batch"], a["max_tracks"], a["reach"], a["max_gap"], p, p, p), word)
    refused(lambda: ctx.track_islands_dev(p, p, p, None, 8, 8, 1, 4, 0, 0, None, p, p), "null state")
    ctx.sync()
    assert not buf.cpu().numpy().any(), "nothing was enqueued"
    # the setter, the getter and the options
    assert ctx.get_detect_tracks() == {"max_tracks": 0, "reach": 1, "max_gap": 2}
    for args in ((-1, 0, 0), (257, 0, 0), (4, 5, 0), (4, -1, 0), (4, 0, 256), (4, 0, -1)):
        refused(lambda: ctx.set_detect_tracks(*args), "set_detect_tracks")
    ctx.set_option("OFPS_HIP_DETECT_TRACKS", 5)
    ctx.set_option("OFPS_HIP_DETECT_TRACK_REACH", 3)
    ctx.set_option("OFPS_HIP_DETECT_TRACK_GAP", 9)
    assert ctx.get_detect_tracks() == {"max_tracks": 5, "reach": 3, "max_gap": 9}
    for name, bad in (("OFPS_HIP_DETECT_TRACKS", 257), ("OFPS_HIP_DETECT_TRACK_REACH", 5), ("OFPS_HIP_DETECT_TRACK_GAP", 256)):
        with pytest.raises(OfpsHipError):
            ctx.set_option(name, bad)
        ctx.set_option(name, None)
    assert ctx.get_detect_tracks() == {"max_tracks": 0, "reach": 1, "max_gap": 2}
    # a ticket pushed with T = 0 has no tracks
    ctx.reset_frames()
    ctx.set_detect_islands(4)
    try:
        for k in range(2):
            r = ctx.push_frame(tc.frames()[k], **tc.FUSED)
            assert "islands" in r and "tracks" not in r
        refused(lambda: ctx.frame_tracks(0), "max_tracks 0")
    finally:
        ctx.set_detect_islands(0)


# ------------------------------------------------------------------------------------------------------------------------ the fused forms
NBLK = (tc.FW // tc.BLOCK) * (tc.FH // tc.BLOCK)
DET = {k: tc.FUSED[k] for k in ("min_size", "subdivide", "target_motion")}
K_F, T_F, REACH_F, GAP_F = 16, 8, 1, 2
N = tc.N_FUSED


class _Settings:
    def __init__(self, ctx, K=K_F, T=T_F, reach=REACH_F, gap=GAP_F):
        self.ctx, self.a = ctx, (K, T, reach, gap)

    def __enter__(self):
        self.ctx.set_detect_islands(self.a[0])
        self.ctx.set_detect_tracks(*self.a[1:])

    def __exit__(self, *exc):
        self.ctx.set_detect_islands(0)
        self.ctx.set_detect_tracks(0)


def _table(trk):
    return np.array([trk["rows"], trk["n_tracked"], trk["n_live"], trk["t"]]), trk["table"]


def _expect_from_records(ctx, records):
    """ofps_hip_detect_tracks on the tickets' records, one frame a call, from a fresh state -> [(track_counts, rows)]"""
    st, out = None, []
    for e in records:
        o, st = _tracks_raw(ctx, [e], DET, K_F, T_F, REACH_F, GAP_F, st)
        out.append((o[0][3], o[0][4][:o[0][3][0]]))
    return out


def _same_tracks(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        c, t = _table(g)
        assert c.tolist() == w[0].tolist(), f"{what}: frame {k}: track_counts {c.tolist()} != {w[0].tolist()}"
        np.testing.assert_array_equal(t, w[1], err_msg=f"{what}: frame {k}: tracks")


def _no_step(trk):
    return trk["rows"] == 0 and trk["n_tracked"] == 0 and trk["n_live"] == 0 and trk["t"] == 0


@pytest.fixture(scope="module")
def sync_run(ctx):
    """the ten frames through ofps_hip_push_frame: the dicts, and what ofps_hip_detect_tracks says on the same records"""
    ctx.reset_frames()
    with _Settings(ctx):
        out = [ctx.push_frame(tc.frames()[k], want_entries=True, **tc.FUSED) for k in range(N)]
    want = _expect_from_records(ctx, [r["entries"] for r in out[1:]])
    return out, want


def test_push_frame(ctx, sync_run):
    out, want = sync_run
    assert not out[0]["have_vectors"] and _no_step(out[0]["tracks"]), "a first frame takes no step"
    _same_tracks([r["tracks"] for r in out[1:]], want, "push_frame")
    # the planted rectangles: two tracks that live through the crossing, no id handed out twice, motion of opposite sign
    first = out[1]["tracks"]
    assert first["rows"] >= 2 and first["id"][:2].tolist() == [1, 2]
    ids = [r["tracks"]["id"].tolist() for r in out[1:]]
    print("ids per frame:", ids)
    assert ids[4] == [1] and ids[N - 2] == [1, 3], "one island while the rectangles cross; the smaller one comes back under a new id"
    assert out[N - 1]["tracks"]["t"] == N - 1
    sums = first["sum_motion"][:2, 0]
    assert sums[0] * sums[1] < 0, "the rectangles move against each other"
    # the restatement on the tickets' own label maps: ids, slots, ages and hits need nothing but labels
    trk = indep.Tracker(15, T_F, REACH_F, GAP_F)
    for k in range(1, N):
        isl = out[k]["islands"]
        tcounts, rows = trk.step(isl["labels"], isl["n_listed"])
        assert _table(out[k]["tracks"])[0].tolist() == tcounts.tolist()
        np.testing.assert_array_equal(out[k]["tracks"]["table"][:, :4], rows[:, :4])


def test_push_frame_async_two_tickets_in_flight(ctx, sync_run):
    ref, want = sync_run
    ctx.reset_frames()
    with _Settings(ctx):
        pins = [ctx.pinned_frame(tc.FH, tc.FW) for _ in range(3)]
        tickets, got = [], []
        for k in range(N):
            if k >= 2:
                got.append(ctx.frame_wait(tickets[k - 2]))
            np.copyto(pins[k % 3], tc.frames()[k])
            tickets.append(ctx.push_frame_async(pins[k % 3], **tc.FUSED))
        got += [ctx.frame_wait(tickets[N - 2]), ctx.frame_wait(tickets[N - 1])]
        for p in pins:
            ctx.free_pinned(p)
    assert _no_step(got[0]["tracks"])
    _same_tracks([r["tracks"] for r in got[1:]], want, "push_frame_async")


@pytest.mark.parametrize("cuts", ((10,), (3, 7), (1,) * 10), ids=("10", "3+7", "1x10"))
def test_push_frames_async_cuts(ctx, sync_run, cuts):
    ref, want = sync_run
    ctx.reset_frames()
    got, at = [], 0
    with _Settings(ctx):
        bufs = []
        tickets = []
        for n in cuts:
            buf = ctx.pinned_array((n, tc.FH, tc.FW), np.uint8)
            np.copyto(buf, tc.frames()[at:at + n])
            at += n
            bufs.append(buf)
            if len(tickets) == 2:
                got += ctx.frames_wait(tickets.pop(0))
            tickets.append(ctx.push_frames_async(buf, **tc.FUSED))
        for t in tickets:
            got += ctx.frames_wait(t)
        for b in bufs:
            ctx.free_pinned(b)
    assert len(got) == N and not got[0]["have_vectors"] and _no_step(got[0]["tracks"])
    _same_tracks([r["tracks"] for r in got[1:]], want, f"push_frames_async {cuts}")
    for k in range(1, N):
        np.testing.assert_array_equal(got[k]["islands"]["labels"], ref[k]["islands"]["labels"])


def test_hip_flow_reduced_through_the_dense_fused_form(ctx):
    kw = dict(levels=3, radius=6, iters=3, max_w=150, max_h=150, contrast_mask=True, reduced=True, farneback=True)
    ctx.lk_reset()
    with _Settings(ctx):
        out = [ctx.lk_push_frame_fused(tc.frames()[k], estimator=False, **kw, **DET) for k in range(N)]
    ctx.lk_reset()
    assert not out[0]["have_vectors"] and _no_step(out[0]["tracks"])
    assert all(r["have_vectors"] for r in out[1:])
    print("hip_flow: rows per frame", [r["tracks"]["rows"] for r in out[1:]], "ids", [r["tracks"]["id"].tolist() for r in out[1:]])
    _same_tracks([r["tracks"] for r in out[1:]], _expect_from_records(ctx, [r["entries"] for r in out[1:]]), "hip_flow reduced, fused")
    assert out[N - 1]["tracks"]["t"] == N - 1


def test_compensation_mode_1_follows_the_compensated_islands(ctx):
    """the detector reads records the caller never sees: what is exact is the restatement on the ticket's own label maps"""
    ctx.reset_frames()
    ctx.set_detect_compensation(1)
    try:
        with _Settings(ctx):
            out = [ctx.push_frame(tc.frames()[k], estimator=True, **tc.FUSED) for k in range(N)]
    finally:
        ctx.set_detect_compensation(0)
    assert _no_step(out[0]["tracks"])
    trk = indep.Tracker(15, T_F, REACH_F, GAP_F)
    for k in range(1, N):
        isl = out[k]["islands"]
        tcounts, rows = trk.step(isl["labels"], isl["n_listed"])
        assert _table(out[k]["tracks"])[0].tolist() == tcounts.tolist(), k
        np.testing.assert_array_equal(out[k]["tracks"]["table"][:, :4], rows[:, :4])


def test_the_state_starts_fresh_after_t_0_and_after_a_reset(ctx, sync_run):
    ref, _ = sync_run
    rec = [r["entries"] for r in ref]
    # T 8 -> 0 -> 8 mid-stream
    ctx.reset_frames()
    got = []
    ctx.set_detect_islands(K_F)
    try:
        for k in range(N):
            ctx.set_detect_tracks(0 if k in (4, 5) else T_F, REACH_F, GAP_F)
            got.append(ctx.push_frame(tc.frames()[k], **tc.FUSED))
    finally:
        ctx.set_detect_islands(0)
        ctx.set_detect_tracks(0)
    assert "tracks" not in got[4] and "tracks" not in got[5] and "islands" in got[4]
    _same_tracks([r["tracks"] for r in got[1:4]], _expect_from_records(ctx, rec[1:4]), "in front of T = 0")
    _same_tracks([r["tracks"] for r in got[6:]], _expect_from_records(ctx, rec[6:]), "behind T = 0")
    assert got[6]["tracks"]["t"] == 1
    # a reset mid-stream: frame 5 is a first frame again
    ctx.reset_frames()
    with _Settings(ctx):
        a = [ctx.push_frame(tc.frames()[k], **tc.FUSED) for k in range(5)]
        ctx.reset_frames()
        b = [ctx.push_frame(tc.frames()[k], **tc.FUSED) for k in range(5, N)]
    _same_tracks([r["tracks"] for r in a[1:]], _expect_from_records(ctx, rec[1:5]), "in front of the reset")
    assert not b[0]["have_vectors"] and _no_step(b[0]["tracks"])
    _same_tracks([r["tracks"] for r in b[1:]], _expect_from_records(ctx, rec[6:]), "behind the reset")
    # reach or gap changed: fresh as well
    ctx.reset_frames()
    ctx.set_detect_islands(K_F)
    try:
        c = []
        for k in range(N):
            ctx.set_detect_tracks(T_F, REACH_F, GAP_F if k < 5 else GAP_F + 1)
            c.append(ctx.push_frame(tc.frames()[k], **tc.FUSED))
    finally:
        ctx.set_detect_islands(0)
        ctx.set_detect_tracks(0)
    assert c[4]["tracks"]["t"] == 4 and c[5]["tracks"]["t"] == 1


def test_with_t_0_the_fused_outputs_are_those_of_a_context_that_never_set_it(ctx):
    from ofps_amd.runtime import HipContext

    def run(c, touch):
        c.reset_frames()
        if touch:
            c.set_detect_tracks(T_F, REACH_F, GAP_F)
            c.set_detect_tracks(0, REACH_F, GAP_F)
        c.set_detect_islands(K_F)
        try:
            return [c.push_frame(tc.frames()[k], want_entries=True, want_field=True, **tc.FUSED) for k in range(4)]
        finally:
            c.set_detect_islands(0)

    other = HipContext(0)
    try:
        want = run(other, False)
    finally:
        other.close()
    got = run(ctx, True)
    for g, w in zip(got, want):
        assert "tracks" not in g and "tracks" not in w
        assert (g["have_vectors"], g["n_vectors"]) == (w["have_vectors"], w["n_vectors"])
        assert g["quat"].tobytes() == w["quat"].tobytes()
        if w["have_vectors"]:
            assert g["entries"].tobytes() == w["entries"].tobytes()
            assert (g["motion"] is None) == (w["motion"] is None)
            if w["motion"]:
                assert g["motion"][0] == w["motion"][0] and g["motion"][1].tobytes() == w["motion"][1].tobytes()
        for key in ("n_islands", "n_components", "dim", "n_listed"):
            assert g["islands"][key] == w["islands"][key]
        assert g["islands"]["table"].tobytes() == w["islands"]["table"].tobytes() and g["islands"]["labels"].tobytes() == w["islands"]["labels"].tobytes()


def test_frame_tracks_capacity_and_item(ctx, sync_run):
    ctx.reset_frames()
    with _Settings(ctx):
        out = [ctx.push_frame(tc.frames()[k], **tc.FUSED) for k in range(2)]
    n = out[1]["tracks"]["rows"]
    assert n >= 2
    counts = np.zeros(4, np.int32)
    rows = np.full(8 * n + GUARD, -7, np.int32)
    lib = ctx._lib
    assert lib.ofps_hip_frame_tracks(ctx._h, 0, counts.ctypes.data_as(I32P), rows.ctypes.data_as(I32P), n - 1) == EINVAL
    assert lib.ofps_hip_frame_tracks(ctx._h, 1, counts.ctypes.data_as(I32P), rows.ctypes.data_as(I32P), n) == EINVAL
    assert lib.ofps_hip_frame_tracks(ctx._h, -1, counts.ctypes.data_as(I32P), rows.ctypes.data_as(I32P), n) == EINVAL
    assert (rows == -7).all()
    assert lib.ofps_hip_frame_tracks(ctx._h, 0, counts.ctypes.data_as(I32P), rows.ctypes.data_as(I32P), n) == 0
    np.testing.assert_array_equal(rows[:8 * n].reshape(n, 8), out[1]["tracks"]["table"])
    assert (rows[8 * n:] == -7).all()
