"""CPU: the island tracks' plain-Python restatement (tests/indep_island_tracks.py) on the hand-derived sequences of
tests/island_track_cases.py, its properties on seeded random sequences, q at its edges, and the three statements of the C ABI
(include/ofps_hip.h A5t)."""
import os
import re

import numpy as np
import pytest

import indep_detect_islands as isl_indep
import indep_island_tracks as indep
import island_track_cases as tc

F = np.float32
ENTRY_POINTS = ("ofps_hip_island_tracker_bytes", "ofps_hip_track_islands_dev", "ofps_hip_detect_tracks", "ofps_hip_set_detect_tracks",
                "ofps_hip_get_detect_tracks", "ofps_hip_frame_tracks")
OPTIONS = ("OFPS_HIP_DETECT_TRACKS", "OFPS_HIP_DETECT_TRACK_REACH", "OFPS_HIP_DETECT_TRACK_GAP")


# ---- the hand-derived sequences ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", tc.HAND, ids=lambda h: h.name)
def test_hand_derived_sequences(h):
    out, _ = indep.run(tc.hand_frames(h), tc.PRM8, tc.K8, h.T, h.reach, h.G)
    assert len(out) == len(h.want)
    for k, ((counts, _, _, tcounts, rows), want) in enumerate(zip(out, h.want)):
        assert counts[2] == 8 and tcounts[0] == len(want) and tcounts[3] == k + 1, (h.name, k)
        assert [tuple(int(v) for v in r[:4]) for r in rows] == want, (h.name, k)


def test_the_hand_cases_say_what_they_are_named_for():
    # D: the larger piece is rank 0; E: the union is one island; F: two islands listed, one row
    d = [isl_indep.islands(e, **tc.PRM8) for e in tc.hand_frames(tc.HAND_BY_NAME["D"])]
    assert [i.n_islands for i in d] == [1, 2, 1] and d[1].table[:, 1].tolist() == [6, 2]
    e = [isl_indep.islands(x, **tc.PRM8) for x in tc.hand_frames(tc.HAND_BY_NAME["E"])]
    assert [i.n_islands for i in e] == [2, 1, 2] and e[1].table[0, 1] == 18 and e[0].table[:, 1].tolist() == [9, 2]
    f, _ = indep.run(tc.hand_frames(tc.HAND_BY_NAME["F"]), tc.PRM8, tc.K8, 1, 0, 0)
    assert f[0][0][3] == 2 and f[0][3][0] == 1
    g = isl_indep.islands(tc.hand_frames(tc.HAND_BY_NAME["G"])[0], **tc.PRM8)
    assert g.table[:, 0].tolist() == [9, 11]
    # G's tie is a tie: one pair of each
    trk = indep.Tracker(8, 4, 1, 0)
    a = isl_indep.listed(g, tc.K8)
    trk.step(a[2], a[0][3])
    b = isl_indep.listed(isl_indep.islands(tc.hand_frames(tc.HAND_BY_NAME["G"])[1], **tc.PRM8), tc.K8)
    assert trk.overlap(b[2], 1)[0, :2].tolist() == [1, 1]


# ---- properties on seeded random sequences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach,G", tc.REACH_GAP)
@pytest.mark.parametrize("d", tc.RANDOM_SIDES_CPU)
def test_properties_on_random_sequences(d, reach, G):
    frames, prm = tc.random_sequence(d), tc.params_of(d)
    K, T = tc.RANDOM_K, tc.RANDOM_T
    trk, seen_free = None, set()
    for k, e in enumerate(frames):
        isl = isl_indep.islands(e, **prm)
        counts, table, labels, _ = isl_indep.listed(isl, K)
        if trk is None:
            trk = indep.Tracker(isl.dim, T, reach, G)
        tcounts, rows = trk.step(labels, counts[3], isl.field)
        n = int(tcounts[0])
        assert n == min(int(counts[3]), T) and tcounts[3] == k + 1
        ids = [int(r[0]) for r in rows if r[0] != 0]
        assert len(ids) == len(set(ids)), "ids within a frame are distinct"
        assert not (set(ids) & seen_free), "no id returns after its slot was freed"
        seen_free |= trk.freed_ids
        for r in rows:
            if r[0]:
                assert 1 <= r[3] <= r[2] and 0 <= r[1] < T, "hits <= age"
            else:
                assert r[1] == -1 and r[2] == 0 and r[3] == 0
        assert len(ids) == tcounts[1] <= tcounts[2] <= T
        # the motion sums against a direct int64 sum, one q at a time
        mx, my = indep.sums_of(rows)
        for r in range(n):
            cells = isl.field[labels == r]
            assert len(cells) == table[r, 1]
            assert int(mx[r]) == sum(indep.q(v) for v in cells[:, 0]) and int(my[r]) == sum(indep.q(v) for v in cells[:, 1])
            assert sum(abs(indep.q(v)) for v in cells[:, 0]) >= len(cells) * indep.q(0.0099), "every lit cell carries its planted motion"


@pytest.mark.parametrize("d,reach,G", [(d, r, g) for d in tc.RANDOM_SIDES_CPU for r, g in ((0, 0), (1, 1), (4, 3))])
def test_cut_independence_and_zero_state(d, reach, G):
    frames, prm = tc.random_sequence(d), tc.params_of(d)
    K, T = tc.RANDOM_K, tc.RANDOM_T
    whole, state = tc.reference(frames, prm, K, T, reach, G)

    def same(got, want, what):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                np.testing.assert_array_equal(a, b, err_msg=what)

    # 12 calls
    st, got = None, []
    for e in frames:
        o, st = indep.run([e], prm, K, T, reach, G, st)
        got += o
    same(got, whole, "12 calls")
    assert st == state
    # 5 + 7
    a, st = indep.run(frames[:5], prm, K, T, reach, G)
    b, st = indep.run(frames[5:], prm, K, T, reach, G, st)
    same(a + b, whole, "5 + 7")
    assert st == state
    # a state of zeros is a fresh tracker
    dim = int(whole[0][0][2])
    z, st = indep.run(frames, prm, K, T, reach, G, bytes(indep.state_size(dim, T)))
    same(z, whole, "zeros")
    assert st == state and len(state) == indep.state_size(dim, T)
    assert indep.Tracker(dim, T, reach, G).state() == bytes(indep.state_size(dim, T))


def test_freed_slots_and_cleared_cells_are_zero_bytes():
    h = tc.HAND_BY_NAME["H"]
    _, state = indep.run(tc.hand_frames(h)[:2], tc.PRM8, tc.K8, h.T, h.reach, h.G)
    # t = 2, one id handed out, nothing alive, nothing owned
    assert state[:16] == np.array([2, 1, 0, 0], np.int32).tobytes() and not any(state[16:])


def test_fused_frames_move_cross_and_part():
    """the frames of the fused GPU tests, through the oracle's search: two islands, one while the rectangles cross, two again -- the larger
    keeps id 1, the other one was gone for more than the gap and comes back as id 3"""
    import oracle
    f = tc.frames()
    assert f.shape == (tc.N_FUSED, tc.FH, tc.FW)
    det = {k: tc.FUSED[k] for k in ("min_size", "subdivide", "target_motion")}
    trk, ids = indep.Tracker(15, 8, 1, 2), []
    for k in range(1, tc.N_FUSED):
        r = oracle.sad_flow(f[k - 1], f[k], tc.BLOCK, tc.RANGE)
        isl = isl_indep.islands(np.asarray(r[0] if isinstance(r, tuple) else r, F), **det)
        counts, _, labels, _ = isl_indep.listed(isl, 16)
        ids.append(trk.step(labels, counts[3], isl.field)[1][:, 0].tolist())
    assert ids == [[1, 2]] * 4 + [[1]] * 4 + [[1, 3]]


# ---- q at its edges ---------------------------------------------------------------------------------------------------------------------------
def test_q_at_its_edges():
    q = indep.q
    u = 2.0 ** -24
    assert q(0.0) == 0 and q(-0.0) == 0 and q(u) == 1 and q(-u) == -1
    # ties at half steps go to the even integer: k + 0.5 steps are exact in f32 for small k
    assert [q((k + 0.5) * u) for k in (0, 1, 2, 3, 4)] == [0, 2, 2, 4, 4]
    assert [q(-(k + 0.5) * u) for k in (0, 1, 2, 3)] == [0, -2, -2, -4]
    # half an ulp either side of a tie (2^-24 steps: the value 2.5 u has an f32 neighbour 2^-22 * 2^-23 away)
    tie = F(2.5 * u)
    assert q(np.nextafter(tie, F(1))) == 3 and q(np.nextafter(tie, F(0))) == 2 and q(tie) == 2
    assert q(64.0) == 1 << 30 and q(-64.0) == -(1 << 30)
    assert q(np.nextafter(F(64), F(0))) == (1 << 30) - 64                # ulp of 64 - is 2^-18: 2^6 steps
    assert q(64.5) == 1 << 30 and q(-1e30) == -(1 << 30) and q(3.4e38) == 1 << 30
    assert q(float("inf")) == 1 << 30 and q(float("-inf")) == -(1 << 30) and q(float("nan")) == 0
    assert q(1e-40) == 0 and q(0.01) == int(np.rint(np.float64(F(0.01)) * 2 ** 24))
    v = np.array([0.0, -0.0, u, 2.5 * u, 3.5 * u, -2.5 * u, 64.0, -64.0, 65.0, np.inf, -np.inf, np.nan, 0.01, -0.03, 1e-40], F)
    assert indep.q_array(v).tolist() == [q(x) for x in v]


# ---- the ABI: header, ctypes table and the Rust block declare the entry points --------------------------------------------------------------------
def test_the_entry_points_are_declared_three_times():
    import ffi_parse as fp
    from ofps_amd import _lib
    hdr, rs = fp.header_signatures(), fp.rust_signatures()
    for name in ENTRY_POINTS:
        assert name in hdr, f"{name}: not in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, f"{name}: not in ofps_amd/_lib.py"
        assert name in rs, f"{name}: not in INTEGRATION.md's extern block"
        args, cargs = hdr[name][1], _lib.PROTOTYPES[name][1]
        assert len(args) == len(cargs) == len(rs[name][1]), name
        for a, c, r in zip(args, cargs, rs[name][1]):
            assert fp.same_class(a, fp.ctypes_class(c), lp64=True), (name, a, c)
            assert fp.same_class(a, r), (name, a, r)
        assert fp.same_class(hdr[name][0], fp.ctypes_class(_lib.PROTOTYPES[name][0]), lp64=True) and fp.same_class(hdr[name][0], rs[name][0]), name
    assert len(hdr["ofps_hip_track_islands_dev"][1]) == 14 and len(hdr["ofps_hip_detect_tracks"][1]) == 17
    assert len(hdr["ofps_hip_frame_tracks"][1]) == 5 and len(hdr["ofps_hip_set_detect_tracks"][1]) == 4
    text = open(os.path.join(fp.ROOT, "include", "ofps_hip.h")).read()
    assert "A5t" in text and "build-defined" in text[text.index("A5t"):text.index("A5t") + 600].lower()
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)     # additive
    integration = open(os.path.join(fp.ROOT, "INTEGRATION.md")).read()
    ctx_src = open(os.path.join(fp.ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    for opt in OPTIONS:
        assert '"' + opt + '"' in names, opt + " is not in the option list"
        assert ctx_src.count('"' + opt + '"') >= 2, opt + " is not handled by apply_option"
        assert "`" + opt + "=" in integration and opt in text
    lib = _lib.load()
    # the size is the header's layout: 16 + 16 T + the two maps, each padded to 16 bytes; 0 outside the ranges
    for d, T in ((1, 1), (8, 4), (15, 16), (160, 256)):
        assert lib.ofps_hip_island_tracker_bytes(d, T) == indep.state_size(d, T)
    assert [lib.ofps_hip_island_tracker_bytes(d, T) for d, T in ((0, 1), (161, 1), (8, 0), (8, 257))] == [0, 0, 0, 0]
    from ofps_amd.runtime import HipContext
    for fn in ("detect_tracks", "track_islands_dev", "set_detect_tracks", "get_detect_tracks", "frame_tracks", "island_tracker_bytes"):
        assert callable(getattr(HipContext, fn)), fn
