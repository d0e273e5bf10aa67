"""hip_klt's motion prediction (include/ofps_hip.h N3p): what the row promises, asserted of the restatement tests/indep_klt_pred.py alone --
the GPU test must not pass on inputs that separate nothing --, the figures the row's issue was written against, and the statements of the
new entry points, the option and the hosts' property.  No GPU."""
import os
import re

import numpy as np

import ffi_parse
import indep_klt as ik
import indep_klt_fb as ifb
import indep_klt_pred as ip
import klt_cases as kc
import klt_pred_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ofps_hip_set_klt_prediction", "ofps_hip_get_klt_prediction", "ofps_hip_klt_predict", "ofps_hip_klt_predict_dev",
               "ofps_hip_klt_track_from", "ofps_hip_klt_track_from_dev", "ofps_hip_klt_flow_from", "ofps_hip_klt_flow_from_dev"]
NEW_OPTION = "OFPS_HIP_KLT_PREDICTION"
SET0 = kc.PARAM_SETS[0]


# ------------------------------------------------------------------------------------------------ 1: declarations
def test_header_ctypes_table_rust_block_option_and_property_tables_declare_the_prediction():
    hdr = ffi_parse.header_signatures()
    rs = ffi_parse.rust_signatures()
    from ofps_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in hdr, name + " is not in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, name + " is not in ofps_amd/_lib.py"
        assert name in rs, name + " is not in INTEGRATION.md's Rust block"
        ret, args = hdr[name]
        res, cargs = _lib.PROTOTYPES[name]
        assert len(args) == len(cargs) == len(rs[name][1]), name
        for a, c, r in zip(args, cargs, rs[name][1]):
            assert ffi_parse.same_class(a, ffi_parse.ctypes_class(c), lp64=True), (name, a, c)
            assert ffi_parse.same_class(a, r), (name, a, r)
    assert len(hdr["ofps_hip_set_klt_prediction"][1]) == 2 and len(hdr["ofps_hip_get_klt_prediction"][1]) == 1
    for name in ("ofps_hip_klt_track", "ofps_hip_klt_track_dev", "ofps_hip_klt_flow", "ofps_hip_klt_flow_dev"):      # the signature plus one argument
        new = name.replace("_track", "_track_from").replace("_flow", "_flow_from")
        assert hdr[new][0] == hdr[name][0] and len(hdr[new][1]) == len(hdr[name][1]) + 1, name
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert "N3p" in text and "IGNORE the setting" in text
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)     # additive
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ctx_src = open(os.path.join(ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    assert '"' + NEW_OPTION + '"' in names, NEW_OPTION + " is not in the option list"
    assert ctx_src.count('"' + NEW_OPTION + '"') >= 2, NEW_OPTION + " is not handled by apply_option"
    assert "`" + NEW_OPTION + "=" in integration and NEW_OPTION in text
    from ofps_amd.runtime import HipContext
    for fn in ("set_klt_prediction", "get_klt_prediction", "klt_predict", "klt_predict_dev", "klt_track_from", "klt_track_from_dev", "klt_flow_from",
               "klt_flow_from_dev"):
        assert callable(getattr(HipContext, fn)), fn
    # both hosts: a boolean extension property "Prediction", behind the decoder's own table, which keeps "Consistency check" last
    from ofps_amd.plugins import HipKltDecoder
    assert [p[0] for p in HipKltDecoder._PROPS][-1] == "Consistency check"
    assert HipKltDecoder._EXT_PROPS == (("Prediction", "bool", "prediction", None, None),)
    assert callable(HipKltDecoder.ext_props) and "set_prop" in vars(HipKltDecoder)
    host = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_host.cpp")).read()
    assert re.search(r'klt_decoder_props\(const KltPropStorage& at\) \{\s*auto props = klt_props\(at\);\s*props\.emplace_back\("Prediction", '
                     r'PropertyMut::boolean\(&at\.settings->prediction\)\);', host)
    assert re.search(r"if \(klt_\) return klt_decoder_props\(", host) and "ofps_hip_set_klt_prediction" in host
    tool = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool.cpp")).read()
    assert '"--klt-predict"' in tool


# ------------------------------------------------------------------------------------------------ 2: zero guesses are N3 / N3m / N3f
def test_zero_guesses_are_the_unpredicted_restatement():
    for name in pc.SMALL_NAMES:
        prev, cur = pc.case(name)
        H, W = prev.shape
        for params in kc.PARAM_SETS:
            cell, r, ms, e, R, L, w, K = params
            pts = np.concatenate([pc.points(name, cell, r, ms), [[W, 3], [-1, 5], [7, H]]])
            for zm in (False, True):
                for F in (0, 64):
                    want = ifb.track(prev, cur, pts, L, w, K, e, R, zm, F)
                    got = ip.track_from(prev, cur, pts, np.zeros_like(pts), L, w, K, e, R, zm, F)
                    np.testing.assert_array_equal(got, want, err_msg=f"{name} {params} {zm} {F}")
                    if params is SET0 or name == "warp97":
                        wf = ifb.flow(prev, cur, L, w, K, cell, r, ms, e, R, zm, F)
                        for ps in (None, np.full((len(wf["slots"]), 6), 3, np.int32)):       # no slots, and slots none of which is kept
                            gf = ip.flow_from(prev, cur, L, w, K, ps, cell, r, ms, e, R, zm, F)
                            np.testing.assert_array_equal(gf["slots"], wf["slots"])
                            np.testing.assert_array_equal(gf["residuals"], wf["residuals"])
                            assert gf["records"].tobytes() == wf["records"].tobytes() and gf["count"] == wf["count"]


# ------------------------------------------------------------------------------------------------ 3: the predictor by hand
def _slots(nx, ny, kept):
    """kept: {(cx, cy): (dqx, dqy)}; every other slot has status 2 and a dq that must not be read"""
    s = np.zeros((ny, nx, 6), np.int32)
    s[..., 3:] = (7777, -7777, ik.ST_FLAT)
    for (cx, cy), v in kept.items():
        s[cy, cx, 3:] = (v[0], v[1], ik.ST_KEPT)
    return s.reshape(-1, 6)


def test_the_predictor_takes_the_lower_middle_of_the_kept_candidates():
    order = ((2, 2), (1, 2), (3, 2), (2, 1), (2, 3))
    vals = ((-7, 301), (12, -5), (-1023, 9), (5, 5), (-3, -777))
    want = [(0, 0), (-7, 301), (-7, -5), (-7, 9), (-7, 5), (-3, 5)]       # k = 0 .. 5: x of sorted [..][(k - 1) // 2], y likewise
    for k in range(6):
        g = ip.predict(_slots(5, 5, dict(zip(order[:k], vals[:k]))), 80, 80, 16).reshape(5, 5, 2)
        assert tuple(g[2, 2]) == want[k], k
    # the hand-made tables of the cases file agree with it
    for k, (name, W, H, cell, slots) in enumerate(pc.predictor_tables()[:6]):
        assert tuple(ip.predict(slots, W, H, cell).reshape(5, 5, 2)[2, 2]) == want[k], name


def test_the_predictor_on_the_corners_and_edges_of_a_ragged_lattice():
    nx, ny = ik.slot_grid(97, 65, 8)
    assert (nx, ny) == (13, 9)
    kept = {(cx, cy): (100 * cx + cy, -(cx + 10 * cy) * 3 - 1) for cx in range(nx) for cy in range(ny)}
    g = ip.predict(_slots(nx, ny, kept), 97, 65, 8).reshape(ny, nx, 2)
    # a corner sees itself and two neighbours: the middle of three
    assert tuple(g[0, 0]) == (sorted([0, 100, 1])[1], sorted([-1, -4, -31])[1])
    assert tuple(g[ny - 1, nx - 1]) == (sorted([1208, 1108, 1207])[1], sorted([-277, -274, -247])[1])
    # an edge sees four: the lower middle, index 1
    assert tuple(g[0, 5]) == (sorted([500, 400, 600, 501])[1], sorted([-16, -13, -19, -46])[1])
    assert tuple(g[4, nx - 1]) == (sorted([1204, 1104, 1203, 1205])[1], sorted([-157, -154, -127, -187])[1])
    # the inside sees five: the median
    assert tuple(g[4, 6]) == (604, -139)
    # nothing wraps around the lattice's rows: the last slot of a row is no neighbour of the next row's first
    lone = ip.predict(_slots(nx, ny, {(nx - 1, 3): (50, 60)}), 97, 65, 8).reshape(ny, nx, 2)
    assert tuple(lone[4, 0]) == (0, 0) and tuple(lone[3, nx - 2]) == (50, 60) and tuple(lone[2, nx - 1]) == (50, 60)
    assert int((lone != 0).any(axis=2).sum()) == 4


def test_the_predictor_ignores_every_status_but_zero_and_keeps_negative_and_odd_values():
    for st in (ik.ST_NONE, ik.ST_FLAT, ik.ST_LEFT, ik.ST_RESIDUAL, ifb.ST_NO_RETURN):
        s = _slots(3, 3, {(1, 1): (-5, 7), (0, 1): (-9, 3)}).reshape(3, 3, 6)
        s[0, 1, 3:] = (-1001, 1001, st)                     # the upper neighbour carries a dq and is not kept
        s[2, 1, 3:] = (-2001, 2001, st)
        g = ip.predict(s.reshape(-1, 6), 48, 48, 16).reshape(3, 3, 2)
        assert tuple(g[1, 1]) == (-9, 3), st                # two candidates: the lower of each component
        assert tuple(g[0, 1]) == (-5, 7), st                # a slot that is not kept is still predicted from its neighbours
    name, W, H, cell, slots = pc.predictor_tables()[7]
    assert name == "mixed" and set(slots[:, 5]) == set(range(6))
    g = ip.predict(slots, W, H, cell)
    assert (g % 2 != 0).any() and (g < 0).any()


# ------------------------------------------------------------------------------------------------ 4: the guess's arithmetic
def test_the_shift_of_a_guess_is_arithmetic():
    assert ip.start_dq(256 * 40, 256 * 30, -1, -3, 2, 96, 64) == (-1, -2)
    assert ip.start_dq(256 * 40, 256 * 30, -1, -3, 3, 96, 64) == (-1, -1)
    assert ip.start_dq(256 * 40, 256 * 30, -1025, 1023, 3, 96, 64) == (-257, 255)
    assert ip.start_dq(256 * 40, 256 * 30, -1025, 1023, 1, 96, 64) == (-1025, 1023)
    # the frame test is on P + dq * 2^(L - 1), not on P + g: -1 >> 2 = -1 stands for -4 at level 0
    assert ip.start_dq(3, 256 * 30, -1, 0, 3, 96, 64) == (0, 0) and ip.start_dq(4, 256 * 30, -1, 0, 3, 96, 64) == (-1, 0)
    assert ip.start_dq(256 * 95 - 7, 0, 7, 0, 1, 96, 64) == (7, 0) and ip.start_dq(256 * 95 - 7, 0, 8, 0, 1, 96, 64) == (0, 0)
    # beyond 2^23 in either component: (0, 0), whatever the frame
    big = 1 << 23
    assert ip.start_dq(0, 0, big, 0, 1, 40000, 40000) == (big, 0) and ip.start_dq(0, 0, big + 1, 0, 1, 40000, 40000) == (0, 0)
    assert ip.start_dq(256 * 39999, 256 * 39999, -5, -big - 1, 1, 40000, 40000) == (0, 0)


def test_an_odd_negative_guess_at_two_and_three_levels_and_at_one():
    prev, cur = pc.case("warp96")
    pts = pc.points("warp96")
    g = np.tile(np.array([[-333, 257]], np.int32), (len(pts), 1))
    for L in (1, 2, 3):
        pp, pcur = ik.pyramid(prev, L), ik.pyramid(cur, L)
        got = ip.track_from(prev, cur, pts, g, L, 4, 10)
        zero = ip.track_from(prev, cur, pts, np.zeros_like(g), L, 4, 10)
        assert (got[:, 3] == ik.ST_KEPT).sum() >= 20, L
        # an iteration that converges ends where it ends from zero; with one iteration per level the start is felt
        assert ip.track_from(prev, cur, pts, g, L, 4, 1).tobytes() != ip.track_from(prev, cur, pts, np.zeros_like(g), L, 4, 1).tobytes(), L
        np.testing.assert_array_equal(got[:, 3], zero[:, 3])
        assert np.abs(got[:, :2] - zero[:, :2]).max() <= 2, L
        # the first line by hand, and the pass behind it through the stage of N3f started one step in
        x, y = (int(v) for v in pts[0])
        assert ip.start_dq(256 * x, 256 * y, -333, 257, L, 96, 64) == (-333 >> (L - 1), 257 >> (L - 1))
        assert tuple(got[0]) == ip.track_q_from(pp, pcur, 256 * x, 256 * y, -333, 257, 4, 10)


def test_a_guess_whose_start_leaves_the_frame_is_the_zero_guess():
    for name in pc.SMALL_NAMES:
        prev, cur = pc.case(name)
        for params in (SET0, kc.PARAM_SETS[2]):
            cell, r, ms, e, R, L, w, K = params
            for zm, F in ((False, 0), (True, 64)):
                pts, gs, got = pc.track_expect(name, params, "leave", zm, F)
                H, W = prev.shape
                for (x, y), (gx, gy) in zip(pts, gs):
                    assert ip.start_dq(256 * int(x), 256 * int(y), int(gx), int(gy), L, W, H) == (0, 0)
                    assert ip.start_dq(256 * int(x) + 300, 256 * int(y) - 150, -int(gx), -int(gy), L, W, H) == (0, 0)     # ... and the way back
                    assert abs(int(gx)) <= ip.MAX_GUESS and abs(int(gy)) <= ip.MAX_GUESS
                np.testing.assert_array_equal(got, pc.track_expect(name, params, "zero", zm, F)[2], err_msg=name)


def test_the_truth_as_guess_keeps_the_clean_pair_within_the_plain_bound():
    """the plain case's bound (tests/test_klt_cpu.py, test_small_pair_every_feature_kept): all 24 features of warp96 kept at levels 2, radius 4,
    the worst within 0.15 px of the planted motion"""
    pts, gs, got = pc.track_expect("warp96", SET0, "truth")
    assert len(pts) == 24 and np.abs(gs).max() > 256
    tx, ty = pc.truth("warp96", pts[:, 0], pts[:, 1])
    err = np.hypot(got[:, 0] / 256.0 - tx, got[:, 1] / 256.0 - ty)
    print("kept", int((got[:, 3] == ik.ST_KEPT).sum()), "worst %.3f px" % err.max())
    assert (got[:, 3] == ik.ST_KEPT).all()
    assert err.max() <= 0.15


def test_a_far_guess_counts_as_zero_and_the_rest_of_the_batch_is_tracked_from_its_guess():
    pts, gs, got = pc.track_expect("warp96", SET0, "far")
    _, _, zero = pc.track_expect("warp96", SET0, "zero")
    far = (np.abs(gs.astype(np.int64)) > ip.MAX_GUESS).any(axis=1)
    assert far.any() and (~far).any()
    np.testing.assert_array_equal(got[far], zero[far])
    prev, cur = pc.case("warp96")
    np.testing.assert_array_equal(got[~far], ip.track_from(prev, cur, pts[~far], gs[~far], 2, 4, 10))


# ------------------------------------------------------------------------------------------------ 5: the ramp table, to the figure
RAMP3 = {
    (False, 0): [(59, 57, 0), (58, 40, 18), (52, 6, 46), (58, 0, 58), (55, 0, 55), (52, 0, 52)],
    (True, 0): [(59, 57, 0), (58, 58, 0), (58, 56, 2), (56, 56, 0), (57, 53, 3), (56, 52, 4)],
    (False, 64): [(58, 57, 0), (35, 34, 1), (8, 3, 5), (6, 0, 6), (6, 0, 6), (4, 0, 4)],
    (True, 64): [(58, 57, 0), (58, 58, 0), (56, 56, 0), (56, 56, 0), (53, 53, 0), (52, 52, 0)],
}


def test_the_ramp_table_of_the_issue():
    for (pred, F), want in RAMP3.items():
        got = pc.ramp_table("ramp3", pc.RAMP_SET, pred, F)
        print("ramp3 prediction", pred, "F", F, got)
        assert got == want, (pred, F)


def test_the_steeper_ramp_at_32_px_per_frame():
    last = {k: pc.ramp_table("ramp4", pc.RAMP_SET, *k)[-1] for k in ((False, 0), (True, 0), (True, 64))}
    print(last)
    assert last[(False, 0)][:2] == (49, 0)                   # 0 of 49 right without prediction
    assert last[(True, 0)][:2] == (56, 46)                   # 46 of 56 with it
    assert last[(True, 64)][:2] == (46, 46)                  # 46 of 46 with the check at a quarter pixel


def test_the_steeper_ramp_at_the_decoders_defaults():
    off = pc.ramp_table("ramp4", pc.DEFAULT_SET, False)
    on = pc.ramp_table("ramp4", pc.DEFAULT_SET, True)
    print("levels 4 radius 7, no prediction", off, "prediction", on)
    assert off[5:] == [(30, 6, 24), (34, 2, 32), (40, 0, 40)]             # the pairs of 24, 28 and 32 px
    assert on[5:] == [(49, 46, 3), (46, 44, 2), (52, 46, 6)]


def test_prediction_separates_at_twelve_pixels_and_more():
    """levels 2, radius 4 reach about 6 px: from 12 px per pair on nothing is right without prediction, and with it the tracker follows.
    Asserted on the table's sequence (3 to 18 px) alone: on the steeper one the issue's own figure, 46 of 56 at 32 px, is below nine in
    ten; its figures are pinned by the two tests above"""
    off = pc.ramp_table("ramp3", pc.RAMP_SET, False)
    on = pc.ramp_table("ramp3", pc.RAMP_SET, True)
    on64 = pc.ramp_table("ramp3", pc.RAMP_SET, True, 64)
    seen = 0
    for st, a, b, c in zip(pc.RAMPS["ramp3"], off, on, on64):
        if st < 12:
            continue
        seen += 1
        assert a[0] > 0 and a[1] == 0, (st, a)                # without prediction no kept track is within 0.25 px
        assert c[0] >= 40 and c[2] == 0, (st, c)              # with prediction and F = 64 no kept track is wrong by 1 px or more
        assert b[0] >= 40 and 10 * b[1] >= 9 * b[0], (st, b)  # with prediction at least nine in ten kept tracks are within 0.25 px
    assert seen == 3


def test_the_chain_passes_each_pairs_slots_to_the_next():
    fr = pc.ramp_frames("ramp3")
    out = pc.ramp_expect("ramp3", pc.RAMP_SET, True)
    cell, r, ms, e, R, L, w, K = pc.RAMP_SET
    assert not out[0]["guesses"].any()                       # the first pair starts from zero
    for k in (1, 4):
        np.testing.assert_array_equal(out[k]["guesses"], ip.predict(out[k - 1]["slots"], pc.RAMP_W, pc.RAMP_H, cell))
        again = ip.flow_from(fr[k], fr[k + 1], L, w, K, out[k - 1]["slots"], cell, r, ms, e, R)
        np.testing.assert_array_equal(again["slots"], out[k]["slots"])
    assert np.median(out[4]["guesses"][:, 0]) == -12 * 256   # pair 4 (15 px) starts from pair 3's 12 px
