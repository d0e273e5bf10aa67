"""hip_klt's forward-backward check (include/ofps_hip.h N3f): what the row promises, asserted of the restatement tests/indep_klt_fb.py alone
-- the GPU test must not pass on inputs that separate nothing --, the figures the row's issue was written against, and the statements of
the new entry points, the option and the hosts' property.  No GPU."""
import os
import re

import numpy as np

import ffi_parse
import indep_klt as ik
import indep_klt_fb as ifb
import indep_klt_zm as iz
import klt_cases as kc
import klt_fb_cases as fc
import klt_zm_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ofps_hip_set_klt_fb", "ofps_hip_get_klt_fb", "ofps_hip_klt_track_q", "ofps_hip_klt_track_q_dev"]
NEW_OPTION = "OFPS_HIP_KLT_FB"
SET0, SET1, DEFAULT = kc.PARAM_SETS[0], kc.PARAM_SETS[1], kc.DEFAULT_SET


def _figures(name, params, fb_limit):
    out = fc.expect(name, params, fb_limit)
    kept, err = fc.errors(name, out)
    fig = int(kept.sum()), int((err > 1.0).sum()), float(err.max()) if len(err) else 0.0
    print(name, params, "limit", fb_limit, "kept %d, wrong by more than 1 px %d, worst %.3f px" % fig)
    assert fig[0] == out["count"]
    return fig


# ------------------------------------------------------------------------------------------------ 1: the stage
def test_track_q_at_whole_pixels_is_track_point():
    """P = 256 (x, y): the level's centre and the frame test are N3's, so the stage answers what N3 answers -- with and without mean removal"""
    prev, cur = fc.case("warp96")
    H, W = prev.shape
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W, 3), (-1, 5), (7, H)] + [(int(x), int(y)) for x, y, _ in ik.features(prev)[::3]]
    seen = set()
    for L, w, K, R, e in ((2, 4, 10, 0, 1), (4, 7, 10, 0, 1), (1, 1, 1, 64, 1), (3, 7, 30, 160, 400), (2, 4, 10, 0, 65535)):
        pp, pc = ik.pyramid(prev, L), ik.pyramid(cur, L)
        for x, y in pts:
            want = ik.track_point(pp, pc, x, y, w, K, e, R)
            assert ifb.track_q(pp, pc, 256 * x, 256 * y, w, K, e, R) == want, (L, w, K, R, e, x, y)
            assert ifb.track_q(pp, pc, 256 * x, 256 * y, w, K, e, R, mean_removal=True) == iz.track_point(pp, pc, x, y, w, K, e, R), (L, w, K, R, e, x, y)
            seen.add(want[3])
    assert seen >= {ik.ST_KEPT, ik.ST_FLAT, ik.ST_LEFT, ik.ST_RESIDUAL}, seen


def test_the_limit_off_is_the_plain_restatement():
    for name in fc.SMALL_NAMES:
        for params in kc.PARAM_SETS:
            got, want = fc.expect(name, params, 0), zc.expect(name, params, mean_removal=False)
            np.testing.assert_array_equal(got["slots"], want["slots"], err_msg=name)
            np.testing.assert_array_equal(got["residuals"], want["residuals"], err_msg=name)
            assert got["records"].tobytes() == want["records"].tobytes()
            gz, wz = fc.expect(name, params, 0, mean_removal=True), zc.expect(name, params)
            np.testing.assert_array_equal(gz["slots"], wz["slots"], err_msg=name)
            np.testing.assert_array_equal(gz["residuals"], wz["residuals"], err_msg=name)


# ------------------------------------------------------------------------------------------------ 2: the issue's table, to the figure
def test_a_clean_pair_keeps_its_tracks():
    assert _figures("warp96", SET0, 0)[:2] == (24, 0) and round(_figures("warp96", SET0, 0)[2], 3) == 0.056
    k, wrong, worst = _figures("warp96", SET0, 64)
    assert (k, wrong, round(worst, 3)) == (24, 0, 0.056)
    assert _figures("warp96", SET0, 16)[0] == 23


def test_a_repainted_rectangle_loses_every_track_inside_it():
    k, wrong, worst = _figures("repaint", SET0, 0)
    assert (k, wrong, round(worst, 1)) == (48, 12, 15.6)
    k, wrong, worst = _figures("repaint", SET0, 64)
    assert (k, wrong, round(worst, 3)) == (35, 0, 0.316)
    s = fc.expect("repaint", SET0, 64)["slots"]
    inside, has, kept = fc.in_repaint(s), s[:, 5] != ik.ST_NONE, s[:, 5] == ik.ST_KEPT
    assert (int((inside & has).sum()), int((~inside & has).sum())) == (11, 37)
    assert (int((inside & kept).sum()), int((~inside & kept).sum())) == (0, 35)
    assert set(s[inside & has, 5]) == {ifb.ST_NO_RETURN}


def test_motion_beyond_the_pyramids_reach_does_not_return():
    k, wrong, _ = _figures("edge", SET0, 0)
    assert (k, wrong) == (45, 45)
    assert _figures("edge", SET0, 16)[0] == 0
    assert _figures("edge", SET0, 64)[0] == 3
    k, wrong, worst = _figures("edge", DEFAULT, 0)
    assert (k, wrong, round(worst, 1)) == (35, 2, 29.9)
    k, wrong, worst = _figures("edge", DEFAULT, 64)
    assert (k, wrong, worst) == (25, 0, 0.0)


def test_the_decoders_defaults_on_the_320_pair():
    k, wrong, worst = _figures("warp320", DEFAULT, 0)
    assert (k, wrong, round(worst, 1)) == (225, 1, 6.9)
    k, wrong, worst = _figures("warp320", DEFAULT, 64)
    assert (k, wrong, round(worst, 3)) == (221, 0, 0.254)
    k, wrong, worst = _figures("warp320", DEFAULT, 16)
    assert (k, wrong, round(worst, 3)) == (210, 0, 0.071)


def test_motion_boundaries_and_unrelated_frames():
    assert _figures("luma", SET0, 0)[:2] == (182, 29)
    assert _figures("luma", SET0, 64)[:2] == (152, 11)
    assert _figures("luma", SET0, 16)[:2] == (144, 7)
    assert [fc.expect("random", SET0, F)["count"] for F in (0, 64, 16)] == [21, 2, 0]


# ------------------------------------------------------------------------------------------------ 3: every reason for "did not return"
def _back_statuses(name, params):
    b = fc.both(name, params)
    ran = b["back"][:, 3] >= 0
    assert (ran == (b["fwd"][:, 3] == ik.ST_KEPT)).all()
    return np.bincount(b["back"][ran, 3], minlength=5), b["back"][ran]


def test_every_reason_for_not_returning_is_reached():
    counts, _ = _back_statuses("luma", SET1)
    print("luma, set 1: backward statuses", counts)
    assert counts[ik.ST_FLAT] == 84 and counts[ik.ST_RESIDUAL] == 25
    counts, _ = _back_statuses("warp320", DEFAULT)
    print("warp320, defaults: backward statuses", counts)
    assert counts[ik.ST_LEFT] == 1
    # the distance alone: a backward pass that is kept and ends too far from the feature
    counts, back = _back_statuses("repaint", SET0)
    assert counts[ik.ST_KEPT] == counts.sum() == 48
    assert (back[:, 4] >= 64).sum() == 13 and (back[:, 4] < 64).sum() == 35
    # and status 5 shows the forward pass's displacement and residual
    off, on = fc.expect("repaint", SET0, 0), fc.expect("repaint", SET0, 64)
    lost = on["slots"][:, 5] == ifb.ST_NO_RETURN
    assert lost.sum() == 13 and (off["slots"][lost, 5] == ik.ST_KEPT).all()
    np.testing.assert_array_equal(on["slots"][lost, :5], off["slots"][lost, :5])
    np.testing.assert_array_equal(on["residuals"], off["residuals"])
    assert np.abs(on["slots"][lost, 3:5]).max() > 256


def test_kept_records_are_the_records_of_the_same_slots_without_the_check():
    for name, params in (("repaint", SET0), ("luma", SET0), ("luma", SET1), ("edge", DEFAULT)):
        off = fc.expect(name, params, 0)
        for F in fc.LIMITS:
            on = fc.expect(name, params, F)
            kept = on["slots"][:, 5] == ik.ST_KEPT
            np.testing.assert_array_equal(on["slots"][kept], off["slots"][kept])
            kept_off = np.flatnonzero(off["slots"][:, 5] == ik.ST_KEPT)
            pick = np.isin(kept_off, np.flatnonzero(kept))
            assert on["records"].tobytes() == off["records"][pick].tobytes(), (name, F)
            other = ~kept & (off["slots"][:, 5] != ik.ST_KEPT)
            np.testing.assert_array_equal(on["slots"][other], off["slots"][other])      # statuses 1 to 4 are the forward pass's


def test_the_limits_nest_and_one_is_an_exact_round_trip():
    for name, params in (("warp96", SET0), ("luma", SET0), ("repaint", SET0)):
        kept = [set(np.flatnonzero(fc.expect(name, params, F)["slots"][:, 5] == ik.ST_KEPT)) for F in fc.LIMITS]
        assert kept[0] <= kept[1] <= kept[2] <= kept[3], name
        b = fc.both(name, params)
        exact = np.flatnonzero((b["back"][:, 3] == ik.ST_KEPT) & (b["back"][:, 4] == 0))
        assert kept[0] == set(exact), name
    assert len(set(np.flatnonzero(fc.expect("luma", SET0, 1)["slots"][:, 5] == ik.ST_KEPT))) > 0


def test_the_widest_limit_keeps_the_clean_pair_whole():
    off, on = fc.expect("warp96", SET0, 0), fc.expect("warp96", SET0, 4096)
    np.testing.assert_array_equal(on["slots"], off["slots"])
    assert on["records"].tobytes() == off["records"].tobytes() and on["count"] == 24


# ------------------------------------------------------------------------------------------------ 4: with mean removal
def test_with_mean_removal_an_offset_that_clips_no_pixel_changes_no_slot_with_the_check_on():
    for F in (16, 64):
        base = fc.expect("inv", zc.SET0_R64, F, mean_removal=True)
        assert base["count"] >= 20
        for o in zc.INVARIANT_OFFSETS:
            got = fc.expect(f"inv{o:+d}", zc.SET0_R64, F, mean_removal=True)
            np.testing.assert_array_equal(got["slots"], base["slots"], err_msg=str(o))
            np.testing.assert_array_equal(got["residuals"], base["residuals"], err_msg=str(o))
            assert got["records"].tobytes() == base["records"].tobytes(), o
            bo, bb = fc.both(f"inv{o:+d}", zc.SET0_R64, True), fc.both("inv", zc.SET0_R64, True)
            np.testing.assert_array_equal(bo["back"], bb["back"], err_msg=str(o))
            # ... where the plain tracker with the same check keeps nothing
            assert fc.expect(f"inv{o:+d}", zc.SET0_R64, F)["count"] == 0, o


def test_the_relit_pairs_separate_the_check_with_and_without_mean_removal():
    for o in zc.RELIT_OFFSETS:
        zm, plain = fc.expect(f"warp96{o:+d}", SET0, 64, mean_removal=True), fc.expect(f"warp96{o:+d}", SET0, 64)
        print(o, "mean removal", np.bincount(zm["slots"][:, 5], minlength=6), "plain", np.bincount(plain["slots"][:, 5], minlength=6))
        assert zm["count"] >= 20
        assert zm["slots"].tobytes() != plain["slots"].tobytes()


# ------------------------------------------------------------------------------------------------ 5: declarations
def test_header_ctypes_table_rust_block_option_and_property_tables_declare_the_check():
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
    assert len(hdr["ofps_hip_set_klt_fb"][1]) == 2 and len(hdr["ofps_hip_get_klt_fb"][1]) == 1
    for name in ("ofps_hip_klt_track_q", "ofps_hip_klt_track_q_dev"):                 # the signature of the form without _q
        assert hdr[name] == hdr[name.replace("_q", "")], name
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert "N3f" in text and "did not return" in text
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)     # additive
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ctx_src = open(os.path.join(ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    assert '"' + NEW_OPTION + '"' in names, NEW_OPTION + " is not in the option list"
    assert ctx_src.count('"' + NEW_OPTION + '"') >= 2, NEW_OPTION + " is not handled by apply_option"
    assert "`" + NEW_OPTION + "=" in integration and NEW_OPTION in text
    from ofps_amd.runtime import HipContext
    for fn in ("set_klt_fb", "get_klt_fb", "klt_track_q", "klt_track_q_dev"):
        assert callable(getattr(HipContext, fn))
    # both hosts: a usize property "Consistency check" (0, 0 .. 4096) behind "Mean removal"
    from ofps_amd.plugins import HipKltDecoder
    props = [p[0] for p in HipKltDecoder._PROPS]
    assert props.index("Consistency check") == props.index("Mean removal") + 1 == len(props) - 1
    assert HipKltDecoder._PROPS[-1] == ("Consistency check", "usize", "fb_limit", 0, 4096)
    host = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_host.cpp")).read()
    table = host[host.index("klt_props(const KltPropStorage& at) {"):]
    table = table[:table.index("\n}\n")]
    assert re.search(r'\{"Mean removal",[^}]*\}\s*,\s*\{"Consistency check",\s*PropertyMut::usize\(&s\.fb_limit,\s*0,\s*kKltMaxFb\)\}\};', table)
    assert "ofps_hip_set_klt_fb" in host
    assert re.search(r"kKltMaxFb\s*=\s*4096", open(os.path.join(ROOT, "ofps_amd", "host", "ofps_host.hpp")).read())
