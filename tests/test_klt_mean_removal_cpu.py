"""hip_klt's mean removal (include/ofps_hip.h N3m): what the row promises, asserted of the NumPy restatements alone -- the GPU test must not
pass on inputs that separate nothing -- and the statements of the new entry points, the option and the hosts' property.  No GPU."""
import os
import re

import numpy as np

import ffi_parse
import indep_klt as ik
import klt_cases as kc
import klt_zm_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ofps_hip_set_klt_mean_removal", "ofps_hip_get_klt_mean_removal"]
NEW_OPTION = "OFPS_HIP_KLT_MEAN_REMOVAL"


def _errors(out):
    s = out["slots"]
    kept = s[:, 5] == ik.ST_KEPT
    tx, ty = kc.warp_truth(96, 64, zc.SMALL_SHIFT, s[kept, 0], s[kept, 1])
    return kept, np.hypot(s[kept, 3] / 256.0 - tx, s[kept, 4] / 256.0 - ty)


# ------------------------------------------------------------------------------------------------ 1: a brightness step that clips
def test_a_step_of_20_grey_levels_costs_the_plain_tracker_its_accuracy_and_mean_removal_nothing():
    kept, err = _errors(zc.expect("warp96+20", zc.SET0))
    print("mean removal: kept", kept.sum(), "worst", err.max(), "median", np.median(err))
    assert len(kept) == 24 and kept.all()
    assert err.max() <= 0.1
    pkept, perr = _errors(zc.expect("warp96+20", zc.SET0, mean_removal=False))
    print("plain: kept", pkept.sum(), "within 0.25 px", (perr <= 0.25).sum(), "median", np.median(perr))
    assert (perr <= 0.25).sum() < 20


# ------------------------------------------------------------------------------------------------ 2: the same pair under a residual limit
def test_with_a_residual_limit_the_plain_tracker_loses_every_record():
    plain, zm = zc.expect("warp96+20", zc.SET0_R64, mean_removal=False), zc.expect("warp96+20", zc.SET0_R64)
    print("plain", zc.status_counts(plain), "mean removal", zc.status_counts(zm))
    assert plain["count"] == 0 and (plain["slots"][:, 5] == ik.ST_RESIDUAL).all()
    assert zm["count"] == 3
    assert zc.expect("warp96", zc.SET0_R64)["count"] == 3      # what the unlit pair keeps under the same limit


# ------------------------------------------------------------------------------------------------ 3: an offset that clips nothing changes nothing
def test_an_offset_that_clips_no_pixel_changes_no_slot():
    prev, cur = zc.case("inv")
    assert (int(prev.min()), int(prev.max())) == (62, 181)
    base = zc.expect("inv", zc.SET0_R64)
    assert base["count"] == 24
    for o in zc.INVARIANT_OFFSETS:
        p, c = zc.case(f"inv{o:+d}")
        moved = cur.astype(np.int64) + o
        assert 0 <= moved.min() and moved.max() <= 255, o     # no clipped pixel: the premise
        np.testing.assert_array_equal(c, moved)
        np.testing.assert_array_equal(p, prev)
        got = zc.expect(f"inv{o:+d}", zc.SET0_R64)
        np.testing.assert_array_equal(got["slots"], base["slots"], err_msg=str(o))
        np.testing.assert_array_equal(got["residuals"], base["residuals"], err_msg=str(o))
        assert got["records"].tobytes() == base["records"].tobytes(), o
        assert zc.expect(f"inv{o:+d}", zc.SET0_R64, mean_removal=False)["count"] == 0, o


# ------------------------------------------------------------------------------------------------ 4: the content cases
def test_the_small_cases_reach_every_status_and_differ_from_the_plain_restatement():
    total = np.zeros(5, np.int64)
    differs = np.zeros(5, bool)
    for name in zc.SMALL_NAMES:
        for params in kc.PARAM_SETS:
            zm, plain = zc.status_counts(zc.expect(name, params)), zc.status_counts(zc.expect(name, params, mean_removal=False))
            print(name, params, "mean removal", zm, "plain", plain)
            total += zm
            differs |= zm != plain
    print("total", total)
    assert (total > 0).all()
    assert tuple(total) == (815, 385, 370, 38, 841)
    # status 1 is the features' verdict, which N3m leaves alone; every status the tracker decides differs in at least one case
    assert differs.tolist() == [True, False, True, True, True]


def test_a_ramp_is_flat_with_mean_removal():
    """3 x 3 windows on smooth content: a window whose gradient is constant has centred A = 0 -- shift and offset cannot be told apart"""
    params = (8, 1, 1, 1, 64, 1, 1, 1)
    assert params in kc.PARAM_SETS
    zm, plain = zc.status_counts(zc.expect("luma", params)), zc.status_counts(zc.expect("luma", params, mean_removal=False))
    assert zm.sum() == plain.sum() == 768
    assert zm[ik.ST_FLAT] == 280 and plain[ik.ST_FLAT] == 0


def test_the_flicker_sequence_separates_the_two_trackers():
    """the batch form's input: items that cross a brightness step answer differently with and without mean removal, and no two items alike"""
    for ref_mode in (0, 1):
        zm, plain = zc.flicker_expect(zc.SET0, ref_mode), zc.flicker_expect(zc.SET0, ref_mode, mean_removal=False)
        crossing = [True] * 5 if ref_mode == 0 else [True, False, True, False, True]
        for k in range(5):
            print(ref_mode, k, "mean removal", zc.status_counts(zm[k]), "plain", zc.status_counts(plain[k]))
            if crossing[k]:
                assert zm[k]["slots"].tobytes() != plain[k]["slots"].tobytes(), (ref_mode, k)
        keys = [e["slots"].tobytes() for e in zm]
        assert len(set(keys)) == 5, ref_mode
        assert all(e["count"] >= 40 for e in zm), [e["count"] for e in zm]


# ------------------------------------------------------------------------------------------------ 5: declarations
def test_header_ctypes_table_rust_block_option_and_property_tables_declare_mean_removal():
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
    assert len(hdr["ofps_hip_set_klt_mean_removal"][1]) == 2 and len(hdr["ofps_hip_get_klt_mean_removal"][1]) == 1
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert "N3m" in text and "9e14" in text                   # the row and its number range
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)     # additive
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ctx_src = open(os.path.join(ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    assert '"' + NEW_OPTION + '"' in names, NEW_OPTION + " is not in the option list"
    assert ctx_src.count('"' + NEW_OPTION + '"') >= 2, NEW_OPTION + " is not handled by apply_option"
    assert NEW_OPTION in integration and NEW_OPTION in text
    from ofps_amd.runtime import HipContext
    for fn in ("set_klt_mean_removal", "get_klt_mean_removal"):
        assert callable(getattr(HipContext, fn))
    # both hosts: a boolean property "Mean removal" behind "Iterations"
    from ofps_amd.plugins import HipKltDecoder
    props = [(p[0], p[1]) for p in HipKltDecoder._PROPS]
    assert ("Mean removal", "bool") in props
    assert props.index(("Mean removal", "bool")) == [p[0] for p in props].index("Iterations") + 1
    host = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_host.cpp")).read()
    table = host[host.index("klt_props(const KltPropStorage& at) {"):]
    table = table[:table.index("\n}\n")]
    assert re.search(r'\{"Iterations",[^}]*\}\s*,\s*\{"Mean removal",\s*PropertyMut::boolean\(', table)
    assert "ofps_hip_set_klt_mean_removal" in host
