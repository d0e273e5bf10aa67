"""hip_klt's chained batch (include/ofps_hip.h N3pb): what the row promises, asserted of the restatement tests/indep_klt_batch_pred.py alone --
the GPU test must not pass on inputs that separate nothing --, the figures the row's issue was written against, and the statements of the
new entry points, the switch and the tools' flags.  No GPU."""
import os
import re

import numpy as np

import ffi_parse
import indep_klt as ik
import indep_klt_batch_pred as ib
import indep_klt_pred as ip
import klt_batch_pred_cases as bc
import klt_pred_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ofps_hip_set_klt_batch_prediction", "ofps_hip_get_klt_batch_prediction", "ofps_hip_klt_flow_batch_from",
               "ofps_hip_klt_flow_batch_from_dev"]
NEW_OPTION = "OFPS_HIP_KLT_BATCH_PREDICTION"


# ------------------------------------------------------------------------------------------------ 1: declarations
def test_header_ctypes_table_rust_block_option_table_and_tools_declare_the_chained_batch():
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
    assert len(hdr["ofps_hip_set_klt_batch_prediction"][1]) == 2 and len(hdr["ofps_hip_get_klt_batch_prediction"][1]) == 1
    for name in ("ofps_hip_klt_flow_batch", "ofps_hip_klt_flow_batch_dev"):       # the signature plus one trailing argument
        new = name.replace("_flow_batch", "_flow_batch_from")
        assert hdr[new][0] == hdr[name][0] and len(hdr[new][1]) == len(hdr[name][1]) + 1, name
        assert list(hdr[new][1][:-1]) == list(hdr[name][1]), name
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert "N3pb" in text and "IGNORE the setting" in text and NEW_OPTION in text
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)     # additive
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ctx_src = open(os.path.join(ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    assert '"' + NEW_OPTION + '"' in names, NEW_OPTION + " is not in the option list"
    assert ctx_src.count('"' + NEW_OPTION + '"') >= 2, NEW_OPTION + " is not handled by apply_option"
    assert "`" + NEW_OPTION + "=" in integration
    from ofps_amd.runtime import HipContext
    for fn in ("set_klt_batch_prediction", "get_klt_batch_prediction", "klt_flow_batch_from", "klt_flow_batch_from_dev"):
        assert callable(getattr(HipContext, fn)), fn
    tool = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool.cpp")).read()
    assert '"--klt-batch-predict"' in tool and "ofps_hip_set_klt_batch_prediction" in tool
    assert "--batch-predict" in open(os.path.join(ROOT, "tools", "klt_time.py")).read()
    kernels = open(os.path.join(ROOT, "ofps_amd", "csrc", "klt.hip")).read()
    for k in ("klt_track_batch_pred_kernel", "klt_track_batch_pred_zm_kernel", "klt_track_batch_pred_fb_kernel", "klt_track_batch_pred_zm_fb_kernel"):
        assert re.search(r"__global__[^\n]*\b" + k + r"\(", kernels), k


# ------------------------------------------------------------------------------------------------ 2: the chain mode is N3p's chain
def test_ref_mode_0_equals_flow_chain():
    for name, params, F, zm in (("ramp3", bc.RAMP_SET, 0, False), ("ramp3", bc.RAMP_SET, 64, True), ("ramp4", bc.DEFAULT_SET, 0, False)):
        got = bc.expect(name, params, True, F, zm)
        want = pc.ramp_expect(name, params, True, F, zm)
        assert len(got) == len(want) == len(pc.RAMPS[name])
        for k, (g, w) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(g["slots"], w["slots"], err_msg=f"{name} item {k}")
            np.testing.assert_array_equal(g["residuals"], w["residuals"])
            assert g["records"].tobytes() == w["records"].tobytes() and g["count"] == w["count"]
        plain = bc.expect(name, params, False, F, zm)
        for g, w in zip(plain, pc.ramp_expect(name, params, False, F, zm)):
            np.testing.assert_array_equal(g["slots"], w["slots"])
        assert any(g["slots"].tobytes() != p["slots"].tobytes() for g, p in zip(got[1:], plain[1:])), name


def test_an_initial_prev_slots_continues_the_chain_in_both_ref_modes():
    cell, r, ms, e, R, L, w, K = bc.RAMP_SET
    kw = dict(cell=cell, r=r, min_score=ms, min_eig=e, max_residual=R)
    for name in ("ramp3", "const4"):
        whole = bc.expect(name, bc.RAMP_SET)
        for first in (1, 3):
            rest = ib.flow_batch_from(bc.tail_frames(name, first), L, w, K, bc.SEQUENCES[name], whole[first - 1]["slots"], **kw)
            assert len(rest) == len(whole) - first
            for k, (g, want) in enumerate(zip(rest, whole[first:])):
                np.testing.assert_array_equal(g["slots"], want["slots"], err_msg=f"{name} from {first}: item {k}")
                np.testing.assert_array_equal(g["guesses"], want["guesses"])
            # the slots matter: the same frames from zero answer differently in the first item
            zero = ib.flow_batch_from(bc.tail_frames(name, first), L, w, K, bc.SEQUENCES[name], None, **kw)
            assert zero[0]["slots"].tobytes() != rest[0]["slots"].tobytes(), (name, first)
            assert not zero[0]["guesses"].any() and rest[0]["guesses"].any()


def test_the_key_mode_shares_the_features_and_passes_each_items_slots_on():
    fr = bc.frames("const4")
    out = bc.expect("const4", bc.RAMP_SET)
    cell, r, ms, e, R, L, w, K = bc.RAMP_SET
    assert len(fr) == 9 and len(out) == 8 and fr[0].shape == (bc.H, bc.W)
    canvas = np.concatenate([fr[0], fr[8][:, -32:]], axis=1)
    for k in range(9):
        np.testing.assert_array_equal(fr[k], canvas[:, 4 * k:4 * k + bc.W])           # "const4": column offsets 0, 4, ... 32
    assert not out[0]["guesses"].any()
    for k in range(1, 8):
        np.testing.assert_array_equal(out[k]["features"], out[0]["features"])           # one lattice for every item
        np.testing.assert_array_equal(out[k]["guesses"], ip.predict(out[k - 1]["slots"], bc.W, bc.H, cell))
    again = ip.flow_from(fr[0], fr[5], L, w, K, out[3]["slots"], cell, r, ms, e, R)
    np.testing.assert_array_equal(again["slots"], out[4]["slots"])
    assert np.median(out[5]["guesses"][:, 0]) == -20 * 256     # item 5 (24 px) starts from item 4's 20 px
    assert ib.pairs_of(fr, 1)[3][0] is fr[0] and ib.pairs_of(fr, 0)[3][0] is fr[3]


# ------------------------------------------------------------------------------------------------ 3: the issue's tables, to the figure
CONST4 = {
    (False, 0): [(58, 58, 0), (55, 11, 43), (53, 1, 52), (53, 0, 53), (58, 0, 58), (59, 0, 59), (56, 0, 56), (57, 0, 57)],
    (True, 0): [(58, 58, 0), (58, 56, 1), (57, 55, 2), (55, 52, 3), (55, 50, 5), (57, 50, 7), (58, 49, 9), (56, 45, 10)],
    (False, 64): [(58, 58, 0), (11, 7, 4), (6, 1, 5), (4, 0, 4), (4, 0, 4), (10, 0, 10), (4, 0, 4), (3, 0, 3)],
    (True, 64): [(58, 58, 0), (56, 56, 0), (55, 55, 0), (52, 52, 0), (50, 50, 0), (51, 50, 1), (49, 49, 0), (46, 45, 0)],
}


def test_the_const4_table_of_the_issue():
    assert bc.displacements("const4") == (4, 8, 12, 16, 20, 24, 28, 32)
    for (chained, F), want in CONST4.items():
        got = bc.table("const4", bc.RAMP_SET, chained, F)
        print("const4 chained", chained, "F", F, got)
        assert got == want, (chained, F)


def test_the_const4_kept_counts_at_the_decoders_defaults():
    off, on = bc.kept("const4", bc.DEFAULT_SET, False, 64), bc.kept("const4", bc.DEFAULT_SET, True, 64)
    print("levels 4 radius 7 F 64: no prediction", off, "chained", on)
    assert off == [56, 55, 52, 29, 2, 1, 1, 1]
    assert on == [56, 56, 52, 51, 46, 49, 44, 43]
    assert all(t[2] == 0 for t in bc.table("const4", bc.DEFAULT_SET, True, 64))       # no wrong track


def test_chaining_separates_at_twelve_pixels_and_more():
    """levels 2, radius 4 reach about 6 px.  In the key-frame form the displacement of item k is 4 (k + 1) px: from 12 px on nothing is right
    without prediction, and chained with the check at a quarter pixel the tracker follows to 32 px."""
    off = bc.table("const4", bc.RAMP_SET, False)
    on64 = bc.table("const4", bc.RAMP_SET, True, 64)
    seen = 0
    for d, a, c in zip(bc.displacements("const4"), off, on64):
        if d < 12:
            continue
        seen += 1
        assert a[1] <= 1, (d, a)                               # without prediction at most 1 kept track within 0.25 px
        assert c[1] >= 45 and c[2] <= 1, (d, c)                # chained, F = 64: at least 45 within 0.25 px, at most 1 wrong by >= 1 px
    assert seen == 6


def test_statuses_of_the_cases_cover_what_the_gpu_test_compares():
    """the sequences the GPU test runs bit for bit hold kept, lost and, with the check, not-returned slots, and chained differs from unchained"""
    for name in bc.SEQUENCES:
        on, off = bc.expect(name, bc.RAMP_SET, True, 64), bc.expect(name, bc.RAMP_SET, False, 64)
        st = set(int(s) for o in on for s in o["slots"][:, 5])
        assert {ik.ST_KEPT, ik.ST_LEFT, 5} <= st, (name, st)  # (every cell of these frames has a feature: no status 1)
        assert any(a["slots"].tobytes() != b["slots"].tobytes() for a, b in zip(on, off)), name
