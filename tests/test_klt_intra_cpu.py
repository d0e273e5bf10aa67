"""hip_klt's intra test and scene-cut rule (include/ofps_hip.h N3i): the hand-derived literals of the activity, the verdict and the cut rule,
and the planted pairs the row's issue was written against, asserted of the restatement tests/indep_klt_intra.py alone -- the GPU test must
not pass on inputs that separate nothing --, and the statements of the new entry points, options and properties.  No GPU."""
import os
import re

import numpy as np

import ffi_parse
import indep_klt_intra as ii
import indep_klt_pred as ip
import klt_intra_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ofps_hip_set_klt_intra", "ofps_hip_get_klt_intra", "ofps_hip_set_klt_cut", "ofps_hip_get_klt_cut", "ofps_hip_klt_activity",
               "ofps_hip_klt_activity_dev", "ofps_hip_klt_intra", "ofps_hip_klt_intra_dev"]
NEW_OPTIONS = ("OFPS_HIP_KLT_INTRA", "OFPS_HIP_KLT_CUT")
L, w, K = xc.SET


# ------------------------------------------------------------------------------------------------ 1: declarations
def test_header_ctypes_table_rust_block_options_and_property_tables_declare_the_intra_test():
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
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert "N3i" in text and "6 intra and 7 cut" in text
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)     # additive
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ctx_src = open(os.path.join(ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    for opt in NEW_OPTIONS:
        assert '"' + opt + '"' in names, opt + " is not in the option list"
        assert ctx_src.count('"' + opt + '"') >= 2, opt + " is not handled by apply_option"
        assert "`" + opt + "=" in integration and opt in text
    from ofps_amd.runtime import HipContext
    for fn in ("set_klt_intra", "get_klt_intra", "set_klt_cut", "get_klt_cut", "klt_activity", "klt_activity_dev", "klt_intra", "klt_intra_dev"):
        assert callable(getattr(HipContext, fn)), fn
    # both hosts: the two properties, named and bounded as on hip_sad
    from ofps_amd.plugins import HipKltDecoder, HipSadDecoder
    for prop in (("Intra test", "usize", "intra_test", 0, 255), ("Scene cut", "usize", "scene_cut", 0, 100)):
        assert prop in HipKltDecoder._PROPS and prop in HipSadDecoder._PROPS
    host = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_host.cpp")).read()
    table = host[host.index("klt_props(const KltPropStorage& at) {"):]
    table = table[:table.index("\n}\n")]
    assert re.search(r'\{"Intra test",\s*PropertyMut::usize\(&s\.intra_test,\s*0,\s*255\)\}', table)
    assert re.search(r'\{"Scene cut",\s*PropertyMut::usize\(&s\.scene_cut,\s*0,\s*100\)\}', table)
    assert "ofps_hip_set_klt_intra" in host and "ofps_hip_set_klt_cut" in host
    tool = open(os.path.join(ROOT, "ofps_amd", "host", "ofps_hip_tool.cpp")).read()
    assert '"--klt-intra"' in tool and '"--klt-cut"' in tool


# ------------------------------------------------------------------------------------------------ 2: the activity by hand
def test_activity_literals():
    flat = np.full((9, 11), 117, np.uint8)
    for wr in (1, 4, 7):
        assert ii.activity_point(flat, 5, 4, wr) == (0, 117) and ii.activity_point(flat, 0, 0, wr) == (0, 117)
    dot = np.zeros((3, 3), np.uint8)
    dot[1, 1] = 255
    # S = 255, m = (255 + 4) // 9 = 28, A = 8 * 28 + (255 - 28) = 451
    assert ii.activity_point(dot, 1, 1, 1) == (451, 28)
    img = np.full((8, 8), 200, np.uint8)
    img[:2, :2] = [[10, 20], [30, 40]]
    # the corner's window, indices clamped: [[10, 10, 20], [10, 10, 20], [30, 30, 40]]: S = 180, m = 20, A = 4 * 10 + 2 * 10 + 20 = 80
    assert ii.activity_point(img, 0, 0, 1) == (80, 20)
    np.testing.assert_array_equal(ii.activity(img, [[0, 0], [-1, 0], [8, 3], [3, 8], [0, -1]], 1), [80, 0, 0, 0, 0])
    # the largest value: half the window 0, half 255 (w = 7: 112 against 113 pixels) stays within 225 * 255
    chk = np.zeros((15, 15), np.uint8)
    chk.reshape(-1)[:113] = 255
    A, m = ii.activity_point(chk, 7, 7, 7)
    assert m == (113 * 255 + 112) // 225 and A == 113 * (255 - m) + 112 * m and A <= 225 * 255


# ------------------------------------------------------------------------------------------------ 3: the verdict by hand
def test_verdict_literals():
    # A = 451, q = 8: q * 256 * A = 923,648 = 16 * 57,728: equality is intra
    st, cnt, cut = ii.verdict([[3, -4, 57728, 0], [3, -4, 57727, 0]], [451, 451], 8)
    assert st.tolist() == [6, 0] and cnt.tolist() == [2, 1] and not cut
    # stage-form activities of 2^31 and more: q * 256 * A passes 2^32 and 2^47; the comparison is 64-bit, nothing wraps
    big = [2 ** 31, 2 ** 32 - 1, 2 ** 31 + 5]
    st, cnt, _ = ii.verdict([[0, 0, 2 ** 31 - 1, 0]] * 3, big, 1)
    assert st.tolist() == [0, 0, 0] and cnt.tolist() == [3, 0]
    st, cnt, _ = ii.verdict([[0, 0, 2 ** 31 - 1, 0]] * 3, big, 255)
    assert st.tolist() == [0, 0, 0] and cnt.tolist() == [3, 0]
    # 16 * (2^31 - 1) = 34,359,738,352 against q * 256 * A at q = 1: A = 134,217,727 is the last intra activity
    st, _, _ = ii.verdict([[0, 0, 2 ** 31 - 1, 0]] * 2, [134217727, 134217728], 1)
    assert st.tolist() == [6, 0]
    # A = 0 with res = 0 is intra
    st, cnt, _ = ii.verdict([[0, 0, 0, 0]], [0], 255)
    assert st.tolist() == [6] and cnt.tolist() == [1, 1]
    # statuses 1, 2, 3 are never candidates (they report res = 0, which would be "intra" against A = 0); 4 and 5 count and keep their status
    quads = [[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3], [5, 5, 10 ** 6, 4], [5, 5, 10 ** 6, 5], [5, 5, 1, 4], [5, 5, 10 ** 6, 0], [1, 1, 1, 0]]
    st, cnt, _ = ii.verdict(quads, [0, 0, 0, 100, 100, 100, 100, 100], 8)
    assert st.tolist() == [1, 2, 3, 4, 5, 4, 6, 0] and cnt.tolist() == [5, 3]
    # statuses the test itself writes are no candidates either
    st, cnt, _ = ii.verdict([[0, 0, 10 ** 6, 6], [0, 0, 10 ** 6, 7]], [1, 1], 8)
    assert st.tolist() == [6, 7] and cnt.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 4: the cut rule by hand
def test_cut_rule_literals():
    def run(n_intra, n_keep, P):
        quads = [[1, 1, 10 ** 6, 0]] * n_intra + [[1, 1, 1, 0]] * n_keep
        return ii.verdict(quads, [100] * (n_intra + n_keep), 8, P)

    st, cnt, cut = run(5, 5, 50)                             # 100 * 5 = 50 * 10: equality is a cut
    assert cut and cnt.tolist() == [10, 5] and st.tolist() == [6] * 5 + [7] * 5
    st, cnt, cut = run(4, 6, 50)                             # one intra fewer is not
    assert not cut and cnt.tolist() == [10, 4] and st.tolist() == [6] * 4 + [0] * 6
    st, cnt, cut = ii.verdict([[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3]], [7, 7, 7], 8, 1)      # no candidate: a cut with P > 0
    assert cut and cnt.tolist() == [0, 0] and st.tolist() == [1, 2, 3]
    assert ii.is_cut(0, 0, 100) and not ii.is_cut(0, 0, 0)
    for args in ((5, 5), (10, 0), (0, 3)):
        assert not run(*args, 0)[2]                          # P = 0 is never a cut
    st, cnt, cut = run(10, 0, 100)
    assert cut and st.tolist() == [6] * 10
    # the candidates of status 4 and 5 count on both sides
    quads = [[1, 1, 10 ** 6, 4], [1, 1, 10 ** 6, 5], [1, 1, 1, 0], [1, 1, 1, 0]]
    st, cnt, cut = ii.verdict(quads, [100] * 4, 8, 50)
    assert cut and cnt.tolist() == [4, 2] and st.tolist() == [4, 5, 7, 7]


# ------------------------------------------------------------------------------------------------ 5: the planted pairs
def _rho(ans, prev):
    """16 res / (256 A) of every candidate slot"""
    out = {}
    for k, s in enumerate(ans["slots"]):
        if int(s[5]) in ii.CANDIDATES:
            A = ii.activity_point(prev, int(s[0]), int(s[1]), w)[0]
            out[k] = 16 * int(ans["residuals"][k]) / (256 * A)
    return out


def test_planted_pairs_separate_at_q_8():
    prev, cur = xc.clean_pair()
    raw = ip.flow_from(prev, cur, L, w, K)
    rho = _rho(raw, prev)
    print("clean rho", min(rho.values()), max(rho.values()))
    assert len(rho) == 48 and 0.78 < min(rho.values()) and max(rho.values()) < 5.36
    got = ii.apply(raw, prev, w, xc.Q)
    assert got["counts"].tolist() == [48, 0] and got["count"] == 48
    np.testing.assert_array_equal(got["slots"], raw["slots"])
    assert got["records"].tobytes() == raw["records"].tobytes()

    prev, cur = xc.repaint_pair()
    raw = ip.flow_from(prev, cur, L, w, K)
    rho = _rho(raw, prev)
    r0, r1, c0, c1 = xc.REPAINT
    ends_inside = {k: r0 <= s[1] + s[4] / 256 < r1 and c0 <= s[0] + s[3] / 256 < c1 for k, s in enumerate(raw["slots"].astype(np.float64)) if k in rho}
    out_rho = [rho[k] for k in rho if not ends_inside[k]]
    in_rho = [rho[k] for k in rho if ends_inside[k]]
    print("repaint rho outside", min(out_rho), max(out_rho), "inside", min(in_rho), max(in_rho))
    assert len(out_rho) == 36 and max(out_rho) < 5.36 and len(in_rho) == 12 and min(in_rho) > 9.34
    got = ii.apply(raw, prev, w, xc.Q)
    assert got["counts"].tolist() == [48, 12] and got["count"] == 36 and not got["cut"]
    kept = got["slots"][:, 5] == 0
    assert kept.sum() == 36 and (got["slots"][~kept & (raw["slots"][:, 5] == 0), 5] == ii.ST_INTRA).all()
    # each record equals the unfiltered record of its slot
    raw_rec = dict(zip(np.flatnonzero(raw["slots"][:, 5] == 0), raw["records"]))
    for rec, k in zip(got["records"], np.flatnonzero(kept)):
        assert rec.tobytes() == raw_rec[k].tobytes()
    np.testing.assert_array_equal(got["slots"][:, :5], raw["slots"][:, :5])

    prev, cur = xc.cut_pair()
    raw = ip.flow_from(prev, cur, L, w, K)
    rho = _rho(raw, prev)
    print("cut rho", min(rho.values()), max(rho.values()))
    hist = np.bincount(raw["slots"][:, 5], minlength=4).tolist()
    assert hist[0] == 40 and hist[3] == 8 and min(rho.values()) > 11.6
    got = ii.apply(raw, prev, w, xc.Q)
    assert got["counts"].tolist() == [40, 40] and got["count"] == 0 and (got["slots"][:, 5] != 0).all()
    for P in (1, 37, 50, 100):
        got = ii.apply(raw, prev, w, xc.Q, P)
        assert got["cut"] and got["count"] == 0 and len(got["records"]) == 0 and (got["slots"][:, 5] != 0).all()
    assert all(ii.is_cut(40, 40, P) for P in range(1, 101))
    # the cut rule on the repainted pair: 12 of 48 = 25 percent
    assert ii.apply(ip.flow_from(*xc.repaint_pair(), L, w, K), xc.repaint_pair()[0], w, xc.Q, 25)["cut"]
    got = ii.apply(ip.flow_from(*xc.repaint_pair(), L, w, K), xc.repaint_pair()[0], w, xc.Q, 26)
    assert not got["cut"] and got["count"] == 36


# ------------------------------------------------------------------------------------------------ 6: prediction across the cut
def test_guesses_after_a_cut_are_zero():
    fr = xc.cut_sequence()
    chain = ii.flow_chain(fr, L, w, K, xc.Q, 50)
    assert not chain[0]["cut"] and chain[0]["count"] == 48 and np.abs(chain[1]["guesses"]).sum() > 0      # the cut pair starts from the first pair's flow
    assert chain[1]["cut"] and chain[1]["count"] == 0 and (chain[1]["slots"][:, 5] != 0).all()
    assert not chain[2]["guesses"].any()
    # the third pair is then the answer of a freshly started stream
    fresh = ii.flow_from(fr[2], fr[3], L, w, K, None, xc.Q, 50)
    np.testing.assert_array_equal(chain[2]["slots"], fresh["slots"])
    assert chain[2]["records"].tobytes() == fresh["records"].tobytes() and fresh["count"] > 40
    # statuses rewritten AFTER the predictor has read them: the unfiltered slots of the cut pair give guesses that are not zero, so a
    # library that rewrote too late would be caught by the comparison with this chain
    late = ip.predict(ip.flow_from(fr[1], fr[2], L, w, K, chain[0]["slots"])["slots"], fr.shape[2], fr.shape[1], 16)
    assert np.abs(late).sum() > 0
    # without the cut rule the intra test alone does the same here: all 40 candidates are intra
    chain_q = ii.flow_chain(fr, L, w, K, xc.Q, 0)
    assert not chain_q[2]["guesses"].any() and not chain_q[1]["cut"]


def test_q_zero_is_the_unfiltered_answer():
    prev, cur = xc.repaint_pair()
    raw = ip.flow_from(prev, cur, L, w, K)
    got = ii.flow_from(prev, cur, L, w, K, None, 0, 50)       # P has no effect while q = 0
    np.testing.assert_array_equal(got["slots"], raw["slots"])
    assert got["records"].tobytes() == raw["records"].tobytes() and got["counts"] is None
