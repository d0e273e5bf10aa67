"""No GPU: the cases of tests/klt_domain_cases.py against the restatements alone -- the conditions that keep tests/test_klt_domain_gpu.py from being
vacuous.  Every case with more than four slots keeps some and drops some; every status 0..7 occurs, 0 and 3 at every window radius and every
depth, 5 at every radius of the N3f sweep, 1 from geometry and 2 from min_eig; the `ties` frame has many equal maxima per cell; the 30th
iteration and the update clamp are reached; the values the cases took from the restatement are what they are said to be; and a table of status
counts that a changed generator cannot empty unnoticed.  Expectations are computed once per process and shared read-only."""
import os
from functools import lru_cache

import numpy as np
import pytest

import indep_klt as ik
import indep_klt_fb as ifb
import indep_klt_intra as ii
import indep_klt_pred as ip
import indep_klt_zm as iz
import klt_domain_cases as dc

BY_ID = {c.id: c for c in dc.FLOW_CASES}


def _kw(c):
    return dict(cell=c.cell, r=c.r, min_score=c.min_score, min_eig=c.min_eig, max_residual=c.R, mean_removal=c.zm, fb_limit=c.F)


@lru_cache(maxsize=None)
def _expect(c):
    prev, cur = dc.pair(c.frame)
    return ii.flow_from(prev, cur, c.L, c.w, c.K, None, c.q, c.P, **_kw(c))


def _counts(e):
    return tuple(int(v) for v in np.bincount(e["slots"][:, 5], minlength=8))


# (case -> status counts 0..7) of the restatement
PIN = {
    "n3-warp131-w1-L1": (141, 0, 0, 12, 0, 0, 0, 0), "n3-warp131-w1-L3": (105, 0, 0, 48, 0, 0, 0, 0),
    "n3-warp131-w2-L2": (136, 0, 0, 17, 0, 0, 0, 0), "n3-warp131-w3-L3": (131, 0, 0, 22, 0, 0, 0, 0),
    "n3-warp131-w5-L2": (143, 0, 0, 10, 0, 0, 0, 0), "n3-warp131-w6-L3": (144, 0, 0, 9, 0, 0, 0, 0),
    "n3-warp131-w7-L1": (146, 0, 0, 7, 0, 0, 0, 0),
    "n3-binary64-w1-L3": (41, 1, 0, 6, 0, 0, 0, 0), "n3-binary64-w2-L3": (43, 1, 0, 4, 0, 0, 0, 0), "n3-binary64-w6-L1": (47, 1, 0, 0, 0, 0, 0, 0),
    "deep-L4-64": (52, 0, 0, 12, 0, 0, 0, 0), "deep-L5-128": (198, 0, 0, 58, 0, 0, 0, 0), "deep-L6-256": (57, 0, 0, 7, 0, 0, 0, 0),
    "deep-257x259": (221, 17, 31, 20, 0, 0, 0, 0), "deep-511x263": (121, 0, 0, 23, 0, 0, 0, 0), "deep-128x131": (195, 16, 0, 61, 0, 0, 0, 0),
    "K1": (146, 0, 0, 7, 0, 0, 0, 0), "K30": (136, 0, 0, 17, 0, 0, 0, 0),
    "eig65535": (0, 1, 47, 0, 0, 0, 0, 0), "R1": (36, 1, 0, 0, 11, 0, 0, 0), "R4080": (47, 1, 0, 0, 0, 0, 0, 0),
    "eig64-warp": (138, 0, 4, 11, 0, 0, 0, 0), "eig4096-binary": (13, 1, 34, 0, 0, 0, 0, 0),
    "zm-warp131-w7-L3": (145, 0, 0, 8, 0, 0, 0, 0), "zm-binary-w7-R1": (36, 1, 0, 0, 11, 0, 0, 0), "zm-relit-w2": (137, 0, 0, 16, 0, 0, 0, 0),
    "fb16-warp131-w1-L1": (93, 0, 0, 12, 0, 48, 0, 0), "fb16-warp131-w2-L3": (118, 0, 0, 26, 0, 9, 0, 0),
    "fb16zm-warp131-w6-L3": (104, 0, 0, 9, 0, 40, 0, 0), "fb1-warp131-w5-L3": (21, 0, 0, 15, 0, 117, 0, 0),
    "fb4096-binary64-w5-L3": (44, 1, 0, 0, 0, 3, 0, 0), "fb16-L6-256": (55, 0, 0, 7, 0, 2, 0, 0),
    "intra-repaint-w7-P50": (35, 0, 0, 0, 0, 0, 13, 0), "intra-cut-w2-P0": (2, 0, 0, 11, 0, 0, 35, 0), "intra-cut-w2-P50": (0, 0, 0, 11, 0, 0, 35, 2),
}


def test_the_case_file_calls_neither_the_library_nor_a_restatement():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "klt_domain_cases.py")).read()
    for word in ("import indep", "runtime", "_lib", "HipContext"):
        assert word not in src, word


def test_the_domain_is_covered():
    ws = {L: set() for L in (1, 2, 3)}
    for c in dc.B1:
        ws[c.L].add(c.w)
    assert all(v == set(dc.WS) for v in ws.values())
    assert {c.L for c in dc.FLOW_CASES} == {1, 2, 3, 4, 5, 6}
    for sweep in (dc.C_ZM, dc.FB16_SWEEP, [c for c in dc.C_FB if c.zm]):
        assert {(c.w, c.L) for c in sweep} >= {(w, L) for w in dc.WS for L in (1, 3)}
        assert any(c.L == 6 for c in (dc.C_FB if sweep is dc.FB16_SWEEP else sweep))
    assert {(c.cell, c.r) for c in dc.FEATURE_CASES} == set(dc.CR_PAIRS)
    assert {(b.kw["cell"], b.kw["r"]) for b in dc.BATCH_SCORE} == {(8, 3), (16, 1), (32, 2)}
    assert {(b.kw["w"], b.kw["L"], b.ref_mode, b.chained) for b in dc.BATCH_TRACK} >= {(w, L, m, ch) for w, L in ((2, 1), (3, 5), (5, 1), (6, 5))
                                                                                       for m in (0, 1) for ch in (False, True)}
    for L, W, H in dc.TOO_SMALL:                              # one pixel below W >> (L - 1) == 8 in one axis, at it in the other
        assert sorted((W >> (L - 1), H >> (L - 1))) == [7, 8]
    for c in dc.DEEP[:3]:
        H, W = dc.pair(c.frame)[0].shape
        assert W >> (c.L - 1) == 8 and H >> (c.L - 1) == 8
    H, W = dc.pair(BY_ID["deep-511x263"].frame)[0].shape
    assert all((W >> l) & 1 for l in range(6)) and all((H >> l) & 1 for l in range(3))      # the width is odd at every level, the height at three


@pytest.mark.parametrize("group", ["n3", "deep", "zm", "fb16-", "fb16zm", "fb1-", "fb1zm", "fb4096-", "fb4096zm", "other"])
def test_every_case_keeps_some_slots_and_drops_some(group):
    named = ("n3", "deep", "zm", "fb")
    mine = [c for c in dc.FLOW_CASES if c.id.startswith(group) or (group == "other" and not c.id.startswith(named))]
    assert mine
    for c in mine:
        e = _expect(c)
        n = _counts(e)
        assert sum(n) == len(e["slots"]) > 4
        if c.id in dc.ALL_OR_NOTHING:
            assert n[0] in (0, len(e["slots"])), (c.id, n)           # and they are what they are said to be
        else:
            assert 0 < n[0] < len(e["slots"]), (c.id, n)
        if c.id in PIN:
            assert n == PIN[c.id], (c.id, n)


def test_the_pin_table_names_cases():
    assert set(PIN) <= set(BY_ID)


def test_every_status_occurs_and_where():
    seen = set()
    per_w, per_L = {w: set() for w in dc.WS}, {L: set() for L in range(1, 7)}
    for c in dc.B1 + dc.DEEP:
        st = {k for k, v in enumerate(_counts(_expect(c))) if v}
        per_w[c.w] |= st; per_L[c.L] |= st
    assert all({0, 3} <= s for s in per_w.values()), per_w
    assert all({0, 3} <= s for s in per_L.values()), per_L
    for w in dc.WS:                                           # N3f: the backward pass drops a track at every w
        assert any(_counts(_expect(c))[5] for c in dc.FB16_SWEEP if c.w == w and c.frame == dc.WARP131 and c.L == 1), w
    for c in dc.FLOW_CASES:
        seen |= {k for k, v in enumerate(_counts(_expect(c))) if v}
    assert seen == set(range(8))
    for cid, status in zip(dc.STATUS_WITNESSES, (1, 2, 4, 6, 7)):
        assert _counts(_expect(BY_ID[cid]))[status] > 0, cid
    assert _counts(_expect(BY_ID["eig65535"]))[2] == 47 and _counts(_expect(BY_ID["eig1"]))[2] == 0      # status 2 comes from min_eig


def test_status_1_comes_from_geometry():
    for c in dc.GEOMETRY_CASES:
        W, H = dc.pair(c.frame)[0].shape[::-1]
        nx, ny = ik.slot_grid(W, H, c.cell)
        f = ik.features(dc.pair(c.frame)[0], c.cell, c.r, 1).reshape(ny, nx, 3)
        j = int(c.id.rsplit("j", 1)[1])
        assert (W - (nx - 1) * c.cell, H - (ny - 1) * c.cell) == (j, j)
        if j < c.r + 2:
            assert (f[:, -1, 0] == -1).all() and (f[-1, :, 0] == -1).all() and (f[:-1, :-1, 0] >= 0).all(), c.id
        else:
            assert (f[:, -1, 0] >= 0).any() and (f[-1, :, 0] >= 0).any(), c.id
            assert set(f[:, -1, 0].tolist()) <= {-1, W - c.r - 2} and set(f[-1, :, 1].tolist()) <= {-1, H - c.r - 2}, c.id


def test_tiny_frames():
    kept = none = 0
    for c in dc.TINY_CASES:
        f = ik.features(dc.pair(c.frame)[0], c.cell, c.r, 1)
        assert len(f) <= 2
        kept += int((f[:, 0] >= 0).sum()); none += int((f[:, 0] < 0).sum())
        if c.frame[1:] == (8, 8):
            assert (f[0, 0] >= 0) == (c.r < 3), c.id
    assert kept > 0 and none > 0


def test_ties_frame_has_many_equal_maxima_in_every_full_cell():
    for r, top in ((1, 2560000), (2, 7680000), (3, 15360000)):
        for W, H in ((64, 48), (67, 35), (131, 67)):
            sc = ik.score_map(dc.pair(("ties", W, H))[0], r)
            assert int(sc.max()) == top
            for C in dc.CELLS:
                for cy in range(H // C):
                    for cx in range(W // C):
                        t = sc[cy * C:(cy + 1) * C, cx * C:(cx + 1) * C]
                        if cx * C >= r + 1 and cy * C >= r + 1 and (cx + 1) * C <= W - r - 1 and (cy + 1) * C <= H - r - 1:      # all of it admissible
                            assert int((t == top).sum()) >= 8, (r, W, H, C, cx, cy)
    f = ik.features(dc.pair(("ties", 64, 48))[0], 8, 1, 1)
    assert f[:4].tolist() == [[2, 2, 2560000], [8, 2, 2560000], [16, 2, 2560000], [24, 2, 2560000]]


def test_binary_frame_drives_the_score_up():
    img = dc.pair(dc.BINARY64)[0]
    assert set(np.unique(img).tolist()) == {0, 255}
    assert [int(ik.score_map(img, r).max()) for r in dc.RADII] == [6242400, 19767600, 33292800]


def test_the_30th_iteration_and_the_clamp_are_reached():
    a, b = _expect(BY_ID["K29"])["slots"], _expect(BY_ID["K30"])["slots"]
    assert int((a != b).any(1).sum()) == dc.K_PIN == 2
    assert dc.CLAMP_PIN == {"clamp-w1": (96, 60), "clamp-w2": (96, 5)}
    for cid, want in dc.CLAMP_PIN.items():
        c = BY_ID[cid]
        s = _expect(c)["slots"]
        k = s[:, 5] == 0
        assert (int(k.sum()), int(((np.abs(s[k, 3]) == 256 * c.w) | (np.abs(s[k, 4]) == 256 * c.w)).sum())) == want, cid


def test_values_taken_from_the_restatement():
    for c in dc.EIG_MIXED:
        n = _counts(_expect(c))
        assert n[0] > 0 and n[2] > 0, (c.id, n)
    c, slot, R = dc.RESIDUAL_EXACT
    n2 = (2 * c.w + 1) ** 2
    for r, status in ((0, 0), (R, 0), (R - 1, 4)):
        e = _expect(c._replace(R=r))
        assert int(e["residuals"][slot]) == 16 * R * n2 and int(e["slots"][slot, 5]) == status
    # min_score: the median cell's best score keeps that cell, one more loses it
    m = dc.MINSCORE_AT
    img = dc.pair(m.frame)[0]
    base = ik.features(img, m.cell, m.r, 1)
    ms = int(np.sort(base[:, 2])[len(base) // 2])
    at, above = ik.features(img, m.cell, m.r, ms), ik.features(img, m.cell, m.r, ms + 1)
    assert ms > 1 and (at[:, 2] == ms).any() and not (above[:, 2] == ms).any() and 0 < (above[:, 0] >= 0).sum() < (at[:, 0] >= 0).sum() < len(base)
    assert (ik.features(dc.pair(dc.BINARY64)[0], 16, 2, 2 ** 31 - 1)[:, 0] == -1).all()


def test_the_restatements_agree_where_they_overlap():
    """ii.flow_from is indep_klt_pred.flow_from under N3i's filter; with every extension off it is indep_klt.flow, with one on the extension's own file"""
    for cid in ("n3-warp131-w5-L3", "n3-binary64-w2-L2", "deep-L4-64"):
        c = BY_ID[cid]
        a, b = _expect(c), ik.flow(*dc.pair(c.frame), c.L, c.w, c.K, c.cell, c.r, c.min_score, c.min_eig, c.R)
        assert all(np.array_equal(a[k], b[k]) for k in ("slots", "residuals", "records", "features"))
    for cid in ("zm-warp131-w6-L3", "zm-binary-w7-R1"):
        c = BY_ID[cid]
        a, b = _expect(c), iz.flow(*dc.pair(c.frame), c.L, c.w, c.K, c.cell, c.r, c.min_score, c.min_eig, c.R)
        assert all(np.array_equal(a[k], b[k]) for k in ("slots", "residuals", "records"))
    for cid in ("fb16-warp131-w3-L3", "fb16zm-binary64-w1-L1"):
        c = BY_ID[cid]
        a, b = _expect(c), ifb.flow(*dc.pair(c.frame), c.L, c.w, c.K, c.cell, c.r, c.min_score, c.min_eig, c.R, c.zm, c.F)
        assert all(np.array_equal(a[k], b[k]) for k in ("slots", "residuals", "records"))


def test_guesses_and_points_reach_what_they_are_there_for():
    prev, cur = dc.pair(dc.POINT_FRAME)
    H, W = prev.shape
    g = dc.guess_list(28)
    assert set(g.ravel().tolist()) == set(dc.GUESSES)
    assert ip.start_dq(256 * 100, 256 * 100, -1, -255, 6, W, H) == (-1, -8)          # the shift is arithmetic
    assert ip.start_dq(256 * 100, 256 * 100, 1 << 23, 0, 6, W, H) == (0, 0) and ip.start_dq(256 * 100, 256 * 100, dc.GUESS_BEYOND, 0, 1, W, H) == (0, 0)
    pts = np.concatenate([dc.frame_points(W, H), dc.px_outside(W, H)])
    q = ik.track(prev, cur, pts, 6, 3, 10, 1, 64)
    assert (q[-4:] == [0, 0, 0, ik.ST_LEFT]).all() and (q[:9, 3] == 0).any()
    qq = ifb.track_points_q(prev, cur, np.concatenate([dc.q_positions(W, H), dc.q_outside(W, H)]), 1, 3, 10, 1, 64)
    assert (qq[-4:] == [0, 0, 0, ik.ST_LEFT]).all() and (qq[:-4, 3] == 0).any()


@pytest.mark.parametrize("bid", [b.id for b in dc.BATCH_CASES + dc.CHAIN_CASES])
def test_batch_items_keep_some_slots_and_drop_some(bid):
    b = next(x for x in dc.BATCH_CASES + dc.CHAIN_CASES if x.id == bid)
    k = dict(b.kw)
    out = ii.flow_batch(dc.sequence(b.seq), k["L"], k["w"], k["K"], b.ref_mode, 0, 0, b.chained, None, cell=k["cell"], r=k["r"],
                        mean_removal=k.get("zm", False), fb_limit=k.get("F", 0))
    assert len(out) == len(dc.sequence(b.seq)) - 1
    for i, e in enumerate(out):
        n = _counts(e)
        assert 0 < n[0] < len(e["slots"]), (bid, i, n)
        if b.chained and i:
            assert np.any(e["guesses"]), (bid, i)             # the chain hands something on
    if k.get("F"):
        assert any(_counts(e)[5] for e in out), bid


def test_activity_cases():
    for spec in dc.ACTIVITY_FRAMES:
        img = dc.pair(spec)[0]
        H, W = img.shape
        pts = dc.activity_points(W, H)
        assert (pts[:4] == [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]).all()
        for w in dc.WS:
            assert (ii.activity(img, pts, w) == 0).all() == (spec[0] == "flat")
