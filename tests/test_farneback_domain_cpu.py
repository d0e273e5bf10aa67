"""CPU half of the hip_flow domain tests: (1) the oracle (oracle/farneback_oracle.c), whose bits tests/test_farneback_domain_gpu.py expects of the
kernels, against the INDEPENDENT float64 restatement (tests/indep_farneback.py) over the same window x polynomial grid, so that a slip of the
oracle at a parameter nobody ran before is not copied into the kernels' expected values; (2) every case of tests/farneback_cases.py has the
property it is named for.

THE ONE PART OF THE GRID WITHOUT A FLOW COMPARISON: winsize 1 with poly_n <= 6.  A 1 x 1 window solves every pixel's 2 x 2 system on its own;
where that system is near-singular rounding decides the outcome and the f32 and f64 restatements differ by tens of pixels on a third of the
pixels.  Nothing is wrong there, and nothing can be asked of the flow; those sets are covered stage-wise instead, by the expansion planes
(linear in the image, well conditioned for every poly_n), for every poly_n in 1 .. 15 and poly_sigma = 0.

Bounds.  1e-4 px is north_star's bound and the existing tests'.  Where docs/history/26_farneback_domain_tests.md records a measured maximum close
to it (winsize 3; winsize 1 with poly_n >= 7; expansion planes whose maximum is 5e-5 or more), the bound is 2 x that maximum over the case
list (two contents, two seeds each): f32-vs-f64 rounding through a near-singular solve varies by about that factor from content to content."""
import numpy as np
import pytest

import farneback_cases as FC
import indep_farneback as F
import oracle

CONTENTS = (("regions", 161), ("regions", 162), ("camera", 3), ("camera", 4))

# measured maxima over CONTENTS (docs/history/26_farneback_domain_tests.md has the table); bounds are 2 x these
MEASURED_FLOW_WINSIZE3 = 1.72e-4            # poly_n 3 on region motion; every poly_n >= 6 stays under 4e-5
MEASURED_FLOW_WINSIZE1 = 8.1e-2             # poly_n 7 at poly_sigma = 0 on region motion (poly_n 7: 3.0e-2, 9: 1.3e-3, 12: 1.8e-5, 15: 7.1e-6): the edge of the chaotic part
BOUND = 1e-4
# expansion planes: poly_n -> measured maximum where it is 5e-5 or more (bound 2 x); every other poly_n keeps 1e-4
MEASURED_PLANES = {1: 5.73e-5}


def _pair(content, seed, W=FC.GRID_W, H=FC.GRID_H):
    return FC.regions(W, H, seed=seed) if content == "regions" else FC.camera(W, H, seed=seed)


def flow_difference(content, seed, kw):
    fr = _pair(content, seed)
    f_o = oracle.farneback_flow(fr[0], fr[1], **kw)
    f_i = F.farneback(fr[0], fr[1], **kw)
    assert np.isfinite(f_o).all() and np.isfinite(f_i).all(), kw
    return float(np.abs(f_o - f_i).max())


def plane_difference(content, seed, k, n, sigma):
    fr = _pair(content, seed)
    I, R = oracle.farneback_layer(fr[0], k, n, sigma)
    h, w = I.shape
    R_i = F.poly_exp(F.layer_image(fr[0], k, w, h), n, sigma)
    assert np.isfinite(R).all() and np.isfinite(R_i).all()
    return float(np.abs(R - R_i).max())


def flow_bound(winsize):
    if winsize >= 5:
        return BOUND
    return 2 * (MEASURED_FLOW_WINSIZE3 if winsize == 3 else MEASURED_FLOW_WINSIZE1)


def plane_bound(n):
    return 2 * MEASURED_PLANES[n] if n in MEASURED_PLANES else BOUND


@pytest.mark.parametrize("winsize", FC.WINSIZES)
def test_oracle_flow_equals_the_independent_restatement_over_the_grid(winsize):
    worst = 0.0
    for kw in FC.grid_sets(winsize):
        if not FC.flow_is_compared(winsize, kw["poly_n"]):
            continue
        for content, seed in CONTENTS:
            d = flow_difference(content, seed, kw)
            worst = max(worst, d)
            assert d < flow_bound(winsize), (kw, content, seed, d)
    print(f"winsize {winsize}: max |oracle - independent| {worst:.2e} px (bound {flow_bound(winsize):.2e})")


@pytest.mark.parametrize("n", range(1, 16))
def test_oracle_expansion_planes_equal_the_independent_restatement(n):
    """every poly_n, layers 0 and 1, the grid's sigma and poly_sigma = 0 (-> 0.3 n): the stage that covers winsize 1 / poly_n <= 6"""
    worst = 0.0
    for k in (0, 1):
        for sigma in (FC.grid_sigma(n), 0.0):
            for content, seed in CONTENTS:
                d = plane_difference(content, seed, k, n, sigma)
                worst = max(worst, d)
                assert d < plane_bound(n), (n, k, sigma, content, seed, d)
    print(f"poly_n {n}: max |oracle - independent| over the five planes {worst:.2e} (bound {plane_bound(n):.2e})")


def test_poly_sigma_zero_is_the_rule_not_a_division_by_zero():
    for n in (1, 5, 15):
        g0 = F.poly_kernels(n, 0.0)
        g1 = F.poly_kernels(n, 0.3 * n)
        for a, b in zip(g0[:3], g1[:3]):
            assert np.isfinite(a).all() and np.array_equal(a, b)
        _, g, xg, xxg, ig = oracle.farneback_kernels(0, n, 0.0)
        np.testing.assert_allclose(g, g0[0][n:], atol=1e-9)
        np.testing.assert_allclose(ig, g0[3], rtol=1e-9)


@pytest.mark.parametrize("name", FC.INTEGER_RATIO_INIT)
def test_oracle_initial_flow_equals_the_independent_restatement(name):
    """the initial flow is the previous pair's; 256 x 128 at levels 2 (the coarsest layer is a quarter: block means of 4 x 4) and 128 x 64 at
    levels 0 (the flow as it is)"""
    c = FC.INIT_CASES[name]
    kw = dict(FC.DEFAULTS, levels=c["levels"], iters=c["iters"])
    fr = FC.regions(c["W"], c["H"], n=3)
    first = oracle.farneback_flow(fr[0], fr[1], **kw)
    f_o = oracle.farneback_flow(fr[1], fr[2], init=first, **kw)
    f_i = F.farneback(fr[1], fr[2], init=first, **kw)
    d = float(np.abs(f_o - f_i).max())
    print(f"{name}: max |oracle - independent| {d:.2e} px")
    assert d < BOUND
    assert not np.array_equal(f_o, oracle.farneback_flow(fr[1], fr[2], **kw))            # the initial flow is not ignored


def test_independent_initial_flow_is_defined_for_integer_ratios_only():
    fr = FC.regions(480, 270, n=2)
    with pytest.raises(NotImplementedError):
        F.farneback(fr[0], fr[1], init=np.zeros((270, 480, 2)))
    a = np.arange(8 * 4 * 2, dtype=np.float64).reshape(4, 8, 2)
    np.testing.assert_array_equal(F.initial_flow(a, 8, 4, 1.0), a)
    np.testing.assert_array_equal(F.initial_flow(a, 2, 1, 0.25)[0, 0], a[:, :4].mean(axis=(0, 1)) * 0.25)


# ---- the cases file -----------------------------------------------------------------------------------------------------------------------------
def test_grid_has_every_window_and_every_expansion_kernel():
    assert [w // 2 for w in FC.WINSIZES] == list(range(8))                         # fb_iter_kernel<0 .. 7>
    assert {1, 5, 7, 15} <= set(FC.POLY_NS)                                        # fb_polyexp_kernel<0> at both ends, <5>, <7>
    for w in FC.WINSIZES:
        sets = FC.grid_sets(w)
        assert len(sets) == 13 and all(s["winsize"] == w and s["iters"] == 2 and s["levels"] == 3 for s in sets)
        assert [s["poly_n"] for s in sets if s["poly_sigma"] == 0.0] == [5, 7, 15]
        for s in sets:
            assert s["poly_sigma"] == float(np.float32(s["poly_sigma"]))           # what the C ABI's float carries
    assert oracle.farneback_layers(FC.GRID_W, FC.GRID_H, FC.GRID_LEVELS) == [(97, 64), (48, 32)]
    assert oracle.farneback_layers(FC.CORNER_W, FC.CORNER_H, FC.CORNER_LEVELS) == [(200, 136), (100, 68), (50, 34)]
    left_out = [(w, n) for w in FC.WINSIZES for n in FC.POLY_NS if not FC.flow_is_compared(w, n)]
    assert left_out == [(1, n) for n in (1, 2, 3, 4, 5, 6)]


@pytest.mark.parametrize("name", FC.LAYER_CASES)
def test_layer_cases_select_the_variant_they_are_named_for(name):
    c = FC.LAYER_CASES[name]
    layers = oracle.farneback_layers(c["W"], c["H"], c["levels"])
    K = len(layers) - 1
    assert K == c["layers"] == F.layers(c["W"], c["H"], c["levels"])
    assert c["W"] <= FC.MAX_W
    assert FC.row_pitch(c["W"], K) == c["pitch"]
    assert tuple(FC.rows_per_lane(k) for k in range(1, K + 1)) == c["forms"]
    for k in range(K + 1):
        assert FC.blur_radius(k) == len(oracle.farneback_kernels(k)[0]) // 2 == len(F.blur_taps(k)) // 2


def test_layer_cases_cover_every_variant():
    cs = FC.LAYER_CASES
    assert sorted(c["layers"] for n, c in cs.items() if n.startswith("layers")) == [0, 1, 2, 3, 4, 5, 6]
    assert FC.blur_radius(6) == 79 and [FC.blur_radius(k) for k in range(1, 6)] == [1, 4, 9, 19, 39]
    reached = {(c["pitch"], f) for c in cs.values() for f in c["forms"]}
    assert reached == {(p, f) for p in (0, 1, 2) for f in (8, 4, 2, 1)}
    # the switch points: one byte of `need` apart
    for last, first in (("pitch0_last", "pitch1_first"), ("pitch1_last", "pitch2_first")):
        assert cs[first]["W"] == cs[last]["W"] + 1 and cs[first]["pitch"] == cs[last]["pitch"] + 1
        assert cs[last]["W"] + 2 * 4 == FC.PITCH_BYTES[cs[last]["pitch"]]
    assert cs["widest"]["W"] == FC.MAX_W
    # smaller than what the size allows
    assert oracle.farneback_layers(640, 360, 5) == oracle.farneback_layers(640, 360, 16) and len(oracle.farneback_layers(640, 360, 5)) == 4
    # the smallest frames that have their layers: one pixel less in a direction loses a layer
    for n, (dw, dh) in (("layers1", (1, 0)), ("layers4", (1, 0)), ("layers5", (1, 0)), ("layers6", (1, 0)), ("layers6", (0, 1))):
        c = cs[n]
        assert len(oracle.farneback_layers(c["W"] - dw, c["H"] - dh, c["levels"])) - 1 == c["layers"] - 1


def test_small_frames_and_the_oracle_on_them():
    assert len(FC.SMALL_FRAMES) == 15 and FC.LARGEST == dict(winsize=15, poly_n=15, poly_sigma=FC.grid_sigma(15))
    for W, H in FC.SMALL_FRAMES:
        fr = FC.regions(W, H)
        assert fr.shape == (2, H, W)
        for kw in ({}, FC.LARGEST):
            f_o = oracle.farneback_flow(fr[0], fr[1], **kw)
            assert np.isfinite(f_o).all()
        for kw in ({}, FC.LARGEST):
            d = float(np.abs(oracle.farneback_flow(fr[0], fr[1], **kw) - F.farneback(fr[0], fr[1], **kw)).max())
            assert d < BOUND, (W, H, kw, d)


def test_initial_flow_cases():
    for name, c in FC.INIT_CASES.items():
        layers = oracle.farneback_layers(c["W"], c["H"], c["levels"])
        assert len(layers) - 1 == c["layers"], name
        w, h = layers[-1]
        assert (c["W"] / w, c["H"] / h) == pytest.approx(c["ratio"]), name
    ratios = {c["ratio"] for c in FC.INIT_CASES.values()}
    assert {(1.0, 1.0), (8.0, 8.0), (64.0, 64.0)} <= ratios and any(r[1] != int(r[1]) for r in ratios)
    for name in FC.INTEGER_RATIO_INIT:
        c = FC.INIT_CASES[name]
        w, h = oracle.farneback_layers(c["W"], c["H"], c["levels"])[-1]
        assert c["W"] % w == 0 and c["H"] % h == 0
    W, H = FC.SYNTH_INIT_W, FC.SYNTH_INIT_H
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sub, forty, out = (FC.synthetic_init(k) for k in FC.SYNTH_INITS)
    for f in (sub, forty, out):
        assert f.shape == (H, W, 2) and f.dtype == np.float32 and np.isfinite(f).all()
    assert np.abs(sub).max() <= 0.5 and 39 < np.abs(forty).max() <= 40
    assert np.abs(out).min() >= 2 * max(W, H)
    x1, y1 = xx + out[..., 0], yy + out[..., 1]
    assert (((x1 < 0) | (x1 > W - 1)) & ((y1 < 0) | (y1 > H - 1))).all()            # every vector points outside, in both directions
    assert (out[..., 0] > 0).any() and (out[..., 0] < 0).any() and (out[..., 1] > 0).any() and (out[..., 1] < 0).any()
    # ... and still does on the coarsest layer (200 x 120 has one layer above it: block means of 2 x 2, halved)
    c = F.initial_flow(out, W // 2, H // 2, 0.5)
    assert (np.abs(c) >= max(W, H) // 2).mean() > 0.9
    for k in FC.SYNTH_INITS:
        fr = FC.regions(W, H, n=2)
        assert np.isfinite(oracle.farneback_flow(fr[0], fr[1], init=FC.synthetic_init(k))).all()


def test_refusals_strides_and_the_rest_of_the_lists():
    fr = FC.regions(128, 96)
    for kw in FC.REFUSED_PARAMS:
        if kw in (dict(iters=65), dict(winsize=17)):
            assert np.isfinite(oracle.farneback_flow(fr[0], fr[1], **kw)).all()
            continue                                  # limits of the kernels (64 updates, window 15), not of the algorithm: the oracle has neither
        with pytest.raises(ValueError):
            oracle.farneback_flow(fr[0], fr[1], **kw)
    g = FC.REFUSED_GEOMETRIES
    assert F.layers(g[0]["W"], g[0]["H"], g[0]["levels"]) == 7 and g[1]["W"] == FC.MAX_W + 1
    assert F.layers(4096, 4096, 6) == 6
    assert FC.ITERS == (1, 2, 5, 64) and oracle.farneback_layers(FC.ITERS_W, FC.ITERS_H, 5) == [(128, 96), (64, 48)]
    assert [W % 4 for W, _ in FC.STRIDE_SIZES] == [2, 0]
    assert all((W + p) % 4 for W, _ in FC.STRIDE_SIZES for p in (1, 3)) and all((W + 64) % 4 == W % 4 for W, _ in FC.STRIDE_SIZES)
    fr = FC.regions(33, 17)
    for fill in FC.STRIDE_FILLS:
        buf, view = FC.padded(fr[0], 33 + 3, fill, offset=2)
        assert np.array_equal(view, fr[0]) and view.strides == (36, 1) and buf.size == 2 + 17 * 36
        pad = buf[2:].reshape(17, 36)[:, 33:]
        assert (pad == 255).all() if fill == "255" else len(np.unique(pad)) > 8
    assert FC.BACK_TO_BACK[0] == FC.BACK_TO_BACK[-1] and [p for _, _, p in FC.BACK_TO_BACK] == [7, 15, 5, 7]
    assert [FC.decoder_winsize(r) for _, r in FC.DECODER_ARGS] == [1, 5, 15, 13, 13]
    assert {l for l, _ in FC.DECODER_ARGS} == {0, 5, 6} and {r for _, r in FC.DECODER_ARGS} == {0, 2, 6, 7}
