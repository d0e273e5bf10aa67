"""No GPU: what holds of the restatement of hip_sad's mean removal alone (tests/indep_sad_prefilter.py, include/ofps_hip.h N1m), and that the
C ABI declares the feature.  The relit scenes are tests/sad_prefilter_cases.py's; tests/test_sad_prefilter_gpu.py runs the library on them."""
import os
import re

import numpy as np
import pytest

import indep_sad_prefilter as ip
import sad_prefilter_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integral_image_equals_the_clamped_loops():
    for (W, H, stride), r in (((1, 1, 1), 1), ((5, 3, 5), 4), ((5, 3, 5), 16), ((37, 23, 40), 1), ((37, 23, 40), 4)):
        for kind in pc.FILTER_KINDS:
            f = pc.filter_frame(kind, W, H, stride)[:, :W]
            np.testing.assert_array_equal(ip.prefilter(f, r), ip.prefilter_loops(f, r), err_msg=f"{W}x{H} r={r} {kind}")


def test_flat_frames_become_128_and_both_clamps_act():
    for r in pc.FILTER_RADII:
        for kind in ("flat0", "flat255"):
            assert (ip.prefilter(pc.filter_frame(kind, 37, 23, 40)[:, :37], r) == 128).all()
    F = ip.prefilter(pc.filter_frame("blocks3", 64, 48, 64), 4)
    assert F.min() == 0 and F.max() == 255


def test_the_multiplier_divides_exactly_for_every_sum_of_every_radius():
    """m = umulhi(S', ceil(2^32 / n)) for every S' = S + (n >> 1), S in [0, 255 n]: what csrc/sad_prefilter.hip computes"""
    for r in range(1, ip.MAX_RADIUS + 1):
        n = (2 * r + 1) ** 2
        M = ip.multiplier(r)
        assert M < 1 << 32 and M * n - (1 << 32) < n
        s = np.arange(n >> 1, 255 * n + (n >> 1) + 1, dtype=np.uint64)
        assert int(s[-1]) < 1 << 19
        np.testing.assert_array_equal((s * np.uint64(M)) >> np.uint64(32), s // np.uint64(n), err_msg=f"r={r}")


@pytest.mark.parametrize("i", range(len(pc.SCENES)))
@pytest.mark.parametrize("lighting", ["step", "ramp"])
def test_mean_removal_returns_the_planted_shift_where_the_plain_search_does_not(i, lighting):
    W, H, B, R, d = pc.SCENES[i]
    inner4 = pc.interior(W, H, B, d, 4)
    plain = int((pc.hits(pc.expect(i, lighting, 0)[1], d) & inner4).sum())
    print(f"scene {i} {lighting}: plain search {plain} of {int(inner4.sum())} interior blocks (at most {pc.PLAIN_AT_MOST[(i, lighting)]})")
    for r in pc.RADII:
        inner = pc.interior(W, H, B, d, r)
        hit = pc.hits(pc.expect(i, lighting, r)[1], d)
        print(f"  r={r}: {int((hit & inner).sum())} of {int(inner.sum())} interior blocks return d")
        assert int(inner.sum()) == pc.INTERIOR[(i, r)]
        assert not (inner & ~hit).any()
    assert plain <= pc.PLAIN_AT_MOST[(i, lighting)]


@pytest.mark.parametrize("i", range(len(pc.SCENES)))
def test_gain_lighting_is_reported(i):
    """0.85 v + 12 changes the contrast as well: a mean cannot remove that, and the restatement itself misses blocks.  Figures only."""
    W, H, B, R, d = pc.SCENES[i]
    inner4 = pc.interior(W, H, B, d, 4)
    print(f"scene {i} gain: plain {int((pc.hits(pc.expect(i, 'gain', 0)[1], d) & inner4).sum())} of {int(inner4.sum())}")
    for r in pc.RADII:
        inner = pc.interior(W, H, B, d, r)
        print(f"  r={r}: {int((pc.hits(pc.expect(i, 'gain', r)[1], d) & inner).sum())} of {int(inner.sum())}")


def test_the_unlit_scene_is_found_by_both_searches():
    for i, (W, H, B, R, d) in enumerate(pc.SCENES):
        inner = pc.interior(W, H, B, d, 4)
        for r in (0, 4):
            assert not (inner & ~pc.hits(pc.expect(i, "none", r)[1], d)).any(), (i, r)


def test_the_abi_declares_the_feature():
    from ofps_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    decl = set(re.findall(r"\b(ofps_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    for name in ("ofps_hip_set_sad_prefilter", "ofps_hip_get_sad_prefilter", "ofps_hip_sad_prefilter", "ofps_hip_sad_prefilter_dev"):
        assert name in decl, f"{name} is not declared in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, f"{name} is not in ofps_amd/_lib.py's table"
    assert "N1m" in hdr and "OFPS_HIP_SAD_PREFILTER" in hdr
