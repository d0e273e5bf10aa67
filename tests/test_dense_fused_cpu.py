"""CPU side of the dense decoders' fused form: the new entry points are declared, exported and bound; the grids of the case list; and the
oracle-side properties of the fixture frames that tests/test_dense_fused_gpu.py relies on (no GPU test passes vacuously)."""
import os
import re

import pytest

import dense_fused_cases as fc
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofps_hip_lk_push_frame_fused_async", "ofps_hip_lk_frame_fused_wait", "ofps_hip_lk_push_frame_fused")


def test_new_symbols_are_declared_exported_and_bound():
    from ofps_amd import _lib
    from ofps_amd.runtime import HipContext
    header = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    for method in ("lk_push_frame_fused_async", "lk_frame_fused_wait", "lk_push_frame_fused"):
        assert callable(getattr(HipContext, method))
    assert "#define OFPS_HIP_API_VERSION 2" in header                  # additive: the version stays


def test_case_grids_and_solver_classes():
    """24 x 13 ... 150 x 84 down-sampled, 12,600 / 50,400 / 129,600 reduced pixels: below and above the cluster's lone-problem threshold
    (1,536), above 8,192 (the one-workgroup solver's limit), above 32,768 (single-workgroup compaction) and above 65,536 (dense arithmetic)"""
    for cap, grid in {**fc.DOWNSAMPLED_CAPS}.items():
        assert tuple(oracle.cv_grid(fc.W, fc.H, *cap)) == grid
    for cap, grid in fc.REDUCED_CAPS.items():
        assert tuple(oracle.cv_grid(fc.W, fc.H, *cap)) == grid
    cells = sorted(g[0] * g[1] for g in list(fc.DOWNSAMPLED_CAPS.values()) + list(fc.REDUCED_CAPS.values()))
    assert cells == [312, 1296, 2304, 5600, 12600, 12600, 50400, 129600]
    assert cells[1] < 1536 < cells[2] and cells[3] < 8192 < cells[4] and cells[5] < 32768 < cells[6] < 65536 < cells[7]


@pytest.mark.parametrize("cap,reduced", fc.CASES)
def test_the_count_is_data_dependent_at_every_cap(cap, reduced):
    """half-flat: 0 < n < n_max; noise: n == n_max; flat: n == 0 -- on the ORACLE's records"""
    half, grid = fc.records("texture", "halfflat", cap, reduced)
    n_max = grid[0] * grid[1]
    assert 0 < len(half) < n_max
    assert len(fc.records("impulse", "noise", cap, reduced)[0]) == n_max
    assert len(fc.records("noise", "flat", cap, reduced)[0]) == 0


def test_impulse_pair_count_at_the_default_cap():
    rec, grid = fc.records("halfflat", "impulse", fc.DEFAULT_CAP, False)
    assert grid == (150, 84) and 3 < len(rec) < grid[0] * grid[1] / 10, len(rec)


def test_the_few_record_frames_give_one_and_two_records():
    for n in (1, 2):
        rec, grid = fc.records(f"few{n}_prev", f"few{n}", fc.FEW_CAP, False)
        assert grid == (12, 6) and len(rec) == n


@pytest.mark.parametrize("cap,reduced", fc.CASES)
def test_the_motion_pairs_constrain_detector_and_estimators_at_every_cap(cap, reduced):
    """No GPU comparison of the motion pairs can pass with an empty field or an estimator that did nothing: per capacity the oracle's detector
    returns an island (both detector grids on the first pair), and the oracle's least-squares and RANSAC quaternions (fewer samples than
    records; more samples than the capacity) are more than 1e-3 from the identity -- 500 least-squares bounds, 10 RANSAC bounds"""
    grid = (fc.REDUCED_CAPS if reduced else fc.DOWNSAMPLED_CAPS)[cap]
    for n, (a, b) in enumerate(fc.MOTION_PAIRS):
        rec, _ = fc.records(a, b, cap, reduced)
        assert 0 < len(rec) <= grid[0] * grid[1]
        det, q = fc.expected(rec)
        assert det is not None and det[0] >= 100, (a, b)
        assert fc.off_identity(q) > 1e-3, (a, b, q)
        if n == 0:
            fine = fc.expected(rec, detector=fc.DETECTOR_FINE)[0]
            assert fine is not None and fine[1].shape == (23, 23, 2)
        for ns in fc.samples_for(grid[0] * grid[1]):
            assert fc.off_identity(fc.expected(rec, True, ns)[1]) > 1e-3, (a, b, ns)
            assert fc.refit_size(rec, ns) >= 3
    half = fc.records(*fc.MOTION_PAIRS[1], cap, reduced)[0]
    assert len(half) < len(fc.records(*fc.MOTION_PAIRS[0], cap, reduced)[0])


def test_the_refusal_stream_frames_give_counts_between_zero_and_capacity():
    """tests/test_stream_refusal_gpu.py's dense forms push texture, halfflat, move0, move1, movehalf, halfflat: the oracle's record counts of
    the five pairs, so that three of five items lie strictly between 0 and the capacity and none is empty"""
    kinds = ("texture", "halfflat", "move0", "move1", "movehalf", "halfflat")
    pairs = list(zip(kinds, kinds[1:]))
    for cap, reduced, farneback, params, capacity, want in (((24, 24), False, False, fc.LK, 312, (149, 312, 311, 169, 149)),
                                                           ((24, 24), False, True, fc.FB, 312, (149, 312, 311, 169, 149)),
                                                           ((150, 150), True, False, fc.LK, 12600, (6179, 12600, 12600, 6853, 6179))):
        got = []
        for a, b in pairs:
            rec, grid = fc.records(a, b, cap, reduced, farneback, params)
            assert grid[0] * grid[1] == capacity
            got.append(len(rec))
        assert tuple(got) == want, (cap, reduced, farneback, got)
        assert sum(0 < n < capacity for n in got) >= 3 and min(got) > 0


def test_a_large_refit_set_behind_more_than_8192_samples():
    """the device-count refit route of RANSAC (more than 8,192 samples -> cluster / stepped solver with the inlier count on the device) is
    compared on refit sets of thousands of records with an answer that is not the identity"""
    sizes = {}
    for cap in ((150, 150), (300, 300), (480, 270)):
        grid = fc.REDUCED_CAPS[cap]
        ns = fc.samples_for(grid[0] * grid[1])[1]
        rec, _ = fc.records(*fc.MOTION_PAIRS[0], cap, True)
        assert ns > 8192 and fc.off_identity(fc.expected(rec, True, ns)[1]) > 1e-3
        sizes[cap] = fc.refit_size(rec, ns)
    assert all(v > 8192 for v in sizes.values()), sizes
