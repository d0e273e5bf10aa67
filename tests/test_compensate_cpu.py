"""CPU: the cases of tests/compensate_cases.py can tell the compensated detector from the raw one.  Everything here goes through the CPU
oracle only -- the oracle's detector on the raw records finds "everything moves", on the records compensated with the oracle's own
quaternion it finds the planted island."""
import numpy as np
import pytest

import compensate_cases as cc
import oracle


def _areas(entries, cam_args, q, detector):
    raw = oracle.detect_motion(entries, **detector)
    comp = oracle.detect_motion(cc.compensate_oracle(entries, oracle.camera(*cam_args), q), **detector)
    return raw, comp


@pytest.mark.parametrize("use_ransac", [True, False], ids=["ransac", "lsq"])
def test_planted_field_raw_is_the_whole_frame_compensated_is_the_island(use_ransac):
    e = cc.planted_field()
    assert e.shape == (880, 4)
    q = cc.oracle_quat(e, cc.CAM, use_ransac)
    raw, comp = _areas(e, cc.CAM, q, cc.DETECTOR)
    print(f"ransac={use_ransac}: quat {q}, raw area {cc.area_of(raw)}, compensated area {cc.area_of(comp)} of {cc.CELLS}")
    assert raw is not None and raw[0] >= 0.9 * cc.CELLS
    assert comp is not None and 1 <= comp[0] <= 0.25 * cc.CELLS
    # the fit is the planted rotation's inverse to a few 1e-4 (the island biases the least squares; RANSAC drops it)
    assert oracle.quat_angle_to(q, cc.quat_conj(cc.planted_quat())) < 2e-3


def test_compensating_the_planted_rotation_exactly_leaves_the_island_only():
    """with the planted rotation itself the residual outside the island is rounding noise"""
    e = cc.planted_field()
    out = cc.compensate_oracle(e, oracle.camera(*cc.CAM), cc.quat_conj(cc.planted_quat()))
    np.testing.assert_array_equal(out[:, :2].view(np.uint32), e[:, :2].view(np.uint32))
    mag = np.hypot(out[:, 2], out[:, 3])
    inside = mag > 5e-3
    assert inside.sum() == cc.ISLAND["w"] * cc.ISLAND["h"]
    assert mag[~inside].max() < 1e-6


def test_identity_delta_is_tiny_but_not_guaranteed_zero():
    """delta(pos, identity) in f32, as the oracle computes it: why "estimator not run" means the RAW records, not an identity compensation"""
    cam = oracle.camera(*cc.CAM)
    ident = oracle.quat_to_homogeneous(np.array([1, 0, 0, 0], np.float32))
    pos = np.concatenate([cc.planted_field()[:, :2], cc.random_records(2000, 3)[:, :2]])
    d = np.array([oracle.camera_delta(cam, p, ident) for p in pos])
    mag = np.hypot(d[:, 0], d[:, 1])
    nonzero = int((mag != 0).sum())
    print(f"identity delta: max |d| = {mag.max():.3g}, {nonzero} of {len(pos)} positions not exactly zero")
    assert mag.max() < 1e-6
    if nonzero:                                          # recorded as it is: unproject -> project does not round-trip bit for bit
        assert not np.all(d == 0)


@pytest.mark.parametrize("use_ransac", [False, True], ids=["lsq", "ransac"])
def test_frame_cases_raw_is_the_whole_frame_compensated_is_the_patch(use_ransac):
    f = cc.frames()
    assert f.shape == (cc.N_FRAMES, cc.FRAME_H, cc.FRAME_W)
    for k in range(1, cc.N_FRAMES):
        e = cc.frame_vectors(k)
        assert e.shape == (240, 4)
        q = cc.oracle_quat(e, cc.FRAME_CAM, use_ransac, cc.FRAME_RANSAC, seed=cc.SEED + k)
        raw, comp = _areas(e, cc.FRAME_CAM, q, cc.FRAME_DETECTOR)
        print(f"pair {k} ransac={use_ransac}: quat {q}, raw area {cc.area_of(raw)}, compensated area {cc.area_of(comp)} of {cc.FRAME_CELLS}")
        assert raw is not None and raw[0] >= 0.9 * cc.FRAME_CELLS
        assert comp is not None and 1 <= comp[0] <= 0.25 * cc.FRAME_CELLS


def test_compensate_oracle_is_the_inlier_test_residual():
    """the helper restates lib.rs:224-231: the records RANSAC counts as inliers are those whose compensated motion is small"""
    e = cc.planted_field()
    cam = oracle.camera(*cc.CAM)
    q, inl = oracle.solve_ypr_ransac(e, cam, seed=cc.SEED, want_inliers=True, **cc.RANSAC)
    out = cc.compensate_oracle(e, cam, q)
    mag = np.hypot(out[:, 2], out[:, 3])
    assert len(inl) >= 800 and mag[np.unique(inl)].max() < 1e-3          # 0.05 deg of a 22 deg field of view: far below the island's 0.01
