"""hip_klt's motion prediction (include/ofps_hip.h N3p) from image to rotation, against a PLANTED camera rotation: tools/accuracy_clips.py's
ramp clip whose pan accelerates by 1 degree per frame to 3 degrees per frame (49 px at the centre of a 1080p frame, beyond what four
pyramid levels reach) and swings back, through HipKltDecoder -> HipAlmeidaEstimator with the decoder's defaults.  The bound is the one
tests/test_accuracy_gpu.py uses, the reference's own estimator test on synthetic fields: error < 10 % of the rotation
(almeida-estimator/src/lib.rs:347-348).  With "Prediction" and "Consistency check" = 16 on, least squares and RANSAC must meet it; the
same decoder without prediction is shown not to, so the clip separates the two."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu


def test_an_accelerating_pan_beyond_the_pyramids_reach_is_followed_with_prediction_and_the_check():
    import accuracy_clips
    row = accuracy_clips.run(quick=True, with_oracle=False, only=["ramp_pan_3.0"], log=lambda s: None, sad_only=True, skip=("hip_sad",), klt=True,
                             klt_fb=(16,), klt_predict=True, ramp_clips=True)["ramp_pan_3.0"]
    for combo in ("hip_klt+lsq", "hip_klt_p+lsq", "hip_klt_f16+lsq", "hip_klt_f16_p+lsq", "hip_klt_f16+ransac", "hip_klt_f16_p+ransac"):
        print(combo, "mean error %.5f degrees per frame, %.4f of the rotation" % (row[combo]["mean_err_deg"], row[combo]["rel_mean"]))
    assert abs(row["hip_klt+lsq"]["mean_rot_deg"] - 1.5) < 1e-9                  # the clip: 0, 1, 2, 3, 2, 1, 0, -1 ... degrees per frame
    assert row["hip_klt_f16_p+lsq"]["rel_mean"] < 0.10 and row["hip_klt_f16_p+ransac"]["rel_mean"] < 0.10
    # the same decoder from zero does not meet the bound with least squares
    assert row["hip_klt+lsq"]["rel_mean"] > 0.10
