"""-m gpu: what quarter-pel vectors buy in the reference's unit (rotation error per frame against planted camera rotations;
tests/test_accuracy_gpu.py is the integer-vector version).  The quick clips slow_pan_0.01, pan_tilt_0.05, pan_0.2, roll_0.3
(tools/accuracy_clips.py: 24 frames, 1920x1080, 16x16 blocks, +-16) through HipSadDecoder -> HipAlmeidaEstimator with
"Quarter pel" on and off.

The yardstick is the CPU chain computed here (integer: oracle.sad_flow -> oracle.solve_ypr_given; quarter-pel:
tests/indep_sad_qpel.py on the same winners -> the same solver), never the HIP output:
  (a) the HIP and CPU quarter-pel chains agree per pair to 1e-6 in every quaternion component (as test_accuracy_gpu.py asks
      of the integer chain);
  (b) slow_pan_0.01, LSQ: relative mean error < 0.10, the reference's own bound (almeida-estimator/src/lib.rs:347-348); the
      integer chain sits at 1.0 there (0.16 px per frame at the centre: every vector is zero);
  (c) pan_tilt_0.05, LSQ: HIP quarter-pel mean error <= 0.75 x the CPU integer chain's (ratio on the first three pairs on the
      CPU: 0.47; if the 24-frame CPU ratio is above 0.6 the bound is that ratio + 0.15);
  (d) RANSAC, the reference's default, all four clips, same seed: HIP quarter-pel mean error <= 0.75 x HIP integer mean error
      (the integer path is the full-pel decoder byte for byte; HIP and CPU RANSAC agree only to 1e-4 per component, so this
      one is not tied to the CPU chain).
Plain LSQ is NOT asserted to gain on every clip: on roll_0.3 its error comes from mismatched blocks, not from quantisation
(profiles/r07/accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

CLIPS = ["slow_pan_0.01", "pan_tilt_0.05", "pan_0.2", "roll_0.3"]


@pytest.fixture(scope="module")
def table():
    import accuracy_clips as ac
    import indep_sad_qpel as iq
    import oracle
    from ofps_amd import synth
    from ofps_amd.plugins import HipSadDecoder, StandardCamera
    clips = ac.clip_table(quick=True)
    res = {}
    for name in CLIPS:
        W, H, fov, eul, dis = clips[name]
        frames, truth = synth.rotation_clip(eul, W, H, fov, seed=21 + list(clips).index(name), distractor=dis)
        cam, ocam = StandardCamera(W / H, fov), oracle.camera(W / H, fov)
        row = {}
        for key, ransac, props in (("hip_i+lsq", False, {}), ("hip_q+lsq", False, {"Quarter pel": True}),
                                   ("hip_i+ransac", True, {}), ("hip_q+ransac", True, {"Quarter pel": True})):
            q, _, _ = ac.track(frames, cam, HipSadDecoder, ransac, **props)
            assert len(q) == len(truth)
            row[key] = dict(ac.stats(q, truth), q=q)
        qi, qq = [], []
        for k in range(len(truth)):
            ent_i, best_i = oracle.sad_flow(frames[k], frames[k + 1], 16, 16, threads=min(16, oracle.num_threads()))
            ent_q, _ = iq.refine(frames[k], frames[k + 1], 16, 16, best_i)
            qi.append(oracle.solve_ypr_given(ent_i, ocam)); qq.append(oracle.solve_ypr_given(ent_q, ocam))
        row["cpu_i+lsq"] = dict(ac.stats(np.array(qi), truth), q=np.array(qi))
        row["cpu_q+lsq"] = dict(ac.stats(np.array(qq), truth), q=np.array(qq))
        res[name] = row
        print(f"[qpel accuracy] {name}: " + "  ".join(f"{k} mean_err {v['mean_err_deg']:.5f} rel {v['rel_mean']:.4f}" for k, v in row.items()), flush=True)
    return res


def test_hip_and_cpu_quarter_pel_chains_agree_pair_by_pair(table):
    for clip, row in table.items():
        d = float(np.abs(row["hip_q+lsq"]["q"] - row["cpu_q+lsq"]["q"]).max())
        print(f"[qpel accuracy] {clip}: max |dq| HIP vs CPU quarter-pel chain {d:.2e}")
        assert d < 1e-6, (clip, d)
        assert float(np.abs(row["hip_i+lsq"]["q"] - row["cpu_i+lsq"]["q"]).max()) < 1e-6, clip


def test_slow_pan_is_seen_at_all(table):
    row = table["slow_pan_0.01"]
    print("[qpel accuracy] slow_pan_0.01 LSQ rel_mean: integer", row["cpu_i+lsq"]["rel_mean"], "quarter-pel HIP", row["hip_q+lsq"]["rel_mean"])
    assert row["cpu_i+lsq"]["rel_mean"] > 0.99                    # the integer chain cannot see this camera move
    assert row["hip_q+lsq"]["rel_mean"] < 0.10


def test_pan_tilt_lsq_error_drops(table):
    row = table["pan_tilt_0.05"]
    cpu_ratio = row["cpu_q+lsq"]["mean_err_deg"] / row["cpu_i+lsq"]["mean_err_deg"]
    bound = 0.75 if cpu_ratio <= 0.6 else cpu_ratio + 0.15
    print(f"[qpel accuracy] pan_tilt_0.05 LSQ: CPU ratio over 24 frames {cpu_ratio:.4f} -> bound {bound:.4f}; "
          f"HIP quarter-pel / CPU integer {row['hip_q+lsq']['mean_err_deg'] / row['cpu_i+lsq']['mean_err_deg']:.4f}")
    assert row["hip_q+lsq"]["mean_err_deg"] <= bound * row["cpu_i+lsq"]["mean_err_deg"]


@pytest.mark.parametrize("clip", CLIPS)
def test_ransac_error_drops_on_every_clip(table, clip):
    row = table[clip]
    print(f"[qpel accuracy] {clip} RANSAC: integer {row['hip_i+ransac']['mean_err_deg']:.5f} quarter-pel {row['hip_q+ransac']['mean_err_deg']:.5f} "
          f"ratio {row['hip_q+ransac']['mean_err_deg'] / row['hip_i+ransac']['mean_err_deg']:.4f}")
    assert row["hip_q+ransac"]["mean_err_deg"] <= 0.75 * row["hip_i+ransac"]["mean_err_deg"]
