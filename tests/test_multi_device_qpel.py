"""-m gpu: the in-process multi-device dispatcher (ofps_hip_multi_*) at motion scale 4.  Its workers take the scale from the
environment variable OFPS_HIP_SAD_MOTION_SCALE at ofps_hip_init only, so the dispatcher runs in a fresh child process with the
variable set before the library is loaded (tests/multi_qpel_child.py; two workers on device 0).  The parent compares what the
child prints with the CPU chain: records against tests/indep_sad_qpel.py bit for bit, the streamed frames' island and quaternion
against the oracle's detector and LSQ solver on those records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

import indep_sad_qpel as iq
import multi_qpel_child as child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_device_workers_take_scale_four_from_the_environment():
    env = dict(os.environ, OFPS_HIP_SAD_MOTION_SCALE="4")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_qpel_child.py")], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    fr = child.frames()
    W, H, B, R, F = child.W, child.H, child.B, child.R, child.F
    nblk = (W // B) * (H // B)

    def expect(prev, cur):
        _, best_i = oracle.sad_flow(prev, cur, B, R)
        ent, best = iq.refine(prev, cur, B, R, best_i)
        return ent, best, best_i

    fractional = 0
    for ref_mode in (0, 1):
        ent_g = np.array(got[f"sad_flow_ref{ref_mode}"], np.uint32).reshape(F - 1, nblk, 4)
        for k in range(F - 1):
            ent_e, best, best_i = expect(fr[0] if ref_mode else fr[k], fr[k + 1])
            np.testing.assert_array_equal(ent_g[k], ent_e.view(np.uint32), err_msg=f"ref_mode {ref_mode} pair {k}")
            fractional += int(((best[:, :2] % 4) != 0).any(axis=1).sum())
    assert fractional > 0                                                          # scale 1 would not pass by accident

    cam = oracle.camera(child.ASPECT, child.FOV)
    stream = got["stream"]
    assert len(stream) == F and not stream[0]["have_vectors"]
    for k in range(1, F):
        ent_e, _, _ = expect(fr[k - 1], fr[k])
        assert stream[k]["have_vectors"]
        np.testing.assert_array_equal(np.array(stream[k]["entries"], np.uint32).reshape(nblk, 4), ent_e.view(np.uint32), err_msg=f"frame {k}")
        det_e = oracle.detect_motion(ent_e)
        assert (stream[k]["motion"] is None) == (det_e is None)
        if det_e is not None:
            assert stream[k]["motion"] == [det_e[0], det_e[1].shape[0]]            # island id and the field's side (the stream returns no field)
        quat = np.array(stream[k]["quat"], np.uint32).view(np.float32)
        np.testing.assert_allclose(quat, oracle.solve_ypr_given(ent_e, cam), atol=2e-6, rtol=0, err_msg=f"frame {k}")
