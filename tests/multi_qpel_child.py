"""Child process of tests/test_multi_device_qpel.py: the multi-device dispatcher's workers read the motion scale from the
environment variable OFPS_HIP_SAD_MOTION_SCALE at ofps_hip_init only, so the variable has to be set before the library is loaded --
in a fresh process.  Prints one JSON object: the records of ofps_hip_multi_sad_flow in both reference modes and, per frame of one
streamed batch sequence, the records, the island and the quaternion (all floats as uint32 bit patterns)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B, R, F = 320, 192, 16, 16, 5
ASPECT, FOV = 16 / 9, 22.275


def frames():
    from ofps_amd import synth
    return synth.luma_sequence(F, W, H, max_step=3, seed=3, region=4096, noise=1)      # sub-pel global motion + sensor noise


def main():
    assert os.environ.get("OFPS_HIP_SAD_MOTION_SCALE") == "4"
    from ofps_amd.runtime import MultiDevice
    fr = frames()
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    out = {}
    md = MultiDevice([0, 0])
    try:
        for ref_mode in (0, 1):
            out[f"sad_flow_ref{ref_mode}"] = bits(md.sad_flow(fr, B, R, ref_mode))
        nblk = (W // B) * (H // B)
        stream = []
        ent = [np.zeros((n, nblk, 4), np.float32) for n in (2, 3)]
        batches = [np.ascontiguousarray(fr[:2]), np.ascontiguousarray(fr[2:])]      # alive until frames_wait, as the API asks
        tickets = [md.push_frames_async(batches[k], block=B, search_range=R, aspect=ASPECT, fov_y_deg=FOV, out_entries=ent[k]) for k in range(2)]
        res = md.frames_wait(tickets[0]) + md.frames_wait(tickets[1])               # one batch per worker, both in flight
        for k, r in enumerate(res):
            e = ent[0][k] if k < 2 else ent[1][k - 2]
            stream.append({"have_vectors": r["have_vectors"], "entries": bits(e) if r["have_vectors"] else [],
                           "motion": r["motion"], "quat": bits(r["quat"])})
        out["stream"] = stream
    finally:
        md.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
