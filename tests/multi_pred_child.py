"""Child process of tests/test_sad_pred_gpu.py: the multi-device dispatcher's workers read the search levels and the predictor mode from
the environment variables OFPS_HIP_SAD_LEVELS / OFPS_HIP_SAD_PREDICTORS at ofps_hip_init only, so both have to be set before the library
is loaded -- in a fresh process (pattern: tests/multi_hier_child.py).  Prints one JSON object: the records of ofps_hip_multi_sad_flow in
both reference modes and of one streamed batch (floats as uint32 bit patterns)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("OFPS_HIP_SAD_LEVELS") == "2" and os.environ.get("OFPS_HIP_SAD_PREDICTORS") == "1"
    import sad_gate_cases as gc
    from ofps_amd.runtime import MultiDevice
    fr = np.ascontiguousarray(gc.frames())
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    out = {}
    md = MultiDevice([0, 0])
    try:
        for ref_mode in (0, 1):
            out[f"sad_flow_ref{ref_mode}"] = bits(md.sad_flow(fr, gc.BLOCK, gc.RANGE, ref_mode))
        ent = np.zeros((len(fr), gc.NBLK, 4), np.float32)
        t = md.push_frames_async(fr, block=gc.BLOCK, search_range=gc.RANGE, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1], out_entries=ent,
                                 **gc.FRAME_DETECTOR)
        res = md.frames_wait(t)
        out["stream"] = [{"have_vectors": r["have_vectors"], "entries": bits(ent[k]) if r["have_vectors"] else []} for k, r in enumerate(res)]
    finally:
        md.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
