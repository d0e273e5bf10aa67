"""Child process of tests/test_sad_prefilter_gpu.py: the multi-device dispatcher's workers read the mean removal's radius from the
environment variable OFPS_HIP_SAD_PREFILTER at ofps_hip_init only, so the variable has to be set before the library is loaded -- in a fresh
process (pattern: tests/multi_hier_child.py).  Prints one JSON object: the records of ofps_hip_multi_sad_flow in both reference modes and of
one streamed batch (floats as uint32 bit patterns)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("OFPS_HIP_SAD_PREFILTER") == "4"
    import sad_prefilter_cases as pc
    from ofps_amd.runtime import MultiDevice
    fr = np.ascontiguousarray(pc.sequence())
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    out = {}
    md = MultiDevice([0, 0])
    try:
        for ref_mode in (0, 1):
            out[f"sad_flow_ref{ref_mode}"] = bits(md.sad_flow(fr, pc.SEQ_B, pc.SEQ_R, ref_mode))
        ent = np.zeros((len(fr), pc.SEQ_NBLK, 4), np.float32)
        t = md.push_frames_async(fr, block=pc.SEQ_B, search_range=pc.SEQ_R, aspect=pc.SEQ_CAM[0], fov_y_deg=pc.SEQ_CAM[1], out_entries=ent,
                                 **pc.SEQ_DETECTOR)
        res = md.frames_wait(t)
        out["stream"] = [{"have_vectors": r["have_vectors"], "entries": bits(ent[k]) if r["have_vectors"] else []} for k, r in enumerate(res)]
    finally:
        md.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
