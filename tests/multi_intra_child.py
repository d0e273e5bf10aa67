"""Child process of tests/test_sad_intra_gpu.py: the multi-device dispatcher's workers read the intra test's ratio, the cut rule's percentage
and the batch filter switch from the environment variables OFPS_HIP_SAD_INTRA, OFPS_HIP_SAD_CUT and OFPS_HIP_SAD_BATCH_FILTER at ofps_hip_init
only, so the variables have to be set before the library is loaded -- in a fresh process (pattern: tests/multi_prefilter_child.py).  Two
workers on device 0, the stream of tests/sad_intra_cases.py in two batches of three.  Prints one JSON list: per frame have_vectors,
n_vectors, the kept records, the quaternion (floats as uint32 bit patterns) and the island."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("OFPS_HIP_SAD_INTRA") and os.environ.get("OFPS_HIP_SAD_CUT") and os.environ.get("OFPS_HIP_SAD_BATCH_FILTER") == "1"
    import sad_intra_cases as ic
    import sad_median_cases as mc
    from ofps_amd.runtime import MultiDevice
    f = np.ascontiguousarray(ic.stream_frames())
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    out = []
    md = MultiDevice([0, 0])
    try:
        ents = [np.zeros((3, mc.SCENE_NBLK, 4), np.float32) for _ in range(2)]
        tickets = [md.push_frames_async(f[3 * j:3 * j + 3], block=mc.SCENE_B, search_range=mc.SCENE_R, aspect=mc.SCENE_CAM[0],
                                        fov_y_deg=mc.SCENE_CAM[1], seed=mc.SCENE_SEED + 3 * j, out_entries=ents[j], **mc.SCENE_DETECTOR)
                   for j in range(2)]
        for j, t in enumerate(tickets):
            for k, r in enumerate(md.frames_wait(t)):
                out.append({"have_vectors": r["have_vectors"], "n_vectors": r["n_vectors"], "entries": bits(ents[j][k][:r["n_vectors"]]),
                            "quat": bits(r["quat"]), "motion": r["motion"]})
    finally:
        md.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
