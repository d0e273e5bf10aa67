"""Child process of tests/test_klt_fb_gpu.py: the multi-device dispatcher's workers read hip_klt's forward-backward check (OFPS_HIP_KLT_FB,
include/ofps_hip.h N3f) from the environment at ofps_hip_init only, like the batch decoder switch and the other settings, so the variables
have to be set before the library is loaded -- in a fresh process (pattern: tests/multi_klt_zm_child.py).  Two workers on device 0, the six
frames of klt_fb_cases.sequence() in two batches of three.  Prints one JSON object: per frame have_vectors, n_vectors, the kept records, the
quaternion (floats as uint32 bit patterns) and the island."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("OFPS_HIP_BATCH_DECODER") == "1" and int(os.environ.get("OFPS_HIP_KLT_FB", "0")) > 0
    import klt_fb_cases as fc
    from ofps_amd.runtime import MultiDevice
    f = np.ascontiguousarray(fc.sequence())
    _, H, W = f.shape
    cap = MultiDevice.batch_record_capacity(W, H)
    seed = int(os.environ.get("KLT_CHILD_SEED", "0"))
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    out = []
    md = MultiDevice([0, 0])
    try:
        ents = [np.zeros((3, cap, 4), np.float32) for _ in range(2)]
        tickets = [md.push_frames_async(f[3 * j:3 * j + 3], seed=seed + 3 * j, out_entries=ents[j]) for j in range(2)]
        for j, t in enumerate(tickets):
            for k, r in enumerate(md.frames_wait(t)):
                out.append({"have_vectors": r["have_vectors"], "n_vectors": r["n_vectors"], "entries": bits(ents[j][k][:r["n_vectors"]]),
                            "quat": bits(r["quat"]), "motion": r["motion"]})
    finally:
        md.close()
    print(json.dumps({"capacity": cap, "frames": out}))


if __name__ == "__main__":
    main()
