"""Child process of tests/test_klt_intra_gpu.py: the multi-device dispatcher's workers follow hip_klt's intra test and scene-cut rule
(OFPS_HIP_KLT_INTRA, OFPS_HIP_KLT_CUT; include/ofps_hip.h N3i).  Their contexts read the environment at ofps_hip_init only, so the variables
have to be set before the dispatcher is made -- in a fresh process (pattern: tests/multi_klt_fb_child.py).  Two workers on device 0, the four
frames of klt_intra_cases.cut_sequence() in two batches of two.  Prints one JSON object: what a plain context made in this environment reads,
and per frame have_vectors, n_vectors, the kept records and the quaternion (floats as uint32 bit patterns) and the island."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("OFPS_HIP_BATCH_DECODER") == "1" and "OFPS_HIP_KLT_INTRA" in os.environ and "OFPS_HIP_KLT_CUT" in os.environ
    import klt_intra_cases as xc
    from ofps_amd.runtime import HipContext, MultiDevice
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    f = np.ascontiguousarray(xc.cut_sequence())
    _, H, W = f.shape
    cap = MultiDevice.batch_record_capacity(W, H)
    seed = int(os.environ.get("KLT_CHILD_SEED", "0"))
    c = HipContext(0)
    seen = [c.get_klt_intra(), c.get_klt_cut()]
    c.close()
    out = []
    md = MultiDevice([0, 0])
    try:
        cuts = ((0, 2), (2, 4))
        ents = [np.zeros((b - a, cap, 4), np.float32) for a, b in cuts]
        tickets = [md.push_frames_async(f[a:b], seed=seed + a, out_entries=ents[j]) for j, (a, b) in enumerate(cuts)]
        for j, t in enumerate(tickets):
            for k, r in enumerate(md.frames_wait(t)):
                out.append({"have_vectors": r["have_vectors"], "n_vectors": r["n_vectors"], "entries": bits(ents[j][k][:r["n_vectors"]]),
                            "quat": bits(r["quat"]), "motion": r["motion"]})
    finally:
        md.close()
    print(json.dumps({"capacity": cap, "settings_seen": seen, "frames": out}))


if __name__ == "__main__":
    main()
