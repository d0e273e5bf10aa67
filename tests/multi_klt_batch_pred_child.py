"""Child process of tests/test_klt_batch_pred_gpu.py: the multi-device dispatcher's workers ignore hip_klt's two prediction settings
(OFPS_HIP_KLT_PREDICTION, OFPS_HIP_KLT_BATCH_PREDICTION; include/ofps_hip.h N3pb).  Their contexts read the environment at ofps_hip_init only,
so the variables have to be set before a dispatcher is made -- in a fresh process (pattern: tests/multi_klt_fb_child.py), which makes two
dispatchers one after the other: one with both variables set, one with neither.  Two workers on device 0, the seven frames of
klt_pred_cases.ramp_frames("ramp3") in batches of four and three.  Prints one JSON object: per dispatcher and frame have_vectors, n_vectors, the
kept records, the quaternion (floats as uint32 bit patterns) and the island; and what a plain context made in each environment reads."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("OFPS_HIP_KLT_PREDICTION", "OFPS_HIP_KLT_BATCH_PREDICTION")


def run(f, cap, seed):
    from ofps_amd.runtime import HipContext, MultiDevice
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()
    c = HipContext(0)
    seen = [c.get_klt_prediction(), c.get_klt_batch_prediction()]
    c.close()
    out = []
    md = MultiDevice([0, 0])
    try:
        cuts = ((0, 4), (4, 7))
        ents = [np.zeros((b - a, cap, 4), np.float32) for a, b in cuts]
        tickets = [md.push_frames_async(f[a:b], seed=seed + a, out_entries=ents[j]) for j, (a, b) in enumerate(cuts)]
        for j, t in enumerate(tickets):
            for k, r in enumerate(md.frames_wait(t)):
                out.append({"have_vectors": r["have_vectors"], "n_vectors": r["n_vectors"], "entries": bits(ents[j][k][:r["n_vectors"]]),
                            "quat": bits(r["quat"]), "motion": r["motion"]})
    finally:
        md.close()
    return seen, out


def main():
    assert os.environ.get("OFPS_HIP_BATCH_DECODER") == "1" and not any(n in os.environ for n in NAMES)
    import klt_pred_cases as pc
    from ofps_amd.runtime import MultiDevice
    f = np.ascontiguousarray(np.stack(pc.ramp_frames("ramp3")))
    _, H, W = f.shape
    cap = MultiDevice.batch_record_capacity(W, H)
    seed = int(os.environ.get("KLT_CHILD_SEED", "0"))
    for n in NAMES:
        os.environ[n] = "1"
    seen_both, both = run(f, cap, seed)
    for n in NAMES:
        del os.environ[n]
    seen_neither, neither = run(f, cap, seed)
    print(json.dumps({"capacity": cap, "settings_seen": {"both": seen_both, "neither": seen_neither}, "both": both, "neither": neither}))


if __name__ == "__main__":
    main()
