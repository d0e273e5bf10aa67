#!/usr/bin/env python3
"""Writes tests/golden/sad_qpel.npz: small frame pairs, the integer winners of the CPU oracle's full search and the
quarter-pel refinement (N1q) of tests/indep_sad_qpel.py on top: (Dx, Dy, SAD) and the records.  Not outputs of the reference
(which has no block matcher): fixed bytes so that neither the restatement nor the HIP kernel can drift silently.

Run from the repo root:  python tests/golden/generate_sad_qpel.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from ofps_amd import synth  # noqa: E402
import indep_sad_qpel as iq  # noqa: E402

CASES = [("a", 96, 64, 16, 8), ("b", 64, 48, 8, 8), ("c", 60, 48, 12, 5)]       # name, W, H, block, range


def main():
    out = {}
    for name, W, H, B, R in CASES:
        fr = synth.luma_sequence(2, W, H, max_step=min(R, 3), seed=700 + W)
        _, best_i = oracle.sad_flow(fr[0], fr[1], B, R)
        ent, best = iq.refine(fr[0], fr[1], B, R, best_i)
        out[f"{name}_frames"] = fr
        out[f"{name}_geom"] = np.array([W, H, B, R], np.int32)
        out[f"{name}_best_int"] = best_i
        out[f"{name}_best"] = best
        out[f"{name}_entries"] = ent
    np.savez_compressed(os.path.join(HERE, "sad_qpel.npz"), **out)


if __name__ == "__main__":
    main()
