"""Seeded inputs for hip_klt's batch form (include/ofps_hip.h N3b), shared by the CPU and GPU tests: two frame sequences, their parameter
sets (cell, r, min_score, min_eig, R, L, w, K) and what the restatement tests/indep_klt.py keeps per item.  Pure functions of their arguments;
the restatement's answers are computed once per process and shared read-only."""
import functools

import numpy as np

from ofps_amd import synth

import indep_klt as ik
import klt_cases as kc

# six frames of 128 x 96: five pairs, 48 slots at cell 16
SMALL = (6, 128, 96, 3)
SMALL_SETS = [kc.PARAM_SETS[0], (8, 1, 1, 1, 64, 1, 1, 1), (32, 3, 1, 400, 160, 3, 7, 30), (16, 2, 50000, 1, 64, 4, 4, 10), kc.DEFAULT_SET]
SMALL_KEPT = {SMALL_SETS[0]: (48, 46, 48, 48, 46), SMALL_SETS[1]: (177, 76, 162, 87, 75), SMALL_SETS[2]: (0, 0, 0, 0, 0),
              SMALL_SETS[3]: (1, 1, 3, 1, 1), SMALL_SETS[4]: (48, 46, 48, 48, 47)}
ALL_FLAT = SMALL_SETS[2]
FEW = SMALL_SETS[3]                      # items below the estimator's minimum
KEY_SETS = [SMALL_SETS[0], SMALL_SETS[1]]        # ref_mode 1

# three frames of 384 x 224 at cell 8: 1,344 slots per item, above the 1,024 records of one round of the segmented compaction
BIG = (3, 384, 224, 3)
BIG_SETS = [(8, 1, 1, 1, 64, 1, 1, 1), (8, 2, 1, 1, 0, 3, 4, 10)]
BIG_KEPT = {BIG_SETS[0]: (856, 733), BIG_SETS[1]: (1337, 1326)}      # the second set's restatement takes 5 s: the GPU test compares it with the one-pair form


@functools.lru_cache(maxsize=None)
def sequence(spec):
    fr = synth.luma_sequence(*spec)
    fr.setflags(write=False)
    return fr


def pair_of(k, ref_mode):
    return (0, k + 1) if ref_mode else (k, k + 1)


@functools.lru_cache(maxsize=None)
def expect(spec, params, ref_mode=0):
    """-> tuple over the items of the restatement's dicts (features, slots, records, count, residuals)"""
    cell, r, min_score, min_eig, R, L, w, K = params
    fr = sequence(spec)
    out = []
    for k in range(len(fr) - 1):
        a, b = pair_of(k, ref_mode)
        out.append(ik.flow(fr[a], fr[b], L, w, K, cell, r, min_score, min_eig, R))
    return tuple(out)


def padded_sequence(spec, pad, extra_rows):
    """-> (view [n, H, W] of a buffer whose rows are W + pad bytes and whose frames lie (H + extra_rows) rows apart, filler 0xA5)"""
    fr = sequence(spec)
    n, H, W = fr.shape
    buf = np.full((n, H + extra_rows, W + pad), 0xA5, np.uint8)
    buf[:, :H, :W] = fr
    return buf[:, :H, :W]
