"""Seeded inputs for hip_klt's mean removal (include/ofps_hip.h N3m), shared by the CPU and GPU tests: the frames of tests/klt_cases.py
relit, the pair on which a brightness offset clips nothing, the batch sequence with every second frame raised, and what the restatement
tests/indep_klt_zm.py answers on them -- computed once per process and shared read-only.  Nothing here calls the library."""
import functools

import numpy as np

import indep_klt as ik
import indep_klt_zm as iz
import klt_batch_cases as bc
import klt_cases as kc

SMALL_SHIFT = (1.3, -0.6)
SET0 = kc.PARAM_SETS[0]                                   # (16, 2, 1, 1, 0, 2, 4, 10)
SET0_R64 = (16, 2, 1, 1, 64, 2, 4, 10)
RELIT_OFFSETS = (20, -20, 40)                             # all three clip pixels of the 96 x 64 pair
INVARIANT_OFFSETS = (20, -20, 60, -60)                    # none clips a pixel of the compressed pair
SMALL_NAMES = tuple(name for name, _, _ in kc.content_cases() if name != "warp320")


def relit(img, offset):
    """clip(img + offset)"""
    return np.clip(img.astype(np.int64) + offset, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (prev, cur) of: a content case of klt_cases by its name; "warp96+20" and the like: that case with cur relit; "inv": the 96 x 64
    pair compressed to 62 .. 181, "inv+20" and the like: its cur raised, which clips nothing"""
    base, sign, off = name.partition("+") if "+" in name else name.partition("-")
    offset = int(sign + off) if sign else 0
    if base == "inv":
        prev, cur = kc.warp_pair(96, 64, SMALL_SHIFT)
        prev, cur = (prev >> 1) + 60, (cur >> 1) + 60
        moved = cur.astype(np.int64) + offset
        assert 0 <= moved.min() and moved.max() <= 255
        out = prev, moved.astype(np.uint8)
    else:
        prev, cur = {n: (p, c) for n, p, c in kc.content_cases()}[base]
        out = prev, (relit(cur, offset) if offset else cur)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expect(name, params, mean_removal=True):
    cell, r, min_score, min_eig, R, L, w, K = params
    prev, cur = case(name)
    return (iz if mean_removal else ik).flow(prev, cur, L, w, K, cell, r, min_score, min_eig, R)


def status_counts(out):
    return np.bincount(out["slots"][:, 5], minlength=5)


# ---- the batch form: klt_batch_cases' six frames of 128 x 96 with frames 1, 3 and 5 raised by 20 (clipped): every pair of the chain crosses a
# brightness step, and three of the key mode's five
@functools.lru_cache(maxsize=None)
def flicker_sequence():
    fr = bc.sequence(bc.SMALL).copy()
    for k in (1, 3, 5):
        fr[k] = relit(fr[k], 20)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def flicker_expect(params, ref_mode=0, mean_removal=True):
    """-> tuple over the items of the restatement's dicts"""
    cell, r, min_score, min_eig, R, L, w, K = params
    fr = flicker_sequence()
    m = iz if mean_removal else ik
    return tuple(m.flow(fr[a], fr[b], L, w, K, cell, r, min_score, min_eig, R) for a, b in (bc.pair_of(k, ref_mode) for k in range(len(fr) - 1)))
