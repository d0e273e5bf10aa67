"""Seeded inputs for hip_klt's forward-backward check (include/ofps_hip.h N3f), shared by the CPU and GPU tests: the pairs of
tests/klt_cases.py and tests/klt_zm_cases.py, and what the restatement tests/indep_klt_fb.py answers on them -- both passes of every
feature computed once per process, the answer at a limit made from them, all shared read-only.  Nothing here calls the library."""
import functools

import numpy as np

import indep_klt as ik
import indep_klt_fb as ifb
import klt_batch_cases as bc
import klt_cases as kc
import klt_zm_cases as zc

LIMITS = (1, 16, 64, 4096)
SET0 = kc.PARAM_SETS[0]
SMALL_NAMES = zc.SMALL_NAMES
REPAINT_RECT = (40, 96, 24, 72)                           # x0, x1, y0, y1 of klt_cases.repaint_pair's repainted rectangle


def case(name):
    """klt_zm_cases.case: a content case by name, "warp96+20" and the like relit, "inv", "inv+20" ..."""
    return zc.case(name)


@functools.lru_cache(maxsize=None)
def both(name, params, mean_removal=False):
    cell, r, min_score, min_eig, R, L, w, K = params
    prev, cur = case(name)
    out = ifb.flow_all(prev, cur, L, w, K, cell, r, min_score, min_eig, R, mean_removal)
    for a in (out["fwd"], out["back"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expect(name, params, fb_limit, mean_removal=False):
    """-> the restatement's dict (slots, residuals, records, count, features) with the check at fb_limit, 0 = off"""
    out = ifb.at_limit(both(name, params, mean_removal), fb_limit)
    for a in (out["slots"], out["residuals"], out["records"]):
        a.setflags(write=False)
    return out


def quads(out):
    """what ofps_hip_klt_track answers on the kept-or-not features of `out`: -> (points int32 [n, 2], quads int32 [n, 4])"""
    s = out["slots"]
    has = s[:, 5] != ik.ST_NONE
    q = np.stack([s[has, 3], s[has, 4], out["residuals"][has], s[has, 5]], 1).astype(np.int32)
    zero = ~np.isin(q[:, 3], (ik.ST_KEPT, ik.ST_RESIDUAL, ifb.ST_NO_RETURN))
    q[zero, :3] = 0
    return np.ascontiguousarray(s[has, :2]), q


def truth(name, x, y):
    """the planted content motion prev -> cur at the pixels (x, y) of a content case, in pixels: -> (tx, ty)"""
    x, y = np.asarray(x), np.asarray(y)
    if name == "warp96":
        return kc.warp_truth(96, 64, (1.3, -0.6), x, y)
    if name == "repaint":
        return kc.warp_truth(128, 96, (1.3, -0.6), x, y)
    if name == "warp320":
        return kc.warp_truth(320, 192, (5.3, -4.6), x, y)
    if name == "edge":
        return np.full(x.shape, -20.0), np.zeros(x.shape)
    if name == "luma":
        sh = kc.luma_region_shift()[y // 64, x // 64]
        return sh[..., 0].astype(np.float64), sh[..., 1].astype(np.float64)
    raise KeyError(name)


def errors(name, out):
    """-> (kept mask over the slots, the kept slots' distance from the planted motion in pixels)"""
    s = out["slots"]
    kept = s[:, 5] == ik.ST_KEPT
    tx, ty = truth(name, s[kept, 0], s[kept, 1])
    return kept, np.hypot(s[kept, 3] / 256.0 - tx, s[kept, 4] / 256.0 - ty)


def in_repaint(s):
    x0, x1, y0, y1 = REPAINT_RECT
    return (s[:, 0] >= x0) & (s[:, 0] < x1) & (s[:, 1] >= y0) & (s[:, 1] < y1)


# ---- the batch form: klt_batch_cases' six frames of 128 x 96, whose pairs the restatement answers one by one
@functools.lru_cache(maxsize=None)
def sequence(flicker=False):
    return zc.flicker_sequence() if flicker else bc.sequence(bc.SMALL)


@functools.lru_cache(maxsize=None)
def sequence_expect(params, ref_mode, fb_limit, mean_removal=False, flicker=False):
    cell, r, min_score, min_eig, R, L, w, K = params
    fr = sequence(flicker)
    return tuple(ifb.flow(fr[a], fr[b], L, w, K, cell, r, min_score, min_eig, R, mean_removal, fb_limit)
                 for a, b in (bc.pair_of(k, ref_mode) for k in range(len(fr) - 1)))
