"""Seeded inputs for hip_klt's chained batch (include/ofps_hip.h N3pb), shared by the CPU and GPU tests: the two ramp sequences of
tests/klt_pred_cases.py, read as chains (ref_mode 0), and "const4", nine frames cut from one canvas 4 px further each, read from its key frame
(ref_mode 1: the displacement of item k is 4 (k + 1) px); and what the restatement tests/indep_klt_batch_pred.py answers on them, computed
once per process and shared read-only.  Nothing here calls the library."""
import functools

import numpy as np

import indep_klt as ik
import indep_klt_batch_pred as ib
import klt_cases as kc
import klt_pred_cases as pc

W, H = pc.RAMP_W, pc.RAMP_H
RAMP_SET, DEFAULT_SET = pc.RAMP_SET, pc.DEFAULT_SET
CONST4_STEP, CONST4_PAIRS = 4, 8
SEQUENCES = {"ramp3": 0, "ramp4": 0, "const4": 1}            # name -> the ref_mode it is read in


@functools.lru_cache(maxsize=None)
def frames(name):
    """-> tuple of frames of 160 x 96"""
    if name != "const4":
        return pc.ramp_frames(name)
    canvas = kc.warp_pair(W + CONST4_STEP * CONST4_PAIRS, H, (0.0, 0.0))[0]
    fr = tuple(np.ascontiguousarray(canvas[:, o:o + W]) for o in range(0, CONST4_STEP * CONST4_PAIRS + 1, CONST4_STEP))
    for f in fr:
        f.setflags(write=False)
    return fr


def displacements(name):
    """the content's motion to the left, in px, of every item of the sequence in its ref_mode"""
    return pc.RAMPS[name] if name != "const4" else tuple(CONST4_STEP * (k + 1) for k in range(CONST4_PAIRS))


@functools.lru_cache(maxsize=None)
def expect(name, params, chained=True, fb_limit=0, mean_removal=False):
    """-> the restatement's answers for the items of the whole sequence, item 0 started from zero"""
    cell, r, min_score, min_eig, R, L, w, K = params
    out = ib.flow_batch_from(frames(name), L, w, K, SEQUENCES[name], None, chained, cell=cell, r=r, min_score=min_score, min_eig=min_eig,
                             max_residual=R, mean_removal=mean_removal, fb_limit=fb_limit)
    for o in out:
        for a in (o["slots"], o["residuals"], o["records"], o["guesses"]):
            a.setflags(write=False)
    return tuple(out)


def tail_frames(name, first):
    """the sequence without its items 0 .. first - 1, as a sequence of its own: the chain from frame `first` on, or the key frame and the frames
    behind frame `first`.  With prev_slots = item first - 1's slots its chained batch is expect(name, ...)[first:]"""
    fr = frames(name)
    return fr[first:] if SEQUENCES[name] == 0 else (fr[0],) + fr[first + 1:]


def table(name, params, chained, fb_limit=0):
    """per item (kept, kept and within 0.25 px, kept and wrong by >= 1 px)"""
    return [pc.ramp_counts(o, d) for o, d in zip(expect(name, params, chained, fb_limit), displacements(name))]


def kept(name, params, chained, fb_limit=0):
    return [int((o["slots"][:, 5] == ik.ST_KEPT).sum()) for o in expect(name, params, chained, fb_limit)]
