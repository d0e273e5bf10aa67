"""Seeded inputs for hip_klt's intra test and scene-cut rule (include/ofps_hip.h N3i), shared by the CPU and GPU tests: built from
tests/klt_cases.py and ofps_amd.synth.  Everything is a pure function of its arguments; nothing here calls the library or the restatement."""
import functools

import numpy as np

import klt_cases as kc
from ofps_amd import synth

SHIFT = (1.3, -0.6)
SET = (2, 4, 10)                                             # (L, w, K) of the planted pairs
Q = 8                                                        # hip_sad's recommended ratio, which separates the planted pairs
REPAINT = (24, 72, 40, 96)                                   # klt_cases.repaint_pair's rectangle: rows 24-71, columns 40-95


def other(W, H):
    """unrelated content of the same texture: another pair's first frame, turned by 180 degrees"""
    return np.ascontiguousarray(kc.warp_pair(W, H, (40.0, 25.0))[0][::-1, ::-1])


@functools.lru_cache(maxsize=None)
def clean_pair(W=128, H=96):
    return kc.warp_pair(W, H, SHIFT)


@functools.lru_cache(maxsize=None)
def cut_pair(W=128, H=96):
    return kc.warp_pair(W, H, SHIFT)[0], other(W, H)


def repaint_pair():
    return kc.repaint_pair()


@functools.lru_cache(maxsize=None)
def cut_sequence(W=128, H=96):
    """four frames: a clean pair, the cut, and a clean pair of the new scene (the same small warp of another seed's texture)"""
    a, b = kc.warp_pair(W, H, SHIFT)
    c, d = synth.camera_warp_pair(W, H, shift=SHIFT, seed=12, **kc.WARP)
    return np.stack([a, b, c, d])


@functools.lru_cache(maxsize=None)
def three_pairs(W=128, H=96):
    """(clean, cut, repaint) as three unrelated pairs -> [(prev, cur)] * 3"""
    return [clean_pair(W, H), cut_pair(W, H), kc.repaint_pair(W, H)]


@functools.lru_cache(maxsize=None)
def key_sequence(W=128, H=96):
    """a key frame and three current frames: its clean partner, unrelated content, the repainted partner (ref_mode 1)"""
    a, b = clean_pair(W, H)
    return np.stack([a, b, other(W, H), kc.repaint_pair(W, H)[1]])


def padded_pair(prev, cur, pad=13):
    """both frames as views of wider buffers with one stride"""
    p, s = kc.padded(prev, pad)
    c, _ = kc.padded(cur, pad)
    return p, c, s
