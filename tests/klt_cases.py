"""Seeded small inputs for hip_klt (include/ofps_hip.h N3), shared by the CPU and GPU tests.  Everything is a pure function of its
arguments; nothing here calls the library or the restatement."""
import functools

import numpy as np

from ofps_amd import synth

WARP = dict(roll_deg=0.5, zoom=1.004)


@functools.lru_cache(maxsize=None)
def warp_pair(W, H, shift):
    return synth.camera_warp_pair(W, H, shift=shift, seed=11, **WARP)


def warp_truth(W, H, shift, x, y):
    """Where the content of prev at pixel (x, y) lies in cur, minus (x, y): the inverse of the generator's map
    s = c + zoom * R(roll) * (p - c) + shift, which says where cur's pixel p samples prev."""
    cx, cy, a = (W - 1) / 2, (H - 1) / 2, np.deg2rad(WARP["roll_deg"])
    ux = (np.asarray(x, np.float64) - cx - shift[0]) / WARP["zoom"]
    uy = (np.asarray(y, np.float64) - cy - shift[1]) / WARP["zoom"]
    px = cx + np.cos(a) * ux + np.sin(a) * uy
    py = cy - np.sin(a) * ux + np.cos(a) * uy
    return px - x, py - y


@functools.lru_cache(maxsize=None)
def luma_pair():
    fr = synth.luma_sequence(2, 256, 192, 6)
    return fr[0], fr[1]


def luma_region_shift():
    """the planted integer motion of every 64 x 64 region of luma_pair(), as content motion prev -> cur: [ry, rx, 2]"""
    W, H, region, max_step, seed = 256, 192, 64, 6, synth.SEED0
    rx, ry = W // region, H // region
    ridx = np.arange(rx * ry, dtype=np.uint32)
    with np.errstate(over="ignore"):
        hx = synth._hash_u32(ridx * np.uint32(2654435761) + np.uint32((seed + 101) & 0xFFFFFFFF))
        hy = synth._hash_u32(hx + np.uint32(0x68E31DA4))
    ox = (hx % np.uint32(2 * max_step + 1)).astype(np.int64) - max_step
    oy = (hy % np.uint32(2 * max_step + 1)).astype(np.int64) - max_step
    # frame 1 samples the texture at its pixel + offset: content moves by -offset
    return np.stack([-ox, -oy], 1).reshape(ry, rx, 2)


def flat_pair(W=96, H=64, value=117):
    f = np.full((H, W), value, np.uint8)
    return f, f.copy()


@functools.lru_cache(maxsize=None)
def random_pair(W=96, H=64):
    fr = synth.random_luma(2, W, H, seed=synth.SEED0 + 5)
    return fr[0], fr[1]


def padded(img, pad):
    """-> (view [H, W] of a wider buffer whose padding holds 0xA5, stride)"""
    H, W = img.shape
    buf = np.full((H, W + pad), 0xA5, np.uint8)
    buf[:, :W] = img
    return buf[:, :W], W + pad


@functools.lru_cache(maxsize=None)
def edge_pair(W=128, H=96, shift=20):
    """content moves `shift` pixels to the left: features near the left edge leave the frame"""
    a, _ = warp_pair(W + shift, H, (0.0, 0.0))
    return np.ascontiguousarray(a[:, :W]), np.ascontiguousarray(a[:, shift:shift + W])


@functools.lru_cache(maxsize=None)
def repaint_pair(W=128, H=96):
    """the pair of a small shift with one region of cur repainted by unrelated texture"""
    a, b = warp_pair(W, H, (1.3, -0.6))
    other, _ = warp_pair(W, H, (40.0, 25.0))
    b = b.copy()
    b[24:72, 40:96] = other[::-1, ::-1][24:72, 40:96]
    return a, b


# (name, prev, cur) of every content case, at the sizes the issue names
def content_cases():
    out = [("warp96", *warp_pair(96, 64, (1.3, -0.6))), ("warp97", *warp_pair(97, 65, (1.3, -0.6))), ("warp320", *warp_pair(320, 192, (5.3, -4.6))),
           ("luma", *luma_pair()),
           ("flat", *flat_pair()), ("random", *random_pair()), ("edge", *edge_pair()), ("repaint", *repaint_pair())]
    return out


# parameter sets (cell, r, min_score, min_eig, R, L, w, K): every value of the issue's lists appears at least once
PARAM_SETS = [
    (16, 2, 1, 1, 0, 2, 4, 10),
    (8, 1, 1, 1, 64, 1, 1, 1),
    (32, 3, 1, 400, 160, 3, 7, 30),
    (16, 2, 50000, 1, 64, 4, 4, 10),
]
# the decoder's defaults on the 320 x 192 pair -- 5 px of motion doubled over four levels under the 225-pixel window --, without and with a
# residual limit.  That pair runs these two sets alone (its restatement is the slowest of the cases'), every other case all of PARAM_SETS
DEFAULT_SET = (16, 2, 1, 1, 0, 4, 7, 10)


def param_sets(name):
    return [DEFAULT_SET, (16, 2, 1, 1, 160, 4, 7, 10)] if name == "warp320" else PARAM_SETS
