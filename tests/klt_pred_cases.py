"""Seeded inputs for hip_klt's motion prediction (include/ofps_hip.h N3p), shared by the CPU and GPU tests: two ramp sequences -- frames cut
from one canvas whose content moves a growing number of pixels to the left per pair --, the small content pairs of tests/klt_cases.py with
caller-given guesses, hand-made slot tables for the predictor, and what the restatement tests/indep_klt_pred.py answers on them, computed
once per process and shared read-only.  Nothing here calls the library."""
import functools

import numpy as np

import indep_klt as ik
import indep_klt_pred as ip
import klt_cases as kc

RAMP_W, RAMP_H = 160, 96
RAMPS = {"ramp3": (3, 6, 9, 12, 15, 18), "ramp4": (4, 8, 12, 16, 20, 24, 28, 32)}
RAMP_SET = (16, 2, 1, 1, 0, 2, 4, 10)                        # cell, r, min_score, min_eig, R, L, w, K: the table's setting
DEFAULT_SET = kc.DEFAULT_SET                                 # the decoder's defaults: levels 4, radius 7


@functools.lru_cache(maxsize=None)
def ramp_frames(name):
    """-> tuple of len(steps) + 1 frames of 160 x 96: frame k is the canvas from column o_k, o the running sum of the steps"""
    steps = RAMPS[name]
    canvas = kc.warp_pair(RAMP_W + sum(steps), RAMP_H, (0.0, 0.0))[0]
    o = np.concatenate([[0], np.cumsum(steps)])
    fr = tuple(np.ascontiguousarray(canvas[:, k:k + RAMP_W]) for k in o)
    for f in fr:
        f.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def ramp_expect(name, params, predict_on, fb_limit=0, mean_removal=False):
    """-> the restatement's answers for the pairs of the sequence in order, each started from the one before (or, predict_on False, from zero)"""
    cell, r, min_score, min_eig, R, L, w, K = params
    out = ip.flow_chain(ramp_frames(name), L, w, K, predict_on, cell=cell, r=r, min_score=min_score, min_eig=min_eig, max_residual=R,
                        mean_removal=mean_removal, fb_limit=fb_limit)
    for o in out:
        for a in (o["slots"], o["residuals"], o["records"], o["guesses"]):
            a.setflags(write=False)
    return tuple(out)


def ramp_counts(out, step):
    """one pair's answer -> (kept, kept and within 0.25 px, kept and wrong by >= 1 px); the error is max(|dqx / 256 + step|, |dqy / 256|)"""
    s = out["slots"]
    k = s[s[:, 5] == ik.ST_KEPT]
    err = np.maximum(np.abs(k[:, 3] / 256.0 + step), np.abs(k[:, 4] / 256.0))
    return len(k), int((err <= 0.25).sum()), int((err >= 1.0).sum())


def ramp_table(name, params, predict_on, fb_limit=0):
    return [ramp_counts(o, st) for o, st in zip(ramp_expect(name, params, predict_on, fb_limit), RAMPS[name])]


# ---- the small content pairs with caller-given guesses
SMALL_NAMES = ("warp96", "warp97", "edge", "repaint")
_SIZES = {"warp96": (96, 64), "warp97": (97, 65), "edge": (128, 96), "repaint": (128, 96)}


def case(name):
    return {n: (p, c) for n, p, c in kc.content_cases()}[name]


def truth(name, x, y):
    """the planted content motion prev -> cur at the pixels (x, y), in pixels: -> (tx, ty)"""
    x, y = np.asarray(x), np.asarray(y)
    if name == "edge":
        return np.full(x.shape, -20.0), np.zeros(x.shape)
    W, H = _SIZES[name]
    return kc.warp_truth(W, H, (1.3, -0.6), x, y)


@functools.lru_cache(maxsize=None)
def points(name, cell=16, r=2, min_score=1):
    """the features of the case's prev frame that exist: int32 [n, 2]"""
    ft = ik.features(case(name)[0], cell, r, min_score)
    pts = np.ascontiguousarray(ft[ft[:, 0] >= 0, :2], np.int32)
    pts.setflags(write=False)
    return pts


GUESS_KINDS = ("zero", "truth", "leave", "far")


def guesses(name, kind, pts):
    """int32 [n, 2] in 1/256 pixel.  zero; truth: the planted motion rounded; leave: a guess whose start lies outside the frame for every
    point of the frame, and so does its negation's (N3f's backward pass): more than the frame's width, mixed signs and odd values; far: beyond +-2^23 in one component or both (the host form refuses it, the _dev form starts from
    zero), with in-range guesses in between"""
    n = len(pts)
    g = np.zeros((n, 2), np.int32)
    if kind == "truth":
        tx, ty = truth(name, pts[:, 0], pts[:, 1])
        g[:, 0] = np.rint(256.0 * tx); g[:, 1] = np.rint(256.0 * ty)
    elif kind == "leave":
        W, H = _SIZES[name]
        k = np.arange(n)
        g[:, 0] = np.where(k % 2 == 0, -256 * (W + 3) - 1 - 2 * k, 256 * (W + 2) + 77 + 2 * k)
        g[:, 1] = np.where(k % 3 == 0, 256 * (H + 5) + 1, -131)
    elif kind == "far":
        k = np.arange(n)
        g[:, 0] = np.where(k % 3 == 0, (1 << 23) + 1, np.where(k % 3 == 1, -333, -(1 << 31)))
        g[:, 1] = np.where(k % 2 == 0, -(1 << 23) - 1, 257)
        g[k % 6 == 1] = (-333, 257)                          # in range: tracked from the guess
    elif kind != "zero":
        raise KeyError(kind)
    return g


@functools.lru_cache(maxsize=None)
def track_expect(name, params, kind, mean_removal=False, fb_limit=0):
    """-> (points, guesses, quads int32 [n, 4]) of the restatement; the points are the features of the set's cell and score radius"""
    cell, r, min_score, min_eig, R, L, w, K = params
    prev, cur = case(name)
    pts = points(name, cell, r, min_score)
    gs = guesses(name, kind, pts)
    q = ip.track_from(prev, cur, pts, gs, L, w, K, min_eig, R, mean_removal, fb_limit)
    for a in (gs, q):
        a.setflags(write=False)
    return pts, gs, q


# ---- hand-made slot tables for the predictor: (name, W, H, cell, slots int32 [n, 6])
def _table(W, H, cell, fill):
    nx, ny = ik.slot_grid(W, H, cell)
    s = np.zeros((ny, nx, 6), np.int32)
    for cy in range(ny):
        for cx in range(nx):
            s[cy, cx] = fill(cx, cy, nx, ny)
    return s.reshape(-1, 6)


def _hash(cx, cy, salt):
    return ((cx * 73856093) ^ (cy * 19349663) ^ (salt * 83492791)) & 0xFFFF


def predictor_tables():
    out = []
    # every k from 0 to 5 around the centre of a 5 x 5 lattice: the centre and its four neighbours kept one after another
    order = ((2, 2), (1, 2), (3, 2), (2, 1), (2, 3))
    vals = ((-7, 301), (12, -5), (-1023, 9), (5, 5), (-3, -777))
    for k in range(6):
        def fill(cx, cy, nx, ny, k=k):
            if (cx, cy) in order[:k]:
                v = vals[order.index((cx, cy))]
                return (cx * 16 + 3, cy * 16 + 4, 100, v[0], v[1], ik.ST_KEPT)
            return (cx * 16 + 3, cy * 16 + 4, 100, 9999, -9999, ik.ST_FLAT)     # a value that must not be read
        out.append((f"k{k}", 80, 80, 16, _table(80, 80, 16, fill)))

    # a ragged lattice, 97 x 65 at cell 8 (13 x 9 slots): every slot kept, negative and odd values: corners see 3, edges 4, the inside 5
    def ragged(cx, cy, nx, ny):
        return (cx * 8 + 1, cy * 8 + 2, 50, _hash(cx, cy, 1) - 32768 | 1, 2 * (_hash(cx, cy, 2) - 32768) - 1, ik.ST_KEPT)
    out.append(("ragged", 97, 65, 8, _table(97, 65, 8, ragged)))

    # the same lattice with every status from 0 to 5 present: only 0 counts, a status-5 and a status-4 neighbour are ignored though they carry a dq
    def mixed(cx, cy, nx, ny):
        st = _hash(cx, cy, 3) % 6
        if st == ik.ST_NONE:
            return (-1, -1, 0, 0, 0, st)
        dq = (_hash(cx, cy, 4) - 30000, 40001 - _hash(cx, cy, 5)) if st in (0, 4, 5) else (0, 0)
        return (cx * 8 + 1, cy * 8 + 2, 50, dq[0], dq[1], st)
    out.append(("mixed", 97, 65, 8, _table(97, 65, 8, mixed)))

    # int32 extremes among the candidates, at cell 32 on one row of slots
    def extreme(cx, cy, nx, ny):
        v = (2147483647, -2147483648, 0, -1, 2147483647)[cx % 5]
        return (cx * 32, 0, 1, v, -v if v != -2147483648 else v, ik.ST_KEPT)
    out.append(("extreme", 150, 20, 32, _table(150, 20, 32, extreme)))
    return out
