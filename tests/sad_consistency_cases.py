"""Cases for hip_sad's forward-backward consistency check (include/ofps_hip.h N1c: ofps_hip_sad_consistency[_dev],
ofps_hip_set_sad_consistency, the checked ofps_hip_sad_flow / ofps_hip_sad_flow_checked_dev and the checked fused per-frame path).
CPU only: numpy and the CPU oracle -- never the library under test.

The restatement: F = oracle.sad_flow(prev, cur), G = oracle.sad_flow(cur, prev) -> partner block by array indexing -> residual ->
residual < limit -> filter, in raster order.  tests/test_sad_consistency_cpu.py pins that these inputs can tell the check from its
absence; tests/test_sad_consistency_gpu.py runs them.  The inputs are the contrast gate's (tests/sad_gate_cases.py)."""
from functools import lru_cache

import numpy as np

import oracle
import sad_gate_cases as gc
from sad_gate_cases import flat_frame, frames, half_flat_pair, two_block_frame  # noqa: F401  (the inputs, re-exported)

LIMIT = 1                                                # an exact round trip: the planted cases' limit
LIMIT_MAX = 129
KEEP_ALL = 2 * gc.RANGE + 1                              # residuals lie in [0, 2 * range]: this limit keeps every block

# ---- the exact kept counts of the restatement at LIMIT (tests/test_sad_consistency_cpu.py asserts them of the oracle alone)
FRAMES_KEPT = {1: 118, 2: 114, 3: 116}                   # frames() pair (k - 1, k), 240 blocks
FRAMES_KEPT_WITH_GATE = {1: 111, 2: 110, 3: 110}         # ... ANDed with the contrast gate at gc.GATE (which alone keeps 156)
HALF_FLAT_KEPT = {8: 78, 16: 16}                         # half_flat_pair() at range 8: of 96 and of 24 blocks
HALF_FLAT_KEPT_WITH_GATE = {8: 38, 16: 8}                # ... with the contrast gate at 1 (alone: 56 and 16)
TEXTURE_COLUMNS = gc.SPLIT // gc.BLOCK                   # block columns 0..11 of frames() are texture (144 blocks), 12..19 noise (96)


# ---- the restatement
def partner(best, W, H, B):
    """-> int [nblk]: the raster index k' of the block of the OTHER frame that holds the centre of block k's match"""
    best = np.asarray(best, np.int64)
    nbx, nby = W // B, H // B
    k = np.arange(nbx * nby)
    cx = (k % nbx) * B + B // 2 + best[:, 0]
    cy = (k // nbx) * B + B // 2 + best[:, 1]
    assert (cx >= 0).all() and (cy >= 0).all(), "a matched block lies inside the frame"
    return np.minimum(cy // B, nby - 1) * nbx + np.minimum(cx // B, nbx - 1)


def residual(F, G, W, H, B):
    """-> uint32 [nblk]: max(|dx + ex|, |dy + ey|), (ex, ey) = G[partner]"""
    F = np.asarray(F, np.int64); G = np.asarray(G, np.int64)
    kp = partner(F, W, H, B)
    return np.maximum(np.abs(F[:, 0] + G[kp, 0]), np.abs(F[:, 1] + G[kp, 1])).astype(np.uint32)


def residual_loops(F, G, W, H, B):
    """the same residual written as a loop over blocks (the check of the indexing)"""
    nbx, nby = W // B, H // B
    out = np.zeros(nbx * nby, np.uint32)
    for by in range(nby):
        for bx in range(nbx):
            k = by * nbx + bx
            dx, dy = int(F[k][0]), int(F[k][1])
            px = min((bx * B + B // 2 + dx) // B, nbx - 1)
            py = min((by * B + B // 2 + dy) // B, nby - 1)
            ex, ey = int(G[py * nbx + px][0]), int(G[py * nbx + px][1])
            out[k] = max(abs(dx + ex), abs(dy + ey))
    return out


def keep_flags(F, G, W, H, B, limit):
    """-> bool [nblk] in raster order"""
    return residual(F, G, W, H, B) < limit


check_filter = gc.gate_filter                            # the kept rows of a per-block array, in raster order


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=16)
def pair_vectors(name, block, search_range=gc.PAIR_RANGE):
    """a named pair's oracle output -> (prev, cur, records [nblk, 4], F [nblk, 3], G [nblk, 3]) read-only"""
    prev, cur = PAIRS[name]()
    ent, F = oracle.sad_flow(prev, cur, block, search_range)
    _, G = oracle.sad_flow(cur, prev, block, search_range)
    return prev, cur, _ro(ent, np.float32), _ro(F, np.int32), _ro(G, np.int32)


def _generic_pair():
    """block 12 on 100 x 60: neither strip kernel's geometry -- the generic search kernel; a ragged margin of 4 x 0 px"""
    rng = np.random.default_rng(12)
    big = rng.integers(0, 256, (60 + 8, 100 + 8), dtype=np.uint8)
    k = np.ones(3, np.float32) / 3
    sm = big.astype(np.float32)
    for axis in (0, 1):
        sm = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, sm)
    sm = sm.astype(np.uint8)
    return sm[4:64, 4:104].copy(), sm[2:62, 5:105].copy()


def _pruned_pair():
    """128 x 64 at block 16, range 16 (the pruned mode's one geometry): smooth texture moved by (5, -3)"""
    from ofps_amd import synth
    c = synth.random_luma(1, 128 + 32, 64 + 32, seed=9)[0].astype(np.float32)
    k = np.ones(5, np.float32) / 5
    for axis in (0, 1):
        c = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, c)
    c = ((c - c.min()) / (c.max() - c.min()) * 255).astype(np.uint8)
    return c[16:80, 16:144].copy(), c[19:83, 11:139].copy()


PAIRS = {"half_flat": half_flat_pair, "generic": _generic_pair, "pruned": _pruned_pair,
         "frames1": lambda: (frames()[0], frames()[1]), "frames2": lambda: (frames()[1], frames()[2]), "frames3": lambda: (frames()[2], frames()[3])}
GENERIC_BLOCK, GENERIC_RANGE = 12, 8
PRUNED_BLOCK, PRUNED_RANGE = 16, 16


@lru_cache(maxsize=8)
def frame_backward(k):
    """the oracle's winners of pair (k, k - 1) of frames(): the backward search of frame k -> [240, 3] read-only"""
    f = frames()
    return _ro(oracle.sad_flow(f[k], f[k - 1], gc.BLOCK, gc.RANGE)[1], np.int32)


@lru_cache(maxsize=32)
def frame_keep(k, limit=LIMIT, gate=0):
    """keep flags of frame k of frames() with the check at `limit` [and the contrast gate at `gate`] -> bool [240] read-only"""
    keep = keep_flags(gc.frame_vectors(k)[1], frame_backward(k), gc.FRAME_W, gc.FRAME_H, gc.BLOCK, limit)
    if gate:
        keep = keep & gc.frame_keep(k, gate)
    keep.setflags(write=False)
    return keep


# ---- synthetic winner arrays for the kernel alone (no search): every vector keeps its matched block inside the frame, as a search's does
def synthetic_winners(nbx, nby, B, W=None, H=None, seed=0, max_d=64):
    """-> (W, H, F [nblk, 3], G [nblk, 3]) int32.  F: random in-frame vectors; the first blocks of the lattice get the extreme vector
    towards each frame edge and corner (for the last block column / row of a ragged frame that centre lies in the margin and is clamped).
    G: the inverse at the partner, exact or off by one or two, for four blocks of five, random for the rest -- residuals of 0, 1, 2 and
    anything up to 2 * max_d all occur where the lattice is large enough (tests/test_sad_consistency_cpu.py asserts which)."""
    W = nbx * B if W is None else W
    H = nby * B if H is None else H
    assert W // B == nbx and H // B == nby
    rng = np.random.default_rng(1000 * nbx + 10 * nby + B + seed)
    n = nbx * nby
    k = np.arange(n)
    x0, y0 = (k % nbx) * B, (k // nbx) * B
    lo_x, hi_x = np.maximum(-x0, -max_d), np.minimum(W - B - x0, max_d)
    lo_y, hi_y = np.maximum(-y0, -max_d), np.minimum(H - B - y0, max_d)
    F = np.zeros((n, 3), np.int32)
    F[:, 0] = rng.integers(lo_x, hi_x + 1)
    F[:, 1] = rng.integers(lo_y, hi_y + 1)
    F[:, 2] = rng.integers(0, 255 * B * B + 1, n)
    zero = np.zeros(n, np.int64)
    corners = [(lo_x, lo_y), (hi_x, lo_y), (lo_x, hi_y), (hi_x, hi_y), (lo_x, zero), (hi_x, zero), (zero, lo_y), (zero, hi_y)]
    for j in range(0, n, 3):                             # every third block points at a frame edge or corner, as far as it may
        ex, ey = corners[(j // 3 + seed) % 8]
        F[j, 0], F[j, 1] = ex[j], ey[j]
    G = np.zeros((n, 3), np.int32)
    G[:, 0] = rng.integers(-max_d, max_d + 1, n)
    G[:, 1] = rng.integers(-max_d, max_d + 1, n)
    G[:, 2] = rng.integers(0, 255 * B * B + 1, n)
    kp = partner(F, W, H, B)
    off = ((0, 0), (1, 0), (0, -1), (-1, 1), (2, 0), (0, 2), (-2, 1), (-1, -2))
    for j in rng.permutation(n):                         # later writers of a shared partner win: the earlier ones keep whatever residual results
        if j % 5 < 4:                                    # residual 0, 1, 1, 1, 2, 2, 2, 2 by j % 8; every fifth block stays random
            G[kp[j], :2] = -F[j, :2] + off[j % 8]
    far = np.flatnonzero((hi_x >= max_d) & (np.bincount(kp, minlength=n)[kp] == 1))
    if len(far):                                         # the largest residual of the domain, 2 * max_d: the limit 129 case's "limit - 1"
        j = far[0]
        F[j, :2] = (max_d, 0)
        kp = partner(F, W, H, B)
        G[kp[j], :2] = (max_d, 0)
    G[:, :2] = np.clip(G[:, :2], -max_d, max_d)          # the standalone form's domain: |d| <= 64 (beyond it the flag is unspecified)
    return W, H, F, G


def ragged_winners():
    """RAGGED by hand: both blocks' matches have their centre at x = 32, y = 16 -- in the margin right of and below the lattice, where
    cx / B = 2 = nbx and cy / B = 1 = nby: the partner is block (1, 0) only through the clamp -> residuals (16, 0)"""
    W, H, B = RAGGED
    F = np.array([[24, 8, 7], [8, 8, 9]], np.int32)
    G = np.array([[5, 5, 1], [-8, -8, 2]], np.int32)
    return W, H, B, F, G, np.array([16, 0], np.uint32)


KERNEL_LATTICES = ((1, 1), (3, 2), (20, 12), (64, 1), (65, 1), (257, 3))        # one lane .. one wave, one wave + 1, 4 workgroups (771 blocks)
KERNEL_BLOCKS = (8, 16)
RAGGED = (40, 24, 16)                                    # W, H, block: 2 x 1 blocks, 8 px of margin right and below: a centre there is clamped
