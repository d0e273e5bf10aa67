"""Cases for hip_sad's search levels (include/ofps_hip.h N1h: ofps_hip_set_sad_levels, ofps_hip_sad_down2[_dev], ofps_hip_sad_refine[_dev] and
every search entry point at levels > 1).  CPU only: numpy, the restatement tests/indep_sad_hier.py and the CPU oracle -- never the library
under test.  tests/test_sad_hier_cpu.py pins that the planted cases hold of the restatement alone; tests/test_sad_hier_gpu.py runs them."""
from functools import lru_cache

import numpy as np

import indep_sad_hier as ih

# ---- the planted shift: (W, H, block, range, levels, (dx, dy), reachable blocks, lattice blocks).  |d| is beyond the plain search's range in
# every case; in the 200 x 136 case the lattice column 24 has no parent of its own (the parent lattice has 12 columns): the parent clamp.
PLANTED = ((192, 128, 16, 8, 2, (15, -11), 60, 96),
           (192, 128, 16, 8, 2, (-17, 13), 60, 96),
           (200, 136, 8, 8, 2, (14, -17), 264, 425),
           (320, 192, 16, 8, 3, (33, -26), 128, 240),
           (320, 192, 16, 8, 3, (-37, 30), 128, 240))
MARGIN = 40                                              # of the canvas around the frame: above every |d| planted


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=4)
def canvas(W, H, seed=2024):
    """smooth texture, uint8 [H + 2 * MARGIN, W + 2 * MARGIN]: value noise with octaves of 16, 4 and 1 px weighted 4 : 2 : 1, 5 x 5 box
    smoothed, scaled to 16..235.  Written with explicit sums in a fixed order: the same bytes everywhere."""
    rng = np.random.default_rng(seed)
    CH, CW = H + 2 * MARGIN, W + 2 * MARGIN
    acc = np.zeros((CH, CW), np.float64)
    for cell, weight in ((16, 4.0), (4, 2.0), (1, 1.0)):
        gh, gw = CH // cell + 2, CW // cell + 2
        g = rng.integers(0, 256, (gh, gw)).astype(np.float64)
        y = np.arange(CH) / cell; x = np.arange(CW) / cell
        yi = y.astype(np.int64); xi = x.astype(np.int64)
        fy = (y - yi)[:, None]; fx = (x - xi)[None, :]
        a = g[yi][:, xi]; b = g[yi][:, xi + 1]; c = g[yi + 1][:, xi]; d = g[yi + 1][:, xi + 1]
        acc = acc + weight * ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy)
    pad = np.pad(acc, 2, mode="edge")
    box = np.zeros_like(acc)
    for oy in range(5):
        for ox in range(5):
            box = box + pad[oy:oy + CH, ox:ox + CW]
    lo, hi = box.min(), box.max()
    return _ro(np.floor(16.0 + (box - lo) * (219.0 / (hi - lo)) + 0.5), np.uint8)


@lru_cache(maxsize=16)
def planted_pair(W, H, d, seed=2024):
    """prev = the canvas cut at the margin; cur[y, x] = prev[y + dy, x + dx] + uniform noise in {-1, 0, 1} -> (prev, cur) read-only"""
    c = canvas(W, H, seed)
    dx, dy = d
    prev = c[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    cur = c[MARGIN + dy:MARGIN + dy + H, MARGIN + dx:MARGIN + dx + W].astype(np.int64)
    cur = cur + np.random.default_rng(seed + 1000 * (dx + 64) + (dy + 64)).integers(-1, 2, cur.shape)
    assert cur.min() >= 0 and cur.max() <= 255
    return _ro(prev, np.uint8), _ro(cur, np.uint8)


def reachable(W, H, B, levels, d):
    """-> bool [nblk] in raster order: the block's top-level ancestor exists in the top lattice, and that ancestor's block moved by d,
    widened by 2^(levels - 1) px each way, lies inside the frame"""
    s = 1 << (levels - 1)
    nbx, nby = W // B, H // B
    tnbx, tnby = (W >> (levels - 1)) // B, (H >> (levels - 1)) // B
    dx, dy = d
    out = np.zeros((nby, nbx), bool)
    for by in range(nby):
        for bx in range(nbx):
            ax, ay = bx >> (levels - 1), by >> (levels - 1)
            if ax >= tnbx or ay >= tnby:
                continue
            x_lo, x_hi = ax * B * s + dx - s, (ax + 1) * B * s + dx + s
            y_lo, y_hi = ay * B * s + dy - s, (ay + 1) * B * s + dy + s
            out[by, bx] = x_lo >= 0 and x_hi <= W and y_lo >= 0 and y_hi <= H
    return out.reshape(-1)


@lru_cache(maxsize=8)
def planted_expect(i):
    """case i of PLANTED through the restatement -> (prev, cur, entries, best, per-level winners), read-only"""
    W, H, B, R, L, d, _, _ = PLANTED[i]
    prev, cur = planted_pair(W, H, d)
    ent, best, per_level = ih.search(prev, cur, B, R, L)
    return prev, cur, _ro(ent, np.float32), _ro(best, np.int32), tuple(_ro(b, np.int32) for b in per_level)


# ---- ofps_hip_sad_down2: (W, H, stride)
DOWN2_SIZES = ((2, 2, 2), (5, 3, 5), (37, 23, 40), (64, 48, 64), (200, 136, 200))


def down2_frame(W, H, stride):
    """-> uint8 [H, stride] random bytes (the margin too: the kernel may not read it into the result); the first quad columns hold the
    rounding cases (1,2,2,2), (0,0,0,1), (0,0,1,1), (255,255,255,254) where the frame is wide enough"""
    f = np.random.default_rng(100 * W + H).integers(0, 256, (H, stride), dtype=np.uint8)
    quads = ((1, 2, 2, 2), (0, 0, 0, 1), (0, 0, 1, 1), (255, 255, 255, 254))
    for j, q in enumerate(quads):
        if 2 * j + 1 < W:
            f[0, 2 * j], f[0, 2 * j + 1], f[1, 2 * j], f[1, 2 * j + 1] = q
    return f


# ---- ofps_hip_sad_refine on synthetic parents, no search: (W, H, block)
REFINE_FRAMES = ((64, 48, 16), (40, 24, 8), (50, 38, 12), (200, 136, 8))
PARENT_KINDS = ("zero", "alternating") + tuple(f"edge{j}" for j in range(8))


def parent_lattice(W, H, B):
    """the lattice of the level above: (nbx, nby) of the halved frame (at least 1 x 1: the standalone call takes any parent lattice)"""
    return max((W >> 1) // B, 1), max((H >> 1) // B, 1)


def refine_pair(W, H, seed=0):
    """two frames of smooth texture a few pixels apart, + noise -> (prev, cur)"""
    c = canvas(W, H, 77 + seed)
    prev = c[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    cur = c[MARGIN - 2:MARGIN - 2 + H, MARGIN + 3:MARGIN + 3 + W].astype(np.int64)
    cur = cur + np.random.default_rng(5 + seed).integers(-1, 2, cur.shape)
    return _ro(prev, np.uint8), _ro(cur, np.uint8)


def parents(kind, pnbx, pnby):
    """-> int32 [pnby, pnbx, 3].  zero; edge0..edge7: every parent +-63 towards one frame edge or corner (the predictor +-126 leaves every
    frame here: the clamp); alternating: (5, -4) and (-6, 7) on a checkerboard, with junk in the sad field, which nobody reads"""
    p = np.zeros((pnby, pnbx, 3), np.int32)
    if kind.startswith("edge"):
        dirs = ((-63, 0), (63, 0), (0, -63), (0, 63), (-63, -63), (63, -63), (-63, 63), (63, 63))
        p[:, :, :2] = dirs[int(kind[4:])]
    elif kind == "alternating":
        for j in range(pnbx * pnby):
            y, x = j // pnbx, j % pnbx
            p[y, x] = (5, -4, 123456) if (x + y) % 2 == 0 else (-6, 7, -1)
    else:
        assert kind == "zero"
    return p
