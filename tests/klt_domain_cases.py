"""Case lists and seeded frame makers for hip_klt's domain sweep (include/ofps_hip.h N3 and its extensions N3m, N3f, N3p, N3pb, N3b, N3i), shared
by tests/test_klt_domain_cpu.py and tests/test_klt_domain_gpu.py.  Data and pure functions of their arguments only: nothing here calls the
library or a restatement.  A frame is named by a tuple (kind, ...) that pair() turns into (prev, cur); a flow case is a Flow tuple of every
setting the decoder reads."""
import collections
import functools

import numpy as np

import klt_cases as kc
import klt_intra_cases as xc
from ofps_amd import synth

WS = (1, 2, 3, 4, 5, 6, 7)
CELLS = (8, 16, 32)
RADII = (1, 2, 3)
CR_PAIRS = tuple((C, r) for C in CELLS for r in RADII)


# ------------------------------------------------------------------------------------------------ frames
def binary_image(W, H, seed=46):
    """a seeded 0/255 image of 4 x 4 blocks"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 2, (-(-H // 4), -(-W // 4)), dtype=np.uint8) * np.uint8(255)
    return np.ascontiguousarray(np.kron(blocks, np.ones((4, 4), np.uint8))[:H, :W])


def ties_image(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return (((x // 2 + y // 2) % 2) * 200 + 20).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pair(spec):
    """(kind, ...) -> (prev, cur), read-only"""
    kind = spec[0]
    if kind == "warp":                                        # klt_cases.WARP: roll 0.5 degrees, zoom 1.004
        out = kc.warp_pair(spec[1], spec[2], spec[3])
    elif kind == "unrot":                                     # a pure shift
        out = synth.camera_warp_pair(spec[1], spec[2], shift=spec[3], seed=11, roll_deg=0, zoom=1)
    elif kind == "binary":
        a = binary_image(spec[1], spec[2])
        out = a, np.roll(a, (1, 2), (0, 1))
    elif kind == "ties":
        a = ties_image(spec[1], spec[2])
        out = a, np.roll(a, (1, 2), (0, 1))
    elif kind == "flat":
        out = kc.flat_pair(spec[1], spec[2])
    elif kind == "relit":                                     # klt_zm_cases.relit: cur raised by spec[2] and clipped
        a, b = pair(spec[1])
        out = a, np.clip(b.astype(np.int64) + spec[2], 0, 255).astype(np.uint8)
    elif kind == "repaint":
        out = xc.repaint_pair()
    elif kind == "cut":
        out = xc.cut_pair()
    else:
        raise ValueError(spec)
    out = tuple(np.ascontiguousarray(a) for a in out)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sequence(spec):
    """(kind, W, H, n) -> uint8 [n, H, W]: n frames of one scene that moves a little further each frame"""
    kind, W, H, n = spec
    if kind == "warpseq":
        fr = [kc.warp_pair(W, H, (0.0, 0.0))[0]] + [kc.warp_pair(W, H, (0.9 * k, -0.7 * k))[1] for k in range(1, n)]
    elif kind == "binaryseq":
        a = binary_image(W, H)
        fr = [np.roll(a, (k, 2 * k), (0, 1)) for k in range(n)]
    else:
        raise ValueError(spec)
    out = np.stack(fr)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ flow cases
# zm: mean removal (N3m); F: forward-backward limit (N3f); q, P: intra ratio and cut percent (N3i); pad: bytes of poisoned row padding
Flow = collections.namedtuple("Flow", "id frame cell r min_score min_eig R L w K zm F q P pad",
                              defaults=(8, 1, 1, 1, 0, 2, 4, 10, False, 0, 0, 0, 0))


def flow(id, frame, **kw):
    return Flow(id, frame, **kw)


WARP131 = ("warp", 131, 67, (2.3, -1.6))
BINARY64 = ("binary", 64, 48)
GRID_FRAMES = (("warp131", WARP131), ("binary64", BINARY64))


def _grid(prefix, Ls, **kw):
    return [flow(f"{prefix}-{fn}-w{w}-L{L}", fs, L=L, w=w, **kw) for fn, fs in GRID_FRAMES for w in WS for L in Ls]


# B.1: every w x L in {1, 2, 3} on the two frames
B1 = _grid("n3", (1, 2, 3))

# B.2: L = 4, 5, 6 at the smallest legal frame of each depth, and the odd frames
DEEP = [
    flow("deep-L4-64", ("warp", 64, 64, (3.1, -2.2)), L=4, w=3),
    flow("deep-L5-128", ("warp", 128, 128, (6.2, -4.3)), L=5, w=5),
    flow("deep-L6-256", ("warp", 256, 256, (9.3, -7.1)), cell=32, r=2, L=6, w=7, K=30),
    flow("deep-257x259", ("warp", 257, 259, (7.4, -5.2)), cell=16, r=1, L=6, w=5),
    flow("deep-511x263", ("warp", 511, 263, (6.3, -4.6)), cell=32, r=2, L=6, w=6),
    flow("deep-128x131", ("warp", 128, 131, (4.2, -3.3)), cell=8, r=3, L=5, w=2),
]
TOO_SMALL = [(4, 63, 64), (4, 64, 63), (5, 127, 128), (5, 128, 127), (6, 255, 256), (6, 256, 255)]      # (L, W, H): refused

# B.3: K at its ends
K_ENDS = [flow("K1", WARP131, L=2, w=2, K=1), flow("K29", WARP131, L=2, w=2, K=29), flow("K30", WARP131, L=2, w=2, K=30)]
K_PIN = 2                                                     # slots in which K = 29 and K = 30 differ: the 30th iteration is reached
UNROT = ("unrot", 96, 64, (5, -4))
CLAMP = [flow("clamp-w1", UNROT, L=1, w=1, K=1), flow("clamp-w2", UNROT, L=1, w=2, K=1)]
CLAMP_PIN = {"clamp-w1": (96, 60), "clamp-w2": (96, 5)}       # (kept, kept slots with a component at +-256 w): the issue's numbers

# B.4: settings at their ends; EIG_MIXED and RESIDUAL_EXACT hold values read off the restatement, which tests/test_klt_domain_cpu.py pins
ENDS = [
    flow("eig1", BINARY64, L=1, w=7, min_eig=1),
    flow("eig65535", BINARY64, L=1, w=7, min_eig=65535),
    flow("R1", BINARY64, L=1, w=7, R=1),
    flow("R4080", BINARY64, L=1, w=7, R=4080),
    flow("eig65535-warp", WARP131, L=2, w=4, min_eig=65535),
]
EIG_MIXED = [flow("eig64-warp", WARP131, L=2, w=4, min_eig=64), flow("eig4096-binary", BINARY64, L=2, w=4, min_eig=4096)]
# (case, slot, R): the restatement's residual of that slot is 16 R n^2 exactly -- kept at R, status 4 at R - 1
RESIDUAL_EXACT = (flow("res-exact", WARP131, L=2, w=2), 126, 52)

# B.6: padded rows at L = 6
PADDED = [flow("pad13-L6", ("warp", 257, 259, (7.4, -5.2)), cell=16, r=1, L=6, w=5, pad=13)]

# C: the other compiled kernels
C_ZM = _grid("zm", (1, 3), zm=True) + [
    flow("zm-L6-256", ("warp", 256, 256, (9.3, -7.1)), cell=32, r=2, L=6, w=7, zm=True),
    flow("zm-binary-w7-R", BINARY64, L=2, w=7, R=64, zm=True),
    flow("zm-binary-w7-R1", BINARY64, L=1, w=7, R=1, zm=True),
    flow("zm-relit-w2", ("relit", WARP131, 20), L=2, w=2, zm=True),
    flow("zm-relit-w6", ("relit", WARP131, 20), L=2, w=6, zm=True),
]
C_FB = ([c for F in (16, 1, 4096) for zm in (False, True) for c in _grid(f"fb{F}{'zm' if zm else ''}", (1, 3), F=F, zm=zm)]
        + [flow("fb16-L6-256", ("warp", 256, 256, (9.3, -7.1)), cell=32, r=2, L=6, w=7, F=16),
           flow("fb16zm-L6-256", ("warp", 256, 256, (9.3, -7.1)), cell=32, r=2, L=6, w=5, F=16, zm=True)])
FB16_SWEEP = [c for c in C_FB if c.id.startswith("fb16-") and "L6" not in c.id]
C_INTRA = [flow(f"intra-{fn}-w{w}-P{P}", (fn,), cell=16, r=2, L=2, w=w, K=10, q=xc.Q, P=P) for fn in ("repaint", "cut") for w in (2, 7) for P in (0, 50)]

FLOW_CASES = B1 + DEEP + K_ENDS + CLAMP + ENDS + EIG_MIXED + PADDED + C_ZM + C_FB + C_INTRA
# the cases whose point is that everything, or nothing, is kept: exempt from 0 < kept < slots
# (F = 1 asks a track to return to the very 1/256 pixel: at w = 1 under mean removal none does)
ALL_OR_NOTHING = frozenset({"clamp-w1", "clamp-w2", "eig65535", "eig65535-warp", "intra-cut-w2-P50", "intra-cut-w7-P0", "intra-cut-w7-P50",
                            "fb1zm-warp131-w1-L1", "fb1zm-binary64-w1-L1"})
# one case per status that the w x L sweep does not reach: 1 (and geometry in A), 2, 4, 6, 7
STATUS_WITNESSES = ("n3-binary64-w1-L1", "eig65535", "R1", "intra-cut-w2-P0", "intra-cut-w2-P50")
assert len({c.id for c in FLOW_CASES}) == len(FLOW_CASES)

# ------------------------------------------------------------------------------------------------ A: features
# (id, frame, cell, r, min_score, bytes of poisoned row padding); the frame's prev alone is read
Feat = collections.namedtuple("Feat", "id frame cell r min_score pad", defaults=(1, 0))


def _feature_cases():
    out = []
    for C, r in CR_PAIRS:
        for kind in ("warp", "binary", "ties"):
            for W, H in ((64, 48), (67, 35), (131, 67)):
                spec = (kind, W, H, (1.3, -0.6)) if kind == "warp" else (kind, W, H)
                out.append(Feat(f"feat-{kind}-{W}x{H}-C{C}-r{r}", spec, C, r))
        k = 1 if C == 32 else 2
        for j in (1, r + 1, r + 2):                           # the last cell: no admissible pixel, none, exactly one column / row
            out.append(Feat(f"geom-C{C}-r{r}-j{j}", ("binary", k * C + j, C + j), C, r))
        for W, H in ((8, 8), (9, 8), (8, 9)) + (((33, 9),) if C == 32 else ()):
            out.append(Feat(f"tiny-{W}x{H}-C{C}-r{r}", ("binary", W, H), C, r))
    for pad in (1, 13):
        out.append(Feat(f"feat-pad{pad}", ("warp", 67, 35, (1.3, -0.6)), 8, 3, 1, pad))
        out.append(Feat(f"feat-pad{pad}-C32", ("binary", 67, 35), 32, 1, 1, pad))
    for ms in (1, 2 ** 31 - 1):
        out.append(Feat(f"feat-minscore{ms}", ("binary", 64, 48), 16, 2, ms))
    return out


FEATURE_CASES = _feature_cases()
GEOMETRY_CASES = [c for c in FEATURE_CASES if c.id.startswith("geom-")]
TINY_CASES = [c for c in FEATURE_CASES if c.id.startswith("tiny-")]
MINSCORE_AT = Feat("feat-minscore-exact", ("warp", 131, 67, (1.3, -0.6)), 16, 2)      # min_score from the restatement's own list

# A.5 and C's batch forms: (id, sequence, ref_mode, chained, the settings that differ from Flow's defaults, what else the case is about)
Batch = collections.namedtuple("Batch", "id seq ref_mode chained kw extra", defaults=(0, False, None, ""))
BATCH_SCORE = [Batch(f"bscore-C{C}-r{r}-m{m}", ("binaryseq" if C == 16 else "warpseq", 131, 67, 3), m, False, dict(cell=C, r=r, L=2, w=3, K=10))
               for C, r in ((8, 3), (16, 1), (32, 2)) for m in (0, 1)]
BATCH4 = ("warpseq", 128, 131, 4)
BATCH_TRACK = [Batch(f"batch-w{w}-L{L}-m{m}-{'chain' if ch else 'plain'}", BATCH4, m, ch, dict(cell=16, r=2, L=L, w=w, K=10))
               for (w, L) in ((2, 1), (3, 5), (5, 1), (6, 5)) for m in (0, 1) for ch in (False, True)]
BATCH_EXTRA = [
    Batch("batch-zm-fb", BATCH4, 0, True, dict(cell=16, r=2, L=5, w=5, K=10, zm=True, F=16)),
    Batch("batch-noslots", BATCH4, 0, False, dict(cell=16, r=2, L=5, w=3, K=10), "noslots"),
    Batch("batch-pitch", BATCH4, 1, True, dict(cell=16, r=2, L=5, w=6, K=10), "pitch"),
]
BATCH_CASES = BATCH_SCORE + BATCH_TRACK + BATCH_EXTRA

# C, N3p chained over three frames
CHAIN_CASES = [Batch("chain-w3-L5", ("warpseq", 128, 131, 3), 0, True, dict(cell=8, r=3, L=5, w=3, K=10)),
               Batch("chain-w6-L5-fb", ("warpseq", 128, 131, 3), 0, True, dict(cell=8, r=3, L=5, w=6, K=10, F=16))]

# B.5 and C's N3p stage forms: the 256 x 256 frame, its corners, edge midpoints and centre
POINT_FRAME = ("warp", 256, 256, (3.3, -2.1))
POINT_LS = (1, 6)


def frame_points(W, H):
    """the four corners, the four edge midpoints and the centre; behind them a ring 3 pixels inside the frame and a few interior points, whose
    windows reach over the border while their tracks stay inside"""
    edge = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W // 2, 0], [W // 2, H - 1], [0, H // 2], [W - 1, H // 2], [W // 2, H // 2]]
    ring = [[3, 3], [W - 4, 3], [3, H - 4], [W - 4, H - 4], [W // 3, 3], [W // 3, H - 4], [3, H // 3], [W - 4, H // 3]]
    inner = [[W // 4, H // 4], [3 * W // 4, H // 4], [W // 4, 3 * H // 4], [3 * W // 4, 3 * H // 4], [W // 2 + 9, H // 2 - 17]]
    return np.array(edge + ring + inner, np.int32)


def q_positions(W, H):
    """_track_q: P = 0, 255, 256 (W - 1) - 1 and 256 (W - 1) in x against the same ends in y; behind them frame_points' ring and interior at
    fractional positions"""
    xs = (0, 255, 256 * (W - 1) - 1, 256 * (W - 1))
    ys = (0, 255, 256 * (H - 1) - 1, 256 * (H - 1))
    inner = 256 * frame_points(W, H)[8:] + np.array([[77, -130]])
    return np.concatenate([np.array([[x, y] for x in xs for y in ys], np.int32), inner]).astype(np.int32)


def q_outside(W, H):
    return np.array([[-1, 0], [256 * (W - 1) + 1, 0], [0, -1], [0, 256 * (H - 1) + 1]], np.int32)


def px_outside(W, H):
    return np.array([[-1, 0], [W, 0], [0, -1], [0, H]], np.int32)


# the issue's list, and six that lie near the motion or well off it, so that a pass of few iterations ends elsewhere than from zero
GUESSES = (0, 1, -1, 255, -255, 1 << 23, -(1 << 23), 845, -538, 2560, -2560, 15360, -15360)
GUESS_ITERS = 2
GUESS_BEYOND = (1 << 23) + 1


def guess_list(n):
    """n guesses (gx, gy) that walk GUESSES in both components, out of step"""
    g = GUESSES
    return np.array([[g[k % len(g)], g[(3 * k + 1) % len(g)]] for k in range(n)], np.int32)


# C, N3i's activity: the frames and the points (corners first)
ACTIVITY_FRAMES = (("binary", 64, 48), ("ties", 64, 48), ("flat", 64, 48))


def activity_points(W, H):
    return np.concatenate([frame_points(W, H), [[5, 7], [W - 3, 2], [17, H - 2]]]).astype(np.int32)


# the fused case
FUSED = flow("fused-L5-w3", ("warp", 128, 131, (4.2, -3.3)), cell=8, r=3, L=5, w=3)

# ------------------------------------------------------------------------------------------------ D: both sides of every bound
# (setter, refused keyword values, accepted neighbours)
SET_KLT_BOUNDS = [("cell", (4, 64), (8, 32)), ("score_radius", (0, 4), (1, 3)), ("min_score", (0,), (1,)), ("min_eig", (0, 65536), (1, 65535)),
                  ("max_residual", (-1, 4081), (0, 4080))]
CALL_BOUNDS = [("L", (0, 7), (1, 6)), ("w", (0, 8), (1, 7)), ("K", (0, 31), (1, 30))]
FB_BOUNDS = ((-1, 4097), (0, 4096))
BOUND_FRAME = ("warp", 256, 256, (3.3, -2.1))                 # deep enough for L = 6
