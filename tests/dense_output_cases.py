"""Case builders for the dense decoders' output stage (ofps_amd/csrc/mask.hip, dense_decoder.hip): frames whose contrast mask has a known
shape, and the expected mask of impulse frames written out from the definitions.  CPU only: numpy, the synthetic clips and the CPU oracle --
never the library under test.  tests/test_dense_output_cases_cpu.py checks that every case has the property it is named for (so that no GPU
test passes vacuously); tests/test_dense_output_stage_gpu.py runs them.

The mask (cv-decoder/src/lib.rs:203-237): Sobel(dx=1, dy=1, ksize 5) -> `> 20` -> dilate(MORPH_ELLIPSE 11 x 11)."""
from functools import lru_cache

import numpy as np

import oracle
from ofps_amd import synth

BG = 128                          # background of the impulse frames: +-21 stays inside u8

# ---- one impulse: literals ----------------------------------------------------------------------------------------------------------------
# Sobel(1, 1, 5) correlates with k (x) k, k = [-1, -2, 0, 2, 1]: an impulse of amplitude a at p answers at p + (dy, dx) with
# a * k[2 - dy] * k[2 - dx].  The eight taps where that product is positive for a > 0 (both offsets of one sign) ...
TAPS_POS = ((-2, -2, 1), (-2, -1, 2), (-1, -2, 2), (-1, -1, 4), (1, 1, 4), (1, 2, 2), (2, 1, 2), (2, 2, 1))          # (dy, dx, weight)
# ... and for a < 0 (offsets of opposite signs): the other two quadrants
TAPS_NEG = ((-2, 2, 1), (-2, 1, 2), (-1, 2, 2), (-1, 1, 4), (1, -1, 4), (1, -2, 2), (2, -1, 2), (2, -2, 1))
THRESHOLD = 20                    # a tap passes when weight * |a| > 20
ELLIPSE_HALF = (0, 3, 4, 5, 5, 5, 5, 5, 4, 3, 0)      # row half-widths of the 11 x 11 ellipse, dy = -5 .. 5
AMPLITUDES = (5, 6, 10, 11, 20, 21)                   # 4a = 20 | 24, 2a = 20 | 22, a = 20 | 21: each weight's last failing / first passing value
SIGNED_AMPLITUDES = AMPLITUDES + tuple(-a for a in AMPLITUDES)
REFLECT_MARGIN = 3                # an impulse this far from every border is not folded into any Sobel window by BORDER_REFLECT_101


def impulse_frame(W, H, impulses, bg=BG):
    """flat frame with single pixels raised / lowered: impulses = [(y, x, amplitude), ...]"""
    g = np.full((H, W), bg, np.uint8)
    for y, x, a in impulses:
        g[y, x] = bg + a
    return g


def impulse_taps(a):
    """the (dy, dx) offsets whose Sobel response to an impulse of amplitude a passes the threshold"""
    return [(dy, dx) for dy, dx, w in (TAPS_POS if a > 0 else TAPS_NEG) if w * abs(a) > THRESHOLD]


def impulse_mask(W, H, impulses):
    """Expected mask of impulse_frame(W, H, impulses) from the literals above: the union of ellipses around the passing taps, clipped to the
    image.  Valid for impulses at least REFLECT_MARGIN from every border and at least 5 apart along one axis (their responses do not add)."""
    m = np.zeros((H, W), np.uint8)
    for n, (y, x, a) in enumerate(impulses):
        assert REFLECT_MARGIN <= y < H - REFLECT_MARGIN and REFLECT_MARGIN <= x < W - REFLECT_MARGIN, (y, x)
        for y2, x2, _ in impulses[:n]:
            assert max(abs(y - y2), abs(x - x2)) >= 5
        for dy, dx in impulse_taps(a):
            ty, tx = y + dy, x + dx                      # inside the image: REFLECT_MARGIN > 2
            for ey, hw in zip(range(-5, 6), ELLIPSE_HALF):
                yy = ty + ey
                if 0 <= yy < H:
                    m[yy, max(tx - hw, 0):min(tx + hw, W - 1) + 1] = 1
    return m


# ---- placements ---------------------------------------------------------------------------------------------------------------------------
SEAM_W, SEAM_H = 200, 56                               # mask tiles are 64 x 16: seams at x = 64, 128 and y = 16, 32
SEAM_XS = tuple(range(57, 71)) + tuple(range(121, 135))
SEAM_YS = tuple(range(9, 23)) + tuple(range(25, 39))
BORDER_W, BORDER_H = 80, 40


def border_placements(W=BORDER_W, H=BORDER_H):
    """(y, x) within 7 pixels of each border and each corner: BORDER_REFLECT_101 folds the impulse into the Sobel window there"""
    near_y = list(range(7)) + list(range(H - 7, H))
    near_x = list(range(7)) + list(range(W - 7, W))
    out = [(y, x) for y in near_y for x in near_x]                                   # the four corners
    out += [(y, W // 2) for y in near_y] + [(H // 2, x) for x in near_x]            # the four borders
    return out


# ---- mask kernel geometry -----------------------------------------------------------------------------------------------------------------
MASK_WS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15, 63, 64, 65, 73, 74, 75, 127, 128, 129, 200)
MASK_HS = (1, 2, 3, 5, 7, 8, 15, 16, 17, 25, 26, 27, 31, 32, 33)
MASK_GEOMETRIES = tuple((W, H) for i, W in enumerate(MASK_WS) for j, H in enumerate(MASK_HS) if (i + j) % 2 == 0)      # 165, every W, every H
MASK_CONTENTS = ("texture", "noise", "checker", "constant")


def mask_content(kind, W, H):
    if kind == "texture":
        return synth.flatten_regions(synth.luma_sequence(1, W, H, max_step=0, seed=W * 31 + H), region=24, seed=W + H)[0]
    if kind == "noise":
        return synth.random_luma(1, W, H, seed=W * 7 + H)[0]
    if kind == "checker":                                # 0 / 255 in 2 x 2 blocks: Sobel responses of +-4 * 255, the steepest steps u8 has
        yy, xx = np.mgrid[0:H, 0:W]                      # (1 x 1 blocks answer 0 everywhere: k sums to zero against alternating signs)
        return ((((yy >> 1) + (xx >> 1)) & 1) * 255).astype(np.uint8)
    assert kind == "constant"
    return np.full((H, W), 200, np.uint8)


# ---- compaction geometries and mask shapes ------------------------------------------------------------------------------------------------
CT = 1024                                               # records per compaction tile
SMALL_MAX = 32768                                       # kCompactSmallMax: up to here one workgroup compacts
COMPACT_GEOMETRIES = ((217, 151), (256, 128), (99, 331), (256, 132), (333, 101), (1024, 1024), (1024, 1025), (1920, 1080), (2048, 1025))
SHAPES = ("a", "b", "c", "d", "e", "f", "g")
# (d) and (e): one weight-4 impulse (amplitude 6: two taps, a 10 x 10 box of mask) in the first / the last rows and columns.  A thresholded pixel
# dilates over 11 rows, so the mask of a frame wider than 102 pixels cannot stay inside 1,024 consecutive raster records: what these shapes
# give there is survivors in the first (last) ten rows' first (last) ten columns only -- the head of the first (tail of the last) few tiles,
# every other tile empty.  At W = 99 shape (d) does stay inside the first 1,024 records.
CORNER = 3                                              # the impulse's distance from the two borders
CORNER_BOX = 10                                         # rows / columns from the corner its mask can reach: CORNER + 1 (tap) + 5 (ellipse) + 1


def shape_applies(shape, W, H):
    return shape in "abcg" or H >= 200


COMPACT_CASES = tuple((W, H, s) for W, H in COMPACT_GEOMETRIES for s in SHAPES if shape_applies(s, W, H))


def sparse_impulses(W, H):
    """shape (f): impulses 47 rows apart (>= 40), columns and amplitudes varying: whole tiles and whole waves between them are empty"""
    amps = (6, 21, -11, -6, 11, -21)
    return [(y, 10 + (37 * k * k + 11 * k) % (W - 20), amps[k % len(amps)]) for k, y in enumerate(range(20, H - 8, 47))]


@lru_cache(maxsize=4)
def _texture_pair(W, H):
    return synth.luma_sequence(2, W, H, max_step=2, seed=W + 3 * H)


@lru_cache(maxsize=16)
def compaction_pair(W, H, shape):
    """-> (prev, cur) u8 [H, W]: `cur` has mask shape `shape` under the oracle mask; `prev` is `cur` moved by a pixel (some flow to record)"""
    if shape == "a":
        cur = np.full((H, W), BG, np.uint8)
    elif shape == "b":
        cur = synth.random_luma(1, W, H, seed=W + H)[0]
    elif shape == "c":
        fr = synth.flatten_regions(_texture_pair(W, H), region=96 if W * H > 200000 else 24, seed=3)
        return fr[0], fr[1]
    elif shape == "d":
        cur = impulse_frame(W, H, [(CORNER, CORNER, 6)])
    elif shape == "e":
        cur = impulse_frame(W, H, [(H - 1 - CORNER, W - 1 - CORNER, 6)])
    elif shape == "f":
        cur = impulse_frame(W, H, sparse_impulses(W, H))
    else:
        assert shape == "g"                             # one vertical band of noise, 30 columns wide
        cur = np.full((H, W), BG, np.uint8)
        c0 = W // 3
        cur[:, c0:c0 + 30] = synth.random_luma(1, 30, H, seed=W)[0]
    return np.roll(cur, (1, 1), (0, 1)), cur


@lru_cache(maxsize=64)
def oracle_mask(W, H, shape):
    m = oracle.contrast_mask(compaction_pair(W, H, shape)[1])
    m.setflags(write=False)
    return m


def tile_counts(mask):
    """survivors per compaction tile of CT raster-order records"""
    flat = np.asarray(mask).reshape(-1).astype(np.int64)
    pad = (-len(flat)) % CT
    return np.concatenate([flat, np.zeros(pad, np.int64)]).reshape(-1, CT).sum(1)


# ---- reduced mode ("Process Fullres" = false): the reduced frame is what is masked and compacted ------------------------------------------
# (source W, H, cap) -> reduced pixels; the 16 : 9 pair straddles SMALL_MAX, the 1 : 1 case is well above it
REDUCED_CASES = ((960, 540, 241), (960, 540, 242), (400, 400, 200))
REDUCED_PIXELS = {(960, 540, 241): 241 * 135, (960, 540, 242): 242 * 136, (400, 400, 200): 200 * 200}


# ---- stream content -----------------------------------------------------------------------------------------------------------------------
STREAM_KINDS = ("flat", "noise", "texture", "impulse")


@lru_cache(maxsize=16)
def stream_frame(W, H, kind):
    """the four frames a stream cycles through: consecutive tickets get masks of n, ~n / 2, a few hundred and 0 survivors"""
    if kind == "flat":
        f = np.full((H, W), BG, np.uint8)
    elif kind == "noise":
        f = synth.random_luma(1, W, H, seed=2 * W + H)[0]
    elif kind == "texture":
        f = synth.flatten_regions(synth.luma_sequence(1, W, H, max_step=0, seed=W + H + 1), region=96 if W * H > 200000 else 24, seed=5)[0]
    else:
        assert kind == "impulse"
        f = impulse_frame(W, H, [(H // 2, W // 2, 21), (H // 4, W // 3, -11)])
    f.setflags(write=False)
    return f


def stream_kinds(n):
    """noise, flat, impulse, texture, ...: record counts large, 0, small, large"""
    order = ("noise", "flat", "impulse", "texture")
    return [order[k % 4] for k in range(n)]
