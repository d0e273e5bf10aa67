"""Case lists for hip_flow (ofps_amd/csrc/farneback.hip) over its kernel and parameter domain, as data, plus the frame makers.  CPU only: numpy,
the synthetic clips and -- in the frame makers' callers -- the CPU oracle; never the library under test.  tests/test_farneback_domain_cpu.py
checks that every case has the property it is named for (so that no GPU test passes vacuously) and the oracle against the independent
restatement over the same grid; tests/test_farneback_domain_gpu.py runs the cases on the device.

What a case is named for is a compiled variant of farneback.hip:
  fb_iter_kernel<M_>            M_ = winsize / 2 = 0 .. 7
  fb_polyexp_kernel<7 | 5 | 0>  poly_n 7, 5, anything else up to 15 (= kMaxPolyN: layer 0's staging fills its LDS region exactly)
  fb_pyr_h_kernel<RS>           row pitch 0 / 1 / 2 by need = W + 2 * ((r_K + 3) & ~3) <= 2,312 / 4,360 / 16,904
  fb_pyr_h_layer<NRL, RS>       rows per lane 8 / 4 / 2 / 1 for layer k <= 2 / 3 / 4 / >= 5
  fb_pyr_v_kernel               short (r <= 4: layers 1, 2) and long column filters (r = 9, 19, 39, 79 for layers 3 .. 6)
  fb_area_kernel                the initial flow brought to the coarsest layer: ratio 1, non-integer, 8, 64"""
from functools import lru_cache

import numpy as np

from ofps_amd import synth

DEFAULTS = dict(levels=5, winsize=13, iters=3, poly_n=7, poly_sigma=1.5)          # cv-decoder/src/lib.rs:188-199

# ---- (a) window x polynomial grid ---------------------------------------------------------------------------------------------------------
WINSIZES = (1, 3, 5, 7, 9, 11, 13, 15)
POLY_NS = (1, 2, 3, 4, 5, 6, 7, 9, 12, 15)
SIGMA0_POLY_NS = (5, 7, 15)                     # poly_sigma = 0 -> 0.3 n (FarnebackPrepareGaussian)
GRID_W, GRID_H, GRID_LEVELS, GRID_ITERS = 97, 64, 3, 2          # two layers (97 x 64, 48 x 32): 4 x 4 update tiles, 2 x 4 expansion tiles
CORNER_W, CORNER_H, CORNER_LEVELS = 200, 136, 5                 # three layers (200 x 136, 100 x 68, 50 x 34)
CORNERS = ((1, 1), (1, 15), (15, 1), (15, 15))                  # (winsize, poly_n)


def grid_sigma(poly_n):
    """the grid's poly_sigma, as the float32 value the C ABI carries (the oracle gets the same value)"""
    return float(np.float32(0.3 * poly_n + 0.2))


def grid_sets(winsize):
    """the 13 parameter sets of one winsize: every poly_n at its grid sigma, then poly_sigma = 0 at 5, 7, 15"""
    out = [dict(levels=GRID_LEVELS, winsize=winsize, iters=GRID_ITERS, poly_n=n, poly_sigma=grid_sigma(n)) for n in POLY_NS]
    out += [dict(levels=GRID_LEVELS, winsize=winsize, iters=GRID_ITERS, poly_n=n, poly_sigma=0.0) for n in SIGMA0_POLY_NS]
    return out


def flow_is_compared(winsize, poly_n):
    """winsize 1 with poly_n <= 6: a 1 x 1 window solves each pixel's 2 x 2 system alone and rounding decides the outcome (f32 and f64
    restatements differ by tens of pixels): no flow comparison between RESTATEMENTS there.  (HIP against the oracle is bits everywhere.)"""
    return winsize >= 3 or poly_n >= 7


# ---- (b) layer counts and row-filter variants -----------------------------------------------------------------------------------------------
# name -> W, H, levels, iters, layers above the frame, row pitch (None: no pyramid launch), rows-per-lane forms of layers 1 .. K
LAYER_CASES = {
    "layers0": dict(W=63, H=64, levels=5, iters=3, layers=0, pitch=None, forms=()),
    "layers1": dict(W=64, H=64, levels=5, iters=3, layers=1, pitch=0, forms=(8,)),
    "layers2": dict(W=129, H=160, levels=5, iters=3, layers=2, pitch=0, forms=(8, 8)),
    "layers3_size_ends_the_pyramid": dict(W=640, H=360, levels=16, iters=3, layers=3, pitch=0, forms=(8, 8, 4)),
    "layers4": dict(W=512, H=600, levels=5, iters=2, layers=4, pitch=0, forms=(8, 8, 4, 2)),
    "layers5": dict(W=1024, H=1100, levels=5, iters=1, layers=5, pitch=0, forms=(8, 8, 4, 2, 1)),
    "layers6": dict(W=2048, H=2048, levels=6, iters=1, layers=6, pitch=0, forms=(8, 8, 4, 2, 1, 1)),
    "levels0": dict(W=640, H=360, levels=0, iters=3, layers=0, pitch=None, forms=()),
    "levels1": dict(W=640, H=360, levels=1, iters=3, layers=1, pitch=0, forms=(8,)),
    "levels2": dict(W=640, H=360, levels=2, iters=3, layers=2, pitch=0, forms=(8, 8)),
    "pitch1_k4": dict(W=2304, H=512, levels=5, iters=1, layers=4, pitch=1, forms=(8, 8, 4, 2)),
    "pitch1_k5": dict(W=2304, H=1024, levels=5, iters=1, layers=5, pitch=1, forms=(8, 8, 4, 2, 1)),
    "pitch2_k5": dict(W=4400, H=1024, levels=5, iters=1, layers=5, pitch=2, forms=(8, 8, 4, 2, 1)),
    "pitch0_last": dict(W=2304, H=64, levels=1, iters=3, layers=1, pitch=0, forms=(8,)),
    "pitch1_first": dict(W=2305, H=64, levels=1, iters=3, layers=1, pitch=1, forms=(8,)),
    "pitch1_last": dict(W=4352, H=64, levels=1, iters=3, layers=1, pitch=1, forms=(8,)),
    "pitch2_first": dict(W=4353, H=64, levels=1, iters=3, layers=1, pitch=2, forms=(8,)),
    "widest": dict(W=16384, H=64, levels=5, iters=1, layers=1, pitch=2, forms=(8,)),
}
PITCH_BYTES = (2312, 4360, 16904)               # kPyrRS0 / 1 / 2
MAX_W = 16384


def blur_radius(k):
    """half the tap count of layer k's Gaussian: sigma = (2^k - 1) / 2, ksize = max(cvRound(5 sigma) | 1, 3)"""
    return max(int(np.rint((2.0 ** k - 1.0) * 0.5 * 5)) | 1, 3) // 2


def row_pitch(W, K):
    """which of the three compiled row pitches a frame of width W with K layers above it selects (None: K = 0, no launch)"""
    if K == 0:
        return None
    need = W + 2 * ((blur_radius(K) + 3) & ~3)
    return next(i for i, b in enumerate(PITCH_BYTES) if need <= b)


def rows_per_lane(k):
    return 8 if k <= 2 else (4 if k == 3 else (2 if k == 4 else 1))


# ---- (c) small and ragged frames (W, H) -----------------------------------------------------------------------------------------------------
SMALL_FRAMES = ((1, 1), (2, 3), (1, 40), (40, 1), (5, 40),
                (31, 33), (33, 17), (32, 16), (64, 16), (65, 17),
                (63, 64), (64, 64), (65, 127), (64, 200), (129, 66))
# the widest halos: 7 (update), 15 (expansion) -- with the grid's sigma (4.7): at cv-decoder's 1.5 the taps beyond 9 are below half an ulp of the sums
LARGEST = dict(winsize=15, poly_n=15, poly_sigma=grid_sigma(15))

# ---- (d) strides ------------------------------------------------------------------------------------------------------------------------------
STRIDE_SIZES = ((322, 181), (640, 360))
STRIDE_PADS = (1, 3, 64)
STRIDE_FILLS = ("255", "noise")
BASE_OFFSETS = (1, 2, 3)                        # bytes into the buffer, at stride W + 64
OUTPUTS = ("flow", "records", "both")

# ---- (e) iterations at 128 x 96 ---------------------------------------------------------------------------------------------------------------
ITERS = (1, 2, 5, 64)
ITERS_W, ITERS_H = 128, 96

# ---- (f) initial flow -------------------------------------------------------------------------------------------------------------------------
# from the previous pair: name -> W, H, levels, iters, layers, ratio of the frame to the coarsest layer (x, y)
INIT_CASES = {
    "ratio1_levels0": dict(W=200, H=120, levels=0, iters=3, layers=0, ratio=(1.0, 1.0)),
    "one_layer": dict(W=200, H=120, levels=5, iters=3, layers=1, ratio=(2.0, 2.0)),
    "three_layers_non_integer": dict(W=480, H=270, levels=5, iters=3, layers=3, ratio=(8.0, 270 / 34)),
    "six_layers_ratio64": dict(W=2048, H=2048, levels=6, iters=1, layers=6, ratio=(64.0, 64.0)),
    "integer_ratio4": dict(W=256, H=128, levels=2, iters=3, layers=2, ratio=(4.0, 4.0)),
    "integer_ratio1": dict(W=128, H=64, levels=0, iters=3, layers=0, ratio=(1.0, 1.0)),
    "ratio8": dict(W=256, H=256, levels=5, iters=3, layers=3, ratio=(8.0, 8.0)),
}
INTEGER_RATIO_INIT = ("integer_ratio4", "integer_ratio1")         # where the independent restatement defines the initial flow
SYNTH_INIT_W, SYNTH_INIT_H = 200, 120
SYNTH_INITS = ("subpixel", "forty", "outside")


def synthetic_init(kind, W=SYNTH_INIT_W, H=SYNTH_INIT_H, seed=7):
    """finite starting flows [H, W, 2] f32: sub-pixel noise, +-40 px, and one whose every vector is at least 2 max(W, H) long in BOTH
    components (signs constant over 40 x 40 blocks, so that the coarsest layer's block means stay that long too)"""
    rng = np.random.default_rng(seed)
    if kind == "subpixel":
        return rng.uniform(-0.5, 0.5, (H, W, 2)).astype(np.float32)
    if kind == "forty":
        return rng.uniform(-40, 40, (H, W, 2)).astype(np.float32)
    assert kind == "outside"
    amp = 2.0 * max(W, H)
    sign = rng.choice([-1.0, 1.0], ((H + 39) // 40, (W + 39) // 40, 2))
    sign = np.repeat(np.repeat(sign, 40, 0), 40, 1)[:H, :W]
    return (sign * amp * rng.uniform(1.0, 1.5, (H, W, 2))).astype(np.float32)


# ---- (g) refusals: keyword arguments of farneback_flow on a 128 x 96 pair, and geometries ---------------------------------------------------
REFUSED_PARAMS = (dict(levels=-1), dict(levels=17), dict(winsize=0), dict(winsize=12), dict(winsize=17), dict(poly_n=0), dict(poly_n=16),
                  dict(iters=0), dict(iters=65))
REFUSED_GEOMETRIES = (dict(W=4096, H=4096, levels=7), dict(W=16385, H=8, levels=5))        # seven layers above the frame; wider than 16,384

# ---- (h) one context, call after call: (W, H, poly_n) ----------------------------------------------------------------------------------------
BACK_TO_BACK = ((2304, 512, 7), (64, 64, 15), (640, 360, 5), (2304, 512, 7))
STREAM_W, STREAM_H = 352, 200

# ---- (i) decoder arguments at 480 x 270: (levels, radius) -------------------------------------------------------------------------------------
DECODER_W, DECODER_H = 480, 270
DECODER_ARGS = ((5, 0), (5, 2), (5, 7), (0, 6), (6, 6))


def decoder_winsize(radius):
    """the window the dense decoders hand to Farneback's flow (dense_decoder.hip: winsize = 2 * radius + 1; poly_n 7, poly_sigma 1.5)"""
    return 2 * radius + 1


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _regions(n, W, H, seed):
    fr = synth.luma_sequence(n, W, H, max_step=3, seed=seed)
    fr.setflags(write=False)
    return fr


def regions(W, H, n=2, seed=None):
    """region-motion content (flow discontinuities), n frames [n, H, W] u8, read-only and shared"""
    return _regions(n, W, H, W + H if seed is None else seed)


@lru_cache(maxsize=None)
def _camera(W, H, seed):
    fr, _ = synth.rotation_clip([(0.1, 0.05, 0.2)], W, H, 60.0, seed=seed)
    fr.setflags(write=False)
    return fr


def camera(W, H, seed=3):
    """a smooth camera rotation, two frames (sizes from 64 px up: the clip needs a margin around the frame)"""
    return _camera(W, H, seed)


def padded(frame, stride, fill, offset=0, seed=1):
    """-> (buffer u8 [offset + H * stride], view [H, W] into it): the frame's rows `stride` bytes apart starting `offset` bytes in; every
    byte that is not a pixel is 255 or noise"""
    H, W = frame.shape
    n = offset + H * stride
    buf = np.full(n, 255, np.uint8) if fill == "255" else np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    view = buf[offset:].reshape(H, stride)[:, :W]
    view[...] = frame
    return buf, view
