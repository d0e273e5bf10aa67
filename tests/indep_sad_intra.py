"""hip_sad's intra test and scene-cut rule (include/ofps_hip.h N1i), restated in plain Python integers from the definition alone.  Imports
nothing of the project; numpy only carries the arrays in and out.

  activity   A(k) of block k of the raw current frame: S = sum p, n = B * B, m = (S + n // 2) // n, A = sum |p - m|
  intra      16 * SAD(k) >= q * A(k) (Python integers: nothing wraps); equality is intra
  keep       gate(k) and not intra(k); gate absent = all ones
  cut        P > 0 and 100 * n_intra >= P * n_cand, n_cand = #gate, n_intra = #(gate and intra): every flag of a cut item is 0
"""
import numpy as np

RATIO_MAX, CUT_MAX = 255, 100


def activity(frame, block):
    """frame: [H, W] u8 (any strides) -> A per full lattice block, uint32 [nby * nbx] in raster order"""
    H, W = frame.shape
    nbx, nby = W // block, H // block
    n = block * block
    out = []
    for by in range(nby):
        for bx in range(nbx):
            px = [int(frame[by * block + y, bx * block + x]) for y in range(block) for x in range(block)]
            m = (sum(px) + n // 2) // n
            out.append(sum(abs(p - m) for p in px))
    assert all(0 <= a < 1 << 32 for a in out)
    return np.array(out, np.uint32).reshape(nby * nbx)


def intra_flags(best, act, ratio):
    """best: [nblk, 3] (dx, dy, sad) with the SAD a signed 32-bit number; act: [nblk] -> bool list"""
    assert 1 <= ratio <= RATIO_MAX
    return [16 * int(b[2]) >= ratio * int(a) for b, a in zip(best, act)]


def verdict(best, act, keep_in, ratio, cut=0):
    """-> (keep u8 [nblk], (n_cand, n_intra), is_cut)"""
    assert 0 <= cut <= CUT_MAX
    intra = intra_flags(best, act, ratio)
    gate = [True] * len(intra) if keep_in is None else [int(g) != 0 for g in keep_in]
    n_cand = sum(gate)
    n_intra = sum(1 for g, i in zip(gate, intra) if g and i)
    is_cut = cut > 0 and 100 * n_intra >= cut * n_cand
    keep = [0 if is_cut else int(g and not i) for g, i in zip(gate, intra)]
    return np.array(keep, np.uint8).reshape(len(intra)), (n_cand, n_intra), is_cut


def keep_flags(best, act, keep_in, ratio, cut=0):
    return verdict(best, act, keep_in, ratio, cut)[0]
