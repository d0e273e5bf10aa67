"""Restatement of N1v, hip_sad's median test (include/ofps_hip.h "N1v"), in plain Python: sorted lists per block, Python integers (nothing
wraps, nothing is rounded).  Nothing of the library under test is imported."""
import numpy as np

LIMIT_MAX = 255
R2_MAX = (1 << 32) - 1                                   # the uint32 the library reports r2 in saturates here


def neighbours(bx, by, nbx, nby):
    """the up to eight lattice neighbours of (bx, by), in raster order"""
    return [(bx + i, by + j) for j in (-1, 0, 1) for i in (-1, 0, 1) if (i or j) and 0 <= bx + i < nbx and 0 <= by + j < nby]


def doubled_median(values):
    """values: a non-empty list of integers -> s[(n - 1) >> 1] + s[n >> 1] of the sorted list: twice the median, exactly"""
    s = sorted(int(v) for v in values)
    n = len(s)
    return s[(n - 1) >> 1] + s[n >> 1]


def residual2(best, keep_in, nbx, nby):
    """best [nbx * nby, >= 2] (dx, dy, ...) integer winners in raster order; keep_in [nbx * nby] or None = all ones
    -> r2 [nbx * nby] uint32: max(|2 dx - M_x|, |2 dy - M_y|) over the kept neighbours, 0 for a block with none"""
    best = np.asarray(best).reshape(nbx * nby, -1)
    kin = [1] * (nbx * nby) if keep_in is None else [int(v) for v in np.asarray(keep_in).reshape(nbx * nby)]
    out = []
    for by in range(nby):
        for bx in range(nbx):
            nb = [y * nbx + x for x, y in neighbours(bx, by, nbx, nby) if kin[y * nbx + x]]
            k = by * nbx + bx
            if not nb:
                out.append(0)
                continue
            rx = abs(2 * int(best[k][0]) - doubled_median([best[j][0] for j in nb]))
            ry = abs(2 * int(best[k][1]) - doubled_median([best[j][1] for j in nb]))
            out.append(min(max(rx, ry), R2_MAX))
    return np.array(out, np.uint32)


def keep_flags(best, keep_in, nbx, nby, limit):
    """-> uint8 [nbx * nby]: keep_in AND r2 < 2 * limit.  One pass: the neighbours' INCOMING flags are read, never a verdict of this test"""
    assert 1 <= limit <= LIMIT_MAX
    r2 = residual2(best, keep_in, nbx, nby)
    kin = np.ones(nbx * nby, bool) if keep_in is None else np.asarray(keep_in).reshape(nbx * nby) != 0
    return (kin & (r2.astype(np.int64) < 2 * limit)).astype(np.uint8)
