"""hip_klt (include/ofps_hip.h, row N3) restated in plain NumPy and Python integers: the per-cell corner features, the pyramid, the
fixed-point bilinear sample and the pyramidal Lucas-Kanade iteration.  Every sum over pixels is an exact integer (Python ints or
int64, far inside its range); the few f64 lines are Python floats in the definition's order; the square root is math.isqrt.  No code
is shared with the library.  Test infrastructure only."""
import math

import numpy as np

ST_KEPT, ST_NONE, ST_FLAT, ST_LEFT, ST_RESIDUAL = 0, 1, 2, 3, 4


def slot_grid(W, H, cell):
    return -(-W // cell), -(-H // cell)


def down2(img):
    """one level of ofps_hip_sad_down2: (a + b + c + d + 2) >> 2 of every 2 x 2 quad, a last odd row / column unused"""
    H, W = img.shape
    a = img[:2 * (H >> 1), :2 * (W >> 1)].astype(np.int64)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        out.append(down2(out[-1]))
    return out


def score_map(img, r):
    """-> int64 [H, W]: the score of every admissible pixel, -1 elsewhere"""
    H, W = img.shape
    p = img.astype(np.int64)
    out = np.full((H, W), -1, np.int64)
    if W < 2 * r + 3 or H < 2 * r + 3:
        return out
    gx = np.zeros((H, W), np.int64); gy = np.zeros((H, W), np.int64)
    gx[1:-1, 1:-1] = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy[1:-1, 1:-1] = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    n = 2 * r + 1
    h, w = H - 2 * r - 2, W - 2 * r - 2                     # the admissible rectangle: x in [r + 1, W - r - 2]
    a = np.zeros((h, w), np.int64); b = np.zeros((h, w), np.int64); c = np.zeros((h, w), np.int64)
    for j in range(n):
        for i in range(n):
            sx = gx[1 + j:1 + j + h, 1 + i:1 + i + w]; sy = gy[1 + j:1 + j + h, 1 + i:1 + i + w]
            a += sx * sx; b += sx * sy; c += sy * sy
    sc = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            av, bv, cv = int(a[y, x]), int(b[y, x]), int(c[y, x])
            D = (av - cv) * (av - cv) + 4 * bv * bv
            s = math.isqrt(D)
            sc[y, x] = av + cv - (s + (1 if s * s < D else 0))
    out[r + 1:H - r - 1, r + 1:W - r - 1] = sc
    return out


def features(img, cell=16, r=2, min_score=1):
    """-> int32 [slots, 3]: (x, y, score) per cell in raster order, (-1, -1, 0) for a cell without a feature"""
    H, W = img.shape
    sc = score_map(img, r)
    nx, ny = slot_grid(W, H, cell)
    out = np.zeros((nx * ny, 3), np.int32)
    for cy in range(ny):
        for cx in range(nx):
            t = sc[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell]
            k = int(np.argmax(t))                           # the first maximum in raster order: smallest y, then smallest x
            ly, lx = divmod(k, t.shape[1])
            best = int(t[ly, lx])
            out[cy * nx + cx] = (cx * cell + lx, cy * cell + ly, best) if best >= min_score else (-1, -1, 0)
    return out


def sample(img, qx, qy):
    """S(img, q) on int64 arrays of 1/256-pixel positions -> int64, 8 fractional bits"""
    H, W = img.shape
    p = img.astype(np.int64)
    ix = qx >> 8; iy = qy >> 8
    fx = qx & 255; fy = qy & 255
    x0 = np.clip(ix, 0, W - 1); x1 = np.clip(ix + 1, 0, W - 1)
    y0 = np.clip(iy, 0, H - 1); y1 = np.clip(iy + 1, 0, H - 1)
    s = (256 - fx) * (256 - fy) * p[y0, x0] + fx * (256 - fy) * p[y0, x1] + (256 - fx) * fy * p[y1, x0] + fx * fy * p[y1, x1]
    return (s + 128) >> 8


def track_point(pp, pc, x, y, w, iters, min_eig=1, max_residual=0):
    """pp, pc: the two pyramids (level 0 first).  -> (dqx, dqy, res, status); a slot that is not kept or lost by its residual reports
    zeros in front of its status"""
    L = len(pp)
    H, W = pp[0].shape
    n = 2 * w + 1
    if not (0 <= x < W and 0 <= y < H):
        return 0, 0, 0, ST_LEFT
    dqx = dqy = 0
    j1, i1 = np.meshgrid(np.arange(-w - 1, w + 2, dtype=np.int64), np.arange(-w - 1, w + 2, dtype=np.int64), indexing="ij")
    j0, i0 = j1[1:-1, 1:-1], i1[1:-1, 1:-1]
    lim = 256 * w

    def inside(l):
        return 0 <= 256 * x + dqx * (1 << l) <= 256 * (W - 1) and 0 <= 256 * y + dqy * (1 << l) <= 256 * (H - 1)

    for l in range(L - 1, -1, -1):
        cqx = (((2 * x + 1) * 128) >> l) - 128
        cqy = (((2 * y + 1) * 128) >> l) - 128
        I = sample(pp[l], cqx + 256 * i1, cqy + 256 * j1)
        Ix = I[1:-1, 2:] - I[1:-1, :-2]
        Iy = I[2:, 1:-1] - I[:-2, 1:-1]
        Ic = I[1:-1, 1:-1]
        A11 = int((Ix * Ix).sum()); A12 = int((Ix * Iy).sum()); A22 = int((Iy * Iy).sum())
        T = min_eig * n * n * 262144
        X = float(A11 - T); Y = float(A22 - T); Z = float(A12)
        if not (X * Y >= Z * Z and X + Y >= 0.0):
            return 0, 0, 0, ST_FLAT
        det = float(A11) * float(A22) - Z * Z
        if det <= 0.0:
            return 0, 0, 0, ST_FLAT
        for _ in range(iters):
            if not inside(l):
                return 0, 0, 0, ST_LEFT
            J = sample(pc[l], cqx + dqx + 256 * i0, cqy + dqy + 256 * j0)
            d = J - Ic
            b1 = int((d * Ix).sum()); b2 = int((d * Iy).sum())
            num_x = float(A22) * float(b1) - Z * float(b2)
            ux = (-512.0 * num_x) / det
            num_y = float(A11) * float(b2) - Z * float(b1)
            uy = (-512.0 * num_y) / det
            uqx = int(max(-lim, min(lim, round(ux))))      # Python's round: half to even
            uqy = int(max(-lim, min(lim, round(uy))))
            dqx += uqx; dqy += uqy
            if uqx == 0 and uqy == 0:
                break
        if l > 0:
            dqx *= 2; dqy *= 2
    if not inside(0):
        return 0, 0, 0, ST_LEFT
    J = sample(pc[0], cqx + dqx + 256 * i0, cqy + dqy + 256 * j0)
    res = int(np.abs(J - Ic).sum())
    if max_residual > 0 and res > 16 * max_residual * n * n:
        return dqx, dqy, res, ST_RESIDUAL
    return dqx, dqy, res, ST_KEPT


def track(prev, cur, points, levels, w, iters, min_eig=1, max_residual=0):
    """points int [n, 2] (x, y) -> int32 [n, 4] (dqx, dqy, res, status)"""
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    return np.array([track_point(pp, pc, int(x), int(y), w, iters, min_eig, max_residual) for x, y in pts], np.int32).reshape(-1, 4)


def record(x, y, dqx, dqy, W, H):
    f = np.float32
    return np.array([(f(x) + f(0.5)) / f(W), (f(y) + f(0.5)) / f(H), (f(dqx) / f(256.0)) / f(W), (f(dqy) / f(256.0)) / f(H)], np.float32)


def flow(prev, cur, levels, w, iters, cell=16, r=2, min_score=1, min_eig=1, max_residual=0):
    """-> dict(slots int32 [n, 6] (x, y, score, dqx, dqy, status), records float32 [count, 4], count)"""
    H, W = prev.shape
    ft = features(prev, cell, r, min_score)
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    slots = np.zeros((len(ft), 6), np.int32)
    res = np.zeros(len(ft), np.int32)
    rec = []
    for k, (x, y, sc) in enumerate(ft):
        if x < 0:
            slots[k] = (-1, -1, 0, 0, 0, ST_NONE)
            continue
        dqx, dqy, rs, st = track_point(pp, pc, int(x), int(y), w, iters, min_eig, max_residual)
        slots[k] = (x, y, sc, dqx, dqy, st)
        res[k] = rs
        if st == ST_KEPT:
            rec.append(record(int(x), int(y), dqx, dqy, W, H))
    records = np.array(rec, np.float32).reshape(-1, 4)
    return {"slots": slots, "residuals": res, "records": records, "count": len(records), "features": ft}
