"""hip_klt with mean removal (include/ofps_hip.h, row N3m) restated in plain NumPy and Python integers: tests/indep_klt.py's pyramid,
sample, features and record as they are, and track_point with the row's three changes -- the centred normal matrix per level, the
centred right-hand side per iteration, the residual around the window's mean difference.  Every sum over pixels is an exact Python
integer; the f64 lines are those of N3, in its order.  No code is shared with the library.  Test infrastructure only."""
import numpy as np

from indep_klt import ST_KEPT, ST_NONE, ST_FLAT, ST_LEFT, ST_RESIDUAL, features, pyramid, record, sample


def track_point(pp, pc, x, y, w, iters, min_eig=1, max_residual=0):
    """pp, pc: the two pyramids (level 0 first).  -> (dqx, dqy, res, status); a slot that is not kept or lost by its residual reports
    zeros in front of its status"""
    L = len(pp)
    H, W = pp[0].shape
    n = 2 * w + 1
    N = n * n
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
        sx = int(Ix.sum()); sy = int(Iy.sum())
        A11 = N * int((Ix * Ix).sum()) - sx * sx
        A12 = N * int((Ix * Iy).sum()) - sx * sy
        A22 = N * int((Iy * Iy).sum()) - sy * sy
        T = min_eig * N * N * 262144
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
            sd = int(d.sum())
            b1 = N * int((d * Ix).sum()) - sd * sx
            b2 = N * int((d * Iy).sum()) - sd * sy
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
    d = J - Ic
    sd = int(d.sum())
    m = (2 * sd + N) // (2 * N)                              # Python's //: floor towards minus infinity
    res = int(np.abs(d - m).sum())
    if max_residual > 0 and res > 16 * max_residual * N:
        return dqx, dqy, res, ST_RESIDUAL
    return dqx, dqy, res, ST_KEPT


def track(prev, cur, points, levels, w, iters, min_eig=1, max_residual=0):
    """points int [n, 2] (x, y) -> int32 [n, 4] (dqx, dqy, res, status)"""
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    return np.array([track_point(pp, pc, int(x), int(y), w, iters, min_eig, max_residual) for x, y in pts], np.int32).reshape(-1, 4)


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
