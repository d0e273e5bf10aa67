"""hip_klt's forward-backward check (include/ofps_hip.h, row N3f) restated in plain NumPy and Python integers, on top of tests/indep_klt.py's
pyramid, sample, features and record: track_q, one pass of N3's tracking started at a position P in 1/256 pixel (with N3m's three changes
where mean removal is on), and the check built from two of them.  Every sum over pixels is an exact Python integer; the f64 lines are
those of N3, in its order.  No code is shared with the library.  Test infrastructure only."""
import numpy as np

from indep_klt import ST_KEPT, ST_NONE, ST_FLAT, ST_LEFT, ST_RESIDUAL, features, pyramid, record, sample

ST_NO_RETURN = 5


def track_q(pp, pc, Px, Py, w, iters, min_eig=1, max_residual=0, mean_removal=False):
    """pp, pc: the pyramids of the frame the template comes from and of the frame it is looked for in (level 0 first); (Px, Py): where the
    pass starts, in 1/256 pixel.  -> (dqx, dqy, res, status); statuses 2 and 3 report zeros in front of the status"""
    L = len(pp)
    H, W = pp[0].shape
    n = 2 * w + 1
    N = n * n
    if not (0 <= Px <= 256 * (W - 1) and 0 <= Py <= 256 * (H - 1)):
        return 0, 0, 0, ST_LEFT
    dqx = dqy = 0
    j1, i1 = np.meshgrid(np.arange(-w - 1, w + 2, dtype=np.int64), np.arange(-w - 1, w + 2, dtype=np.int64), indexing="ij")
    j0, i0 = j1[1:-1, 1:-1], i1[1:-1, 1:-1]
    lim = 256 * w

    def inside(l):
        return 0 <= Px + dqx * (1 << l) <= 256 * (W - 1) and 0 <= Py + dqy * (1 << l) <= 256 * (H - 1)

    for l in range(L - 1, -1, -1):
        cqx = ((Px + 128) >> l) - 128                        # Python's >> on ints: arithmetic
        cqy = ((Py + 128) >> l) - 128
        I = sample(pp[l], cqx + 256 * i1, cqy + 256 * j1)
        Ix = I[1:-1, 2:] - I[1:-1, :-2]
        Iy = I[2:, 1:-1] - I[:-2, 1:-1]
        Ic = I[1:-1, 1:-1]
        A11 = int((Ix * Ix).sum()); A12 = int((Ix * Iy).sum()); A22 = int((Iy * Iy).sum())
        T = min_eig * N * 262144
        if mean_removal:
            sx = int(Ix.sum()); sy = int(Iy.sum())
            A11 = N * A11 - sx * sx; A12 = N * A12 - sx * sy; A22 = N * A22 - sy * sy
            T *= N
        X = float(A11 - T); Y = float(A22 - T); Z = float(A12)
        if not (X * Y >= Z * Z and X + Y >= 0.0):
            return 0, 0, 0, ST_FLAT
        det = float(A11) * float(A22) - Z * Z
        if det <= 0.0:
            return 0, 0, 0, ST_FLAT
        for _ in range(iters):
            if not inside(l):
                return 0, 0, 0, ST_LEFT
            d = sample(pc[l], cqx + dqx + 256 * i0, cqy + dqy + 256 * j0) - Ic
            b1 = int((d * Ix).sum()); b2 = int((d * Iy).sum())
            if mean_removal:
                sd = int(d.sum())
                b1 = N * b1 - sd * sx; b2 = N * b2 - sd * sy
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
    d = sample(pc[0], cqx + dqx + 256 * i0, cqy + dqy + 256 * j0) - Ic
    if mean_removal:
        d = d - (2 * int(d.sum()) + N) // (2 * N)             # Python's //: floor towards minus infinity
    res = int(np.abs(d).sum())
    if max_residual > 0 and res > 16 * max_residual * N:
        return dqx, dqy, res, ST_RESIDUAL
    return dqx, dqy, res, ST_KEPT


def track_points_q(prev, cur, points_q, levels, w, iters, min_eig=1, max_residual=0, mean_removal=False):
    """points int [n, 2] (Px, Py) in 1/256 pixel -> int32 [n, 4] (dqx, dqy, res, status)"""
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    pts = np.asarray(points_q, np.int64).reshape(-1, 2)
    return np.array([track_q(pp, pc, int(x), int(y), w, iters, min_eig, max_residual, mean_removal) for x, y in pts], np.int32).reshape(-1, 4)


def check_point(pp, pc, x, y, w, iters, min_eig=1, max_residual=0, mean_removal=False, fb_limit=0):
    """the pixel (x, y) forward, and with fb_limit > 0 back again.  -> (dqx, dqy, res, status, back): back is None where no backward pass
    ran, else its (bqx, bqy, bres, bstatus, e)"""
    H, W = pp[0].shape
    if not (0 <= x < W and 0 <= y < H):
        return 0, 0, 0, ST_LEFT, None
    dqx, dqy, res, st = track_q(pp, pc, 256 * x, 256 * y, w, iters, min_eig, max_residual, mean_removal)
    if fb_limit <= 0 or st != ST_KEPT:
        return dqx, dqy, res, st, None
    bqx, bqy, bres, bst = track_q(pc, pp, 256 * x + dqx, 256 * y + dqy, w, iters, min_eig, max_residual, mean_removal)
    e = max(abs(dqx + bqx), abs(dqy + bqy))
    kept = bst == ST_KEPT and e < fb_limit
    return dqx, dqy, res, (ST_KEPT if kept else ST_NO_RETURN), (bqx, bqy, bres, bst, e)


def track(prev, cur, points, levels, w, iters, min_eig=1, max_residual=0, mean_removal=False, fb_limit=0):
    """points int [n, 2] (x, y) -> int32 [n, 4] (dqx, dqy, res, status)"""
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    return np.array([check_point(pp, pc, int(x), int(y), w, iters, min_eig, max_residual, mean_removal, fb_limit)[:4] for x, y in pts],
                    np.int32).reshape(-1, 4)


def flow_all(prev, cur, levels, w, iters, cell=16, r=2, min_score=1, min_eig=1, max_residual=0, mean_removal=False):
    """Both passes of every feature once, whatever the limit: -> dict(features, fwd int64 [n, 4], back int64 [n, 5] (bqx, bqy, bres, bstatus,
    e; -1 in bstatus where the forward pass was not kept)).  at_limit() makes the answer of a limit from it"""
    ft = features(prev, cell, r, min_score)
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    fwd = np.zeros((len(ft), 4), np.int64)
    back = np.zeros((len(ft), 5), np.int64)
    back[:, 3] = -1
    for k, (x, y, sc) in enumerate(ft):
        if x < 0:
            fwd[k] = (0, 0, 0, ST_NONE)
            continue
        out = check_point(pp, pc, int(x), int(y), w, iters, min_eig, max_residual, mean_removal, fb_limit=1)
        fwd[k] = out[:4]
        if out[4] is not None:
            fwd[k, 3] = ST_KEPT
            back[k] = out[4]
    return {"features": ft, "fwd": fwd, "back": back, "shape": prev.shape}


def at_limit(both, fb_limit):
    """-> dict(slots int32 [n, 6] (x, y, score, dqx, dqy, status), residuals, records float32 [count, 4], count) as indep_klt.flow, with the
    check at fb_limit (0 = off)"""
    ft, fwd, back = both["features"], both["fwd"], both["back"]
    H, W = both["shape"]
    slots = np.zeros((len(ft), 6), np.int32)
    res = np.zeros(len(ft), np.int32)
    rec = []
    for k, (x, y, sc) in enumerate(ft):
        dqx, dqy, rs, st = (int(v) for v in fwd[k])
        if st == ST_NONE:
            slots[k] = (-1, -1, 0, 0, 0, ST_NONE)
            continue
        if st == ST_KEPT and fb_limit > 0 and not (back[k, 3] == ST_KEPT and back[k, 4] < fb_limit):
            st = ST_NO_RETURN
        slots[k] = (x, y, sc, dqx, dqy, st)
        res[k] = rs
        if st == ST_KEPT:
            rec.append(record(int(x), int(y), dqx, dqy, W, H))
    records = np.array(rec, np.float32).reshape(-1, 4)
    return {"slots": slots, "residuals": res, "records": records, "count": len(records), "features": ft}


def flow(prev, cur, levels, w, iters, cell=16, r=2, min_score=1, min_eig=1, max_residual=0, mean_removal=False, fb_limit=0):
    return at_limit(flow_all(prev, cur, levels, w, iters, cell, r, min_score, min_eig, max_residual, mean_removal), fb_limit)
