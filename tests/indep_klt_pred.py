"""hip_klt's motion prediction (include/ofps_hip.h, row N3p) restated in plain NumPy and Python integers, on top of tests/indep_klt.py's
pyramid, sample, features and record and of tests/indep_klt_fb.py's statuses: the predictor, a pass of N3's tracking that starts from a guess,
the forward-backward check with the negated guess, and the flow of a pair whose features start from the previous pair's slots.  Written from
the header's text; every sum over pixels is an exact Python integer, the f64 lines are those of N3 in its order.  No code is shared with
the library.  Test infrastructure only."""
import numpy as np

from indep_klt import ST_KEPT, ST_NONE, ST_FLAT, ST_LEFT, ST_RESIDUAL, features, pyramid, record, sample, slot_grid
from indep_klt_fb import ST_NO_RETURN

MAX_GUESS = 1 << 23


def predict(prev_slots, W, H, cell):
    """prev_slots int [slots, 6] (x, y, score, dqx, dqy, status) of the previous pair -> int32 [slots, 2], the guess of every slot"""
    nx, ny = slot_grid(W, H, cell)
    ps = np.asarray(prev_slots, np.int64).reshape(ny, nx, 6)
    out = np.zeros((ny, nx, 2), np.int32)
    for cy in range(ny):
        for cx in range(nx):
            cand = [ps[y, x] for x, y in ((cx, cy), (cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1))
                    if 0 <= x < nx and 0 <= y < ny and ps[y, x, 5] == ST_KEPT]
            k = len(cand)
            if k:
                out[cy, cx] = [sorted(int(c[comp]) for c in cand)[(k - 1) // 2] for comp in (3, 4)]
    return out.reshape(-1, 2)


def start_dq(Px, Py, gx, gy, L, W, H):
    """the line that replaces N3's dq = (0, 0) in a pass of L levels that starts at P with the guess g"""
    if abs(gx) > MAX_GUESS or abs(gy) > MAX_GUESS:
        return 0, 0
    dqx, dqy = gx >> (L - 1), gy >> (L - 1)                  # Python's >> on ints: arithmetic
    s = 1 << (L - 1)
    if not (0 <= Px + dqx * s <= 256 * (W - 1) and 0 <= Py + dqy * s <= 256 * (H - 1)):
        return 0, 0
    return dqx, dqy


def track_q_from(pp, pc, Px, Py, gx, gy, w, iters, min_eig=1, max_residual=0, mean_removal=False):
    """one pass from the position P (1/256 pixel) with the guess g: N3's text (N3m's with mean_removal) behind the new first line.
    -> (dqx, dqy, res, status), dq the whole displacement; statuses 2 and 3 report zeros"""
    L = len(pp)
    H, W = pp[0].shape
    n = 2 * w + 1
    N = n * n
    if not (0 <= Px <= 256 * (W - 1) and 0 <= Py <= 256 * (H - 1)):
        return 0, 0, 0, ST_LEFT
    dqx, dqy = start_dq(Px, Py, gx, gy, L, W, H)
    j1, i1 = np.meshgrid(np.arange(-w - 1, w + 2, dtype=np.int64), np.arange(-w - 1, w + 2, dtype=np.int64), indexing="ij")
    j0, i0 = j1[1:-1, 1:-1], i1[1:-1, 1:-1]
    lim = 256 * w

    def inside(l):
        return 0 <= Px + dqx * (1 << l) <= 256 * (W - 1) and 0 <= Py + dqy * (1 << l) <= 256 * (H - 1)

    for l in range(L - 1, -1, -1):
        cqx = ((Px + 128) >> l) - 128
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
        d = d - (2 * int(d.sum()) + N) // (2 * N)
    res = int(np.abs(d).sum())
    if max_residual > 0 and res > 16 * max_residual * N:
        return dqx, dqy, res, ST_RESIDUAL
    return dqx, dqy, res, ST_KEPT


def point_from(pp, pc, x, y, gx, gy, w, iters, min_eig=1, max_residual=0, mean_removal=False, fb_limit=0):
    """the pixel (x, y) forward from the guess g and, with fb_limit > 0, back again from -g.  -> (dqx, dqy, res, status)"""
    H, W = pp[0].shape
    if not (0 <= x < W and 0 <= y < H):
        return 0, 0, 0, ST_LEFT
    dqx, dqy, res, st = track_q_from(pp, pc, 256 * x, 256 * y, gx, gy, w, iters, min_eig, max_residual, mean_removal)
    if fb_limit <= 0 or st != ST_KEPT:
        return dqx, dqy, res, st
    bqx, bqy, _, bst = track_q_from(pc, pp, 256 * x + dqx, 256 * y + dqy, -gx, -gy, w, iters, min_eig, max_residual, mean_removal)
    e = max(abs(dqx + bqx), abs(dqy + bqy))
    return dqx, dqy, res, (ST_KEPT if bst == ST_KEPT and e < fb_limit else ST_NO_RETURN)


def track_from(prev, cur, points, guesses, levels, w, iters, min_eig=1, max_residual=0, mean_removal=False, fb_limit=0):
    """points int [n, 2] (x, y), guesses int [n, 2] (gx, gy) -> int32 [n, 4] (dqx, dqy, res, status)"""
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    gs = np.asarray(guesses, np.int64).reshape(-1, 2)
    return np.array([point_from(pp, pc, int(x), int(y), int(gx), int(gy), w, iters, min_eig, max_residual, mean_removal, fb_limit)
                     for (x, y), (gx, gy) in zip(pts, gs)], np.int32).reshape(-1, 4)


def flow_from(prev, cur, levels, w, iters, prev_slots=None, cell=16, r=2, min_score=1, min_eig=1, max_residual=0, mean_removal=False, fb_limit=0):
    """-> dict(slots int32 [n, 6], residuals, records float32 [count, 4], count, features, guesses) as indep_klt.flow; every feature starts
    from its slot's predicted guess, from zero where prev_slots is None"""
    H, W = prev.shape
    ft = features(prev, cell, r, min_score)
    gs = np.zeros((len(ft), 2), np.int32) if prev_slots is None else predict(prev_slots, W, H, cell)
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    slots = np.zeros((len(ft), 6), np.int32)
    res = np.zeros(len(ft), np.int32)
    rec = []
    for k, (x, y, sc) in enumerate(ft):
        if x < 0:
            slots[k] = (-1, -1, 0, 0, 0, ST_NONE)
            continue
        dqx, dqy, rs, st = point_from(pp, pc, int(x), int(y), int(gs[k, 0]), int(gs[k, 1]), w, iters, min_eig, max_residual, mean_removal, fb_limit)
        slots[k] = (x, y, sc, dqx, dqy, st)
        res[k] = rs
        if st == ST_KEPT:
            rec.append(record(int(x), int(y), dqx, dqy, W, H))
    records = np.array(rec, np.float32).reshape(-1, 4)
    return {"slots": slots, "residuals": res, "records": records, "count": len(records), "features": ft, "guesses": gs}


def flow_chain(frames, levels, w, iters, predict_on=True, **kw):
    """the pairs (frames[k], frames[k + 1]) in order, each started from the slots of the one before -> the list of flow_from's answers"""
    out, prev_slots = [], None
    for a, b in zip(frames[:-1], frames[1:]):
        out.append(flow_from(a, b, levels, w, iters, prev_slots if predict_on else None, **kw))
        prev_slots = out[-1]["slots"]
    return out
