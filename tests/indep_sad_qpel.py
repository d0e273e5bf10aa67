"""NumPy restatement of N1q, the quarter-pel refinement of the SAD block matcher (include/ofps_hip.h, DESIGN.md "N1q").

Independent of the HIP kernel in form: the whole previous frame is interpolated once to its 4x plane (H.264 luma
interpolation, ITU-T H.264 8.4.2.2.1, frame edges replicated) and every candidate of every block is a gather from it.
The integer winners come from the caller (oracle.sad_flow's `best`)."""
import numpy as np

TAPS = (1, -5, 20, 20, -5, 1)


def _tap6(p, axis):
    """six-tap sums at the half positions between samples i and i+1, i = 0 .. n-2, of an int array; edges replicated"""
    n = p.shape[axis]
    idx = np.arange(n - 1)
    acc = np.zeros(np.take(p, idx, axis=axis).shape, np.int64)
    for k, w in zip(range(-2, 4), TAPS):
        acc += w * np.take(p, np.clip(idx + k, 0, n - 1), axis=axis)
    return acc


def _clip255(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def half_plane(img):
    """-> [2H-1, 2W-1] u8: the half-pel grid (integer samples at even, even)"""
    a = np.asarray(img, np.uint8).astype(np.int64)
    H, W = a.shape
    b1 = _tap6(a, 1)                                   # [H, W-1], unrounded
    h1 = _tap6(a, 0)                                   # [H-1, W]
    j1 = _tap6(b1, 0)                                  # [H-1, W-1]: the six taps over the unrounded b1 of six rows
    hg = np.zeros((2 * H - 1, 2 * W - 1), np.uint8)
    hg[0::2, 0::2] = a
    hg[0::2, 1::2] = _clip255((b1 + 16) >> 5)
    hg[1::2, 0::2] = _clip255((h1 + 16) >> 5)
    hg[1::2, 1::2] = _clip255((j1 + 512) >> 10)
    return hg


def quarter_plane(img):
    """-> [4(H-1)+1, 4(W-1)+1] u8: the frame at every quarter-pel position"""
    hg = half_plane(img).astype(np.int32)
    q = np.zeros((2 * hg.shape[0] - 1, 2 * hg.shape[1] - 1), np.uint8)
    q[0::2, 0::2] = hg
    q[0::2, 1::2] = (hg[:, :-1] + hg[:, 1:] + 1) >> 1                    # left and right neighbours
    q[1::2, 0::2] = (hg[:-1, :] + hg[1:, :] + 1) >> 1                    # upper and lower neighbours
    # both odd: of the four surrounding half-grid points the two that are half-pel in exactly one direction, i.e. whose
    # half-grid coordinates have an odd sum (never the integer sample (even, even), never j (odd, odd))
    ya, xa = np.meshgrid(np.arange(hg.shape[0] - 1), np.arange(hg.shape[1] - 1), indexing="ij")
    main = (hg[:-1, :-1] + hg[1:, 1:] + 1) >> 1
    anti = (hg[:-1, 1:] + hg[1:, :-1] + 1) >> 1
    q[1::2, 1::2] = np.where((xa + ya) % 2 == 1, main, anti)
    return q


def refine(prev, cur, B, R, best_int, W=None):
    """best_int: [nblk, 3] (dx, dy, sad) integer winners, raster order -> (entries [nblk, 4] f32, best [nblk, 3] i32 (Dx, Dy, SAD))"""
    prev = np.asarray(prev, np.uint8); cur = np.asarray(cur, np.uint8)
    H = prev.shape[0]
    W = prev.shape[1] if W is None else W
    prev = prev[:, :W]; cur = cur[:, :W]
    nbx, nby = W // B, H // B
    n = nbx * nby
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32)
    q = quarter_plane(prev)
    d = np.asarray(best_int, np.int64).reshape(n, 3)
    x0 = (np.arange(n) % nbx) * B
    y0 = (np.arange(n) // nbx) * B
    yy, xx = np.meshgrid(np.arange(B), np.arange(B), indexing="ij")
    cblk = cur[(y0[:, None, None] + yy), (x0[:, None, None] + xx)].astype(np.int32)      # [n, B, B]
    bias = 4 * R + 3
    best_key = np.full(n, np.iinfo(np.int64).max, np.int64)
    for fy in range(-3, 4):
        for fx in range(-3, 4):
            Dx, Dy = 4 * d[:, 0] + fx, 4 * d[:, 1] + fy
            valid = (4 * x0 + Dx >= 0) & (4 * (x0 + B - 1) + Dx <= 4 * (W - 1)) & (4 * y0 + Dy >= 0) & (4 * (y0 + B - 1) + Dy <= 4 * (H - 1))
            qx = np.clip(4 * (x0[:, None, None] + xx) + Dx[:, None, None], 0, q.shape[1] - 1)
            qy = np.clip(4 * (y0[:, None, None] + yy) + Dy[:, None, None], 0, q.shape[0] - 1)
            sad = np.abs(cblk - q[qy, qx].astype(np.int32)).sum(axis=(1, 2)).astype(np.int64)
            key = (sad << 40) | ((Dx * Dx + Dy * Dy) << 20) | ((Dy + bias) << 10) | (Dx + bias)
            best_key = np.where(valid & (key < best_key), key, best_key)
    bDx = (best_key & 1023) - bias
    bDy = ((best_key >> 10) & 1023) - bias
    best = np.stack([bDx, bDy, best_key >> 40], axis=1).astype(np.int32)
    return entries(best, B, W, H), best


def candidate_is_valid(x0, y0, B, W, H, Dx, Dy):
    """every sample of the block displaced by (Dx, Dy) quarter pels lies inside the frame"""
    return 4 * x0 + Dx >= 0 and 4 * (x0 + B - 1) + Dx <= 4 * (W - 1) and 4 * y0 + Dy >= 0 and 4 * (y0 + B - 1) + Dy <= 4 * (H - 1)


def refine_by_tuples(prev, cur, B, R, best_int, W=None):
    """refine() once more, slowly and without the packed 64-bit key: per block Python's min over the tuples
    (SAD, Dx*Dx + Dy*Dy, Dy, Dx) of the valid candidates (Python integers: no field can run into its neighbour).
    The 49 SADs of every block are gathered from quarter_plane(); nothing else is shared with refine().
    -> (entries, best, n_valid [nblk]: how many of the 49 candidates passed the validity rule)"""
    prev = np.asarray(prev, np.uint8); cur = np.asarray(cur, np.uint8)
    H = prev.shape[0]
    W = prev.shape[1] if W is None else W
    prev = prev[:, :W]; cur = cur[:, :W]
    nbx, nby = W // B, H // B
    n = nbx * nby
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.int32)
    q = quarter_plane(prev)
    d = np.asarray(best_int, np.int64).reshape(n, 3)
    x0 = (np.arange(n) % nbx) * B
    y0 = (np.arange(n) // nbx) * B
    cblk = cur[(y0[:, None, None] + np.arange(B)[None, :, None]), (x0[:, None, None] + np.arange(B)[None, None, :])].astype(np.int64)
    sads = {}
    for fy in range(-3, 4):
        for fx in range(-3, 4):
            # positions of an invalid candidate may leave the plane: clamp them, the candidate is dropped below
            qy = np.clip(4 * (y0[:, None, None] + np.arange(B)[None, :, None]) + (4 * d[:, 1] + fy)[:, None, None], 0, q.shape[0] - 1)
            qx = np.clip(4 * (x0[:, None, None] + np.arange(B)[None, None, :]) + (4 * d[:, 0] + fx)[:, None, None], 0, q.shape[1] - 1)
            sads[(fx, fy)] = np.abs(cblk - q[qy, qx]).sum(axis=(1, 2)).tolist()
    best = np.zeros((n, 3), np.int32)
    n_valid = np.zeros(n, np.int32)
    for k in range(n):
        cands = []
        for (fx, fy), s in sads.items():
            Dx, Dy = 4 * int(d[k, 0]) + fx, 4 * int(d[k, 1]) + fy
            if candidate_is_valid(int(x0[k]), int(y0[k]), B, W, H, Dx, Dy):
                cands.append((s[k], Dx * Dx + Dy * Dy, Dy, Dx))
        sad, _, Dy, Dx = min(cands)                                           # f = 0 is always valid: never empty
        best[k] = (Dx, Dy, sad)
        n_valid[k] = len(cands)
    return entries(best, B, W, H), best, n_valid


def entries(best, B, W, H):
    """(Dx, Dy, .) -> the decoder's records, in the kernel's f32 operation order"""
    best = np.asarray(best, np.int64)
    n = best.shape[0]
    nbx = W // B
    f = np.float32
    nx, ny = f(1.0) / f(W), f(1.0) / f(H)
    cx = (np.arange(n) % nbx) * B + B // 2
    cy = (np.arange(n) // nbx) * B + B // 2
    e = np.zeros((n, 4), np.float32)
    e[:, 0] = ((4 * cx + best[:, 0]).astype(np.float32) * f(0.25)) * nx
    e[:, 1] = ((4 * cy + best[:, 1]).astype(np.float32) * f(0.25)) * ny
    e[:, 2] = (best[:, 0].astype(np.float32) / f(4.0)) * (-nx)
    e[:, 3] = (best[:, 1].astype(np.float32) / f(4.0)) * (-ny)
    return e


def sad_flow_qpel(prev, cur, B, R, threads=1):
    """the whole CPU chain: oracle.sad_flow's integer winners, refined"""
    import oracle
    _, best = oracle.sad_flow(prev, cur, B, R, threads=threads)
    return refine(prev, cur, B, R, best)
