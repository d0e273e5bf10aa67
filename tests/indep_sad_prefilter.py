"""hip_sad's mean removal (include/ofps_hip.h N1m) restated in NumPy, and N1's full search beside it so that a search on the filtered pair
can be stated without the library or the CPU oracle.  Imports nothing from the project: integers only, the definition's words in order."""
import numpy as np

MAX_RADIUS = 16


def multiplier(r):
    """M = ceil(2^32 / n) of the kernel's division (the definition itself divides)"""
    n = (2 * r + 1) ** 2
    return ((1 << 32) + n - 1) // n


def prefilter(img, r):
    """F = clamp(v - m + 128, 0, 255), m = (S + (n >> 1)) // n, S = the (2r + 1)^2 box sum with a replicated border.
    Padded integral image in Python integers (object arrays): no width to overflow."""
    v = np.asarray(img, np.uint8)
    assert v.ndim == 2 and 1 <= r <= MAX_RADIUS
    H, W = v.shape
    k = 2 * r + 1
    n = k * k
    pad = np.pad(v, r, mode="edge").astype(object)                       # (H + 2r) x (W + 2r)
    I = np.zeros((H + 2 * r + 1, W + 2 * r + 1), object)
    I[1:, 1:] = pad.cumsum(axis=0).cumsum(axis=1)
    S = I[k:, k:] - I[:-k, k:] - I[k:, :-k] + I[:-k, :-k]                # H x W
    m = (S + (n >> 1)) // n
    F = v.astype(object) - m + 128
    return np.clip(F.astype(np.int64), 0, 255).astype(np.uint8)


def prefilter_loops(img, r):
    """the same, pixel by pixel with clamped coordinates (the check of the integral image; small frames only)"""
    v = np.asarray(img, np.uint8)
    H, W = v.shape
    n = (2 * r + 1) ** 2
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            S = 0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    S += int(v[min(max(y + j, 0), H - 1), min(max(x + i, 0), W - 1)])
            m = (S + (n >> 1)) // n
            out[y, x] = min(max(int(v[y, x]) - m + 128, 0), 255)
    return out


def full_search(prev, cur, B, R):
    """N1: per lattice block the candidate d in [-R, R]^2 whose block lies inside the frame with the least
    (SAD, dx*dx + dy*dy, dy + R, dx + R) -> int32 [nblk, 3] (dx, dy, SAD), raster order.  The block of cur at (x0, y0) against prev at (x0 + dx, y0 + dy)."""
    prev = np.asarray(prev, np.uint8).astype(np.int64); cur = np.asarray(cur, np.uint8).astype(np.int64)
    H, W = prev.shape
    nbx, nby = W // B, H // B
    x0 = np.arange(nbx) * B; y0 = np.arange(nby) * B
    pp = np.pad(prev, R, mode="edge")                                   # only valid candidates are ever compared
    c = cur[:nby * B, :nbx * B]
    best_key = np.full((nby, nbx), np.iinfo(np.int64).max, np.int64)
    best = np.zeros((nby, nbx, 3), np.int32)
    for dy in range(-R, R + 1):
        vy = (y0 + dy >= 0) & (y0 + dy + B <= H)
        for dx in range(-R, R + 1):
            vx = (x0 + dx >= 0) & (x0 + dx + B <= W)
            ref = pp[R + dy:R + dy + nby * B, R + dx:R + dx + nbx * B]
            sad = np.abs(c - ref).reshape(nby, B, nbx, B).sum(axis=(1, 3))
            key = ((sad * 16384 + (dx * dx + dy * dy)) * 256 + (dy + R)) * 256 + (dx + R)
            take = vy[:, None] & vx[None, :] & (key < best_key)
            best_key = np.where(take, key, best_key)
            best[take] = np.stack([np.full_like(sad, dx), np.full_like(sad, dy), sad], axis=-1)[take]
    return best.reshape(-1, 3)


def entries(best, B, W, H):
    """(dx, dy, .) -> N1's records: pos = (block centre + d) / (W, H), motion = -d / (W, H), in the kernels' f32 operation order"""
    best = np.asarray(best, np.int64)
    n = best.shape[0]
    nbx = max(W // B, 1)
    f = np.float32
    nx, ny = f(1.0) / f(W), f(1.0) / f(H)
    e = np.zeros((n, 4), np.float32)
    e[:, 0] = ((np.arange(n) % nbx) * B + B // 2 + best[:, 0]).astype(np.float32) * nx
    e[:, 1] = ((np.arange(n) // nbx) * B + B // 2 + best[:, 1]).astype(np.float32) * ny
    e[:, 2] = best[:, 0].astype(np.float32) * (-nx)
    e[:, 3] = best[:, 1].astype(np.float32) * (-ny)
    return e


def search(prev, cur, B, R, r):
    """the plain search of a context with sad_prefilter = r (0 = off) -> (entries, best)"""
    if r:
        prev, cur = prefilter(prev, r), prefilter(cur, r)
    H, W = np.asarray(prev).shape
    best = full_search(prev, cur, B, R)
    return entries(best, B, W, H), best
