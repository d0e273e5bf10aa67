"""NumPy restatement of N1h, hip_sad's search levels (include/ofps_hip.h, DESIGN.md "N1h").

All-integer.  Every block's winner is Python's min over the tuples (SAD, dx*dx + dy*dy, dy + R_l, dx + R_l) of its valid candidates (Python
integers: no field can run into its neighbour).  Nothing of the library under test is imported; the top search is the CPU oracle's plain
search unless the caller brings another."""
import numpy as np

REFINE = 3                                               # the refinement radius: a constant of the build
MAX_REACH = 127


def down2(img):
    """[H, W] u8 -> [H >> 1, W >> 1] u8: (a + b + c + d + 2) >> 2 of every 2 x 2 quad; a last odd column or row is unused"""
    a = np.asarray(img, np.uint8).astype(np.int64)
    Ho, Wo = a.shape[0] >> 1, a.shape[1] >> 1
    a = a[:2 * Ho, :2 * Wo]
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(img, levels):
    """-> [level 0 = the frame, ..., level levels - 1]"""
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        out.append(down2(out[-1]))
    return out


def reach(R, levels):
    """R_0 of a search of range R over `levels` levels, or None when the pair is invalid"""
    if not (0 <= R <= 64 and 1 <= levels <= 3):
        return None
    for _ in range(1, levels):
        R = 2 * R + REFINE
    return R if R <= MAX_REACH else None


def reaches(R, levels):
    """-> [R_0, ..., R_{levels - 1} = R]"""
    out = [R]
    for _ in range(1, levels):
        out.insert(0, 2 * out[0] + REFINE)
    return out


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def predictor(parent_best, pnbx, pnby, bx, by, x0, y0, B, W, H):
    """twice the parent's winner, clamped so that the block lies inside the frame"""
    pb = parent_best[min(by >> 1, pnby - 1) * pnbx + min(bx >> 1, pnbx - 1)]
    return clamp(2 * int(pb[0]), -x0, W - B - x0), clamp(2 * int(pb[1]), -y0, H - B - y0)


def refine(prev, cur, B, parent_best, pnbx, pnby, R_l):
    """one refinement step on the lattice of (prev, cur): parent_best [pnbx * pnby, 3] (dx, dy, sad) of the coarser lattice
    -> (best [nblk, 3] i32, n_valid [nblk]: how many of the 49 candidates were valid)"""
    prev = np.asarray(prev, np.uint8).astype(np.int64); cur = np.asarray(cur, np.uint8).astype(np.int64)
    H, W = prev.shape
    nbx, nby = W // B, H // B
    parent_best = np.asarray(parent_best, np.int64).reshape(pnbx * pnby, 3)
    best = np.zeros((nbx * nby, 3), np.int32)
    n_valid = np.zeros(nbx * nby, np.int32)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = bx * B, by * B
            px, py = predictor(parent_best, pnbx, pnby, bx, by, x0, y0, B, W, H)
            cblk = cur[y0:y0 + B, x0:x0 + B]
            cands = []
            for ey in range(-REFINE, REFINE + 1):
                for ex in range(-REFINE, REFINE + 1):
                    dx, dy = px + ex, py + ey
                    if 0 <= x0 + dx <= W - B and 0 <= y0 + dy <= H - B:
                        sad = int(np.abs(cblk - prev[y0 + dy:y0 + dy + B, x0 + dx:x0 + dx + B]).sum())
                        cands.append((sad, dx * dx + dy * dy, dy + R_l, dx + R_l))
            sad, _, ky, kx = min(cands)                  # e = 0 is always valid: never empty
            best[by * nbx + bx] = (kx - R_l, ky - R_l, sad)
            n_valid[by * nbx + bx] = len(cands)
    return best, n_valid


def entries(best, B, W, H):
    """(dx, dy, .) -> the decoder's records in N1's convention, in the kernels' f32 operation order"""
    best = np.asarray(best, np.int64)
    n = best.shape[0]
    nbx = max(W // B, 1)
    f = np.float32
    nx, ny = f(1.0) / f(W), f(1.0) / f(H)
    cx = (np.arange(n) % nbx) * B + B // 2 + best[:, 0]
    cy = (np.arange(n) // nbx) * B + B // 2 + best[:, 1]
    e = np.zeros((n, 4), np.float32)
    e[:, 0] = cx.astype(np.float32) * nx
    e[:, 1] = cy.astype(np.float32) * ny
    e[:, 2] = (best[:, 0].astype(np.float32) / f(1.0)) * (-nx)
    e[:, 3] = (best[:, 1].astype(np.float32) / f(1.0)) * (-ny)
    return e


def oracle_top(prev, cur, B, R):
    import oracle
    return oracle.sad_flow(prev, cur, B, R)[1]


def is_valid(W, H, B, R, levels):
    return reach(R, levels) is not None and (W >> (levels - 1)) >= B and (H >> (levels - 1)) >= B


def search(prev, cur, B, R, levels, top=oracle_top):
    """the whole definition -> (entries [nblk, 4] f32, best [nblk, 3] i32, [best of level 0, ..., best of the top level])"""
    prev = np.asarray(prev, np.uint8); cur = np.asarray(cur, np.uint8)
    H, W = prev.shape
    assert is_valid(W, H, B, R, levels)
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    rl = reaches(R, levels)
    per_level = [None] * levels
    per_level[levels - 1] = np.asarray(top(pp[-1], pc[-1], B, R), np.int32)
    for l in range(levels - 2, -1, -1):
        ph, pw = pp[l + 1].shape
        per_level[l], _ = refine(pp[l], pc[l], B, per_level[l + 1], pw // B, ph // B, rl[l])
    return entries(per_level[0], B, W, H), per_level[0], per_level
