"""NumPy / Python restatement of N1s, hip_sad's split blocks (include/ofps_hip.h, DESIGN.md "N1s").

All-integer but for the records.  Plain loops over blocks, sub-blocks, predictors and candidates: a sub-block's candidates are the union over
its predictors -- the block's own winner, its four lattice neighbours' winners (those that exist) and zero, each clamped on its own for this
sub-block -- of the 7 x 7 windows around them, its winner is Python's min over the tuples (SAD, dx*dx + dy*dy, dy + R0 + 3, dx + R0 + 3) of
the valid candidates, and a block is split iff 16 * (SAD_parent - sum of the four sub-block SADs) >= T * B * B.  Nothing of the library
under test is imported."""
import numpy as np

E = 3                                                    # the window radius: a constant of the build
T_MAX = 4080
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # the definition's order: left, right, above, below


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def is_valid(B, R0, T):
    return B % 2 == 0 and B // 2 >= 4 and B <= 64 and 0 <= R0 and R0 + E <= 127 and 1 <= T <= T_MAX


def predictors(best, nbx, nby, bx, by, sx0, sy0, b, W, H):
    """-> the predictors of one sub-block of block (bx, by), clamped for it, in the definition's order, duplicates included"""
    lattice = [(bx, by)] + [(bx + ox, by + oy) for ox, oy in NEIGHBOURS if 0 <= bx + ox < nbx and 0 <= by + oy < nby]
    raw = [(int(best[y * nbx + x][0]), int(best[y * nbx + x][1])) for x, y in lattice] + [(0, 0)]
    return [(clamp(px, -sx0, W - b - sx0), clamp(py, -sy0, H - b - sy0)) for px, py in raw]


def sub_winner(prev, cur, sx0, sy0, b, plist, R0):
    """prev, cur int64 [H, W] -> the winner's key of the b x b sub-block at (sx0, sy0)"""
    H, W = prev.shape
    cblk = cur[sy0:sy0 + b, sx0:sx0 + b]
    cands, seen = [], set()
    for px, py in plist:
        for ey in range(-E, E + 1):
            for ex in range(-E, E + 1):
                dx, dy = px + ex, py + ey
                if (dx, dy) in seen:                     # the key is a function of d: a duplicate candidate cannot change the minimum
                    continue
                seen.add((dx, dy))
                if 0 <= sx0 + dx <= W - b and 0 <= sy0 + dy <= H - b:
                    sad = int(np.abs(cblk - prev[sy0 + dy:sy0 + dy + b, sx0 + dx:sx0 + dx + b]).sum())
                    cands.append((sad, dx * dx + dy * dy, dy + R0 + E, dx + R0 + E))
    return min(cands)                                    # d = 0 (the zero predictor's e = 0) is always valid: never empty


def record(cx, cy, dx, dy, W, H):
    """N1's record of a block centre and its vector, in the kernels' f32 operation order"""
    f = np.float32
    nx, ny = f(1.0) / f(W), f(1.0) / f(H)
    return (f(cx + dx) * nx, f(cy + dy) * ny, (f(dx) / f(1.0)) * (-nx), (f(dy) / f(1.0)) * (-ny))


def split_step(prev, cur, B, best, keep, R0, T):
    """The step alone: best [nblk, 3] the parents' (dx, dy, SAD), keep [nblk] bytes or None (all ones) ->
    dict(sub_best i32 [nblk, 4, 3], split u8 [nblk], entries f32 [nblk, 4, 4] (the raw slots), slot_flags u8 [nblk, 4],
         n_pred [nblk, 4]: distinct clamped predictors per sub-block).  Rows of blocks that are not kept are zero."""
    assert is_valid(B, R0, T)
    prev = np.asarray(prev, np.uint8).astype(np.int64); cur = np.asarray(cur, np.uint8).astype(np.int64)
    H, W = prev.shape
    nbx, nby, b = W // B, H // B, B // 2
    nblk = nbx * nby
    best = np.asarray(best, np.int64).reshape(nblk, 3)
    keep = np.ones(nblk, np.uint8) if keep is None else np.asarray(keep, np.uint8).reshape(nblk)
    sub_best = np.zeros((nblk, 4, 3), np.int32)
    split = np.zeros(nblk, np.uint8)
    entries = np.zeros((nblk, 4, 4), np.float32)
    slot_flags = np.zeros((nblk, 4), np.uint8)
    n_pred = np.zeros((nblk, 4), np.int32)
    for by in range(nby):
        for bx in range(nbx):
            k = by * nbx + bx
            if not keep[k]:
                continue
            total = 0
            for s in range(4):
                sx0, sy0 = bx * B + (s & 1) * b, by * B + (s >> 1) * b
                plist = predictors(best, nbx, nby, bx, by, sx0, sy0, b, W, H)
                key = sub_winner(prev, cur, sx0, sy0, b, plist, R0)
                sub_best[k, s] = (key[3] - R0 - E, key[2] - R0 - E, key[0])
                n_pred[k, s] = len(set(plist))
                total += key[0]
            gain = int(best[k][2]) - total
            if 16 * gain >= T * B * B:
                split[k] = 1
                slot_flags[k] = 1
                for s in range(4):
                    sx0, sy0 = bx * B + (s & 1) * b, by * B + (s >> 1) * b
                    entries[k, s] = record(sx0 + b // 2, sy0 + b // 2, int(sub_best[k, s, 0]), int(sub_best[k, s, 1]), W, H)
            else:
                slot_flags[k, 0] = 1
                entries[k, 0] = record(bx * B + B // 2, by * B + B // 2, int(best[k][0]), int(best[k][1]), W, H)
    return {"sub_best": sub_best, "split": split, "entries": entries, "slot_flags": slot_flags, "n_pred": n_pred}


def records(step):
    """the record stream: the raw slots compacted by their flags, block raster order, a split block's four in sub-block order"""
    return step["entries"].reshape(-1, 4)[step["slot_flags"].reshape(-1) != 0]
