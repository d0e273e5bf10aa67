"""NumPy restatement of N1p, the neighbour and zero predictors of hip_sad's search levels (include/ofps_hip.h, DESIGN.md "N1p").

All-integer.  A block's candidates are the union over its predictors -- twice the winners of its parent and of the parent's lattice
neighbours that exist, and zero, each clamped on its own -- of the 7 x 7 windows around them; its winner is Python's min over the tuples
(SAD, dx*dx + dy*dy, dy + R_l, dx + R_l) of the valid candidates.  Nothing of the library under test is imported; the pyramid, the reaches,
the clamp and the record arithmetic are tests/indep_sad_hier.py's, whose one-predictor refinement this file does not call."""
import numpy as np

from indep_sad_hier import REFINE, clamp, down2, entries, is_valid, oracle_top, pyramid, reaches  # noqa: F401  (re-exported for the cases)

PRED_PARENT, PRED_NEIGHBOURS = 0, 1
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # the definition's order: left, right, above, below


def predictors(parent_best, pnbx, pnby, bx, by, x0, y0, B, W, H, mode):
    """-> the clamped predictors of block (bx, by) in the definition's order, duplicates included"""
    qx, qy = min(bx >> 1, pnbx - 1), min(by >> 1, pnby - 1)
    lattice = [(qx, qy)]
    if mode == PRED_NEIGHBOURS:
        lattice += [(qx + ox, qy + oy) for ox, oy in NEIGHBOURS if 0 <= qx + ox < pnbx and 0 <= qy + oy < pnby]
    raw = [(2 * int(parent_best[y * pnbx + x][0]), 2 * int(parent_best[y * pnbx + x][1])) for x, y in lattice]
    if mode == PRED_NEIGHBOURS:
        raw.append((0, 0))
    return [(clamp(px, -x0, W - B - x0), clamp(py, -y0, H - B - y0)) for px, py in raw]


def refine(prev, cur, B, parent_best, pnbx, pnby, R_l, mode):
    """one refinement step -> (best [nblk, 3] i32, keys: the winner's key per block, n_pred [nblk]: distinct clamped predictors)"""
    assert mode in (PRED_PARENT, PRED_NEIGHBOURS)
    prev = np.asarray(prev, np.uint8).astype(np.int64); cur = np.asarray(cur, np.uint8).astype(np.int64)
    H, W = prev.shape
    nbx, nby = W // B, H // B
    parent_best = np.asarray(parent_best, np.int64).reshape(pnbx * pnby, 3)
    best = np.zeros((nbx * nby, 3), np.int32)
    keys = []
    n_pred = np.zeros(nbx * nby, np.int32)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = bx * B, by * B
            cblk = cur[y0:y0 + B, x0:x0 + B]
            plist = predictors(parent_best, pnbx, pnby, bx, by, x0, y0, B, W, H, mode)
            cands, seen = [], set()
            for px, py in plist:
                for ey in range(-REFINE, REFINE + 1):
                    for ex in range(-REFINE, REFINE + 1):
                        dx, dy = px + ex, py + ey
                        if (dx, dy) in seen:             # the key is a function of d: a duplicate candidate cannot change the minimum
                            continue
                        seen.add((dx, dy))
                        if 0 <= x0 + dx <= W - B and 0 <= y0 + dy <= H - B:
                            sad = int(np.abs(cblk - prev[y0 + dy:y0 + dy + B, x0 + dx:x0 + dx + B]).sum())
                            cands.append((sad, dx * dx + dy * dy, dy + R_l, dx + R_l))
            key = min(cands)                             # e = 0 of every predictor is valid: never empty
            best[by * nbx + bx] = (key[3] - R_l, key[2] - R_l, key[0])
            keys.append(key)
            n_pred[by * nbx + bx] = len(set(plist))
    return best, keys, n_pred


def search(prev, cur, B, R, levels, mode, top=oracle_top):
    """the whole definition -> (entries [nblk, 4] f32, best [nblk, 3] i32, [best of level 0, ..., best of the top level], level-0 keys)"""
    prev = np.asarray(prev, np.uint8); cur = np.asarray(cur, np.uint8)
    H, W = prev.shape
    assert is_valid(W, H, B, R, levels)
    pp, pc = pyramid(prev, levels), pyramid(cur, levels)
    rl = reaches(R, levels)
    per_level = [None] * levels
    per_level[levels - 1] = np.asarray(top(pp[-1], pc[-1], B, R), np.int32)
    keys = None
    for l in range(levels - 2, -1, -1):
        ph, pw = pp[l + 1].shape
        per_level[l], keys, _ = refine(pp[l], pc[l], B, per_level[l + 1], pw // B, ph // B, rl[l], mode)
    return entries(per_level[0], B, W, H), per_level[0], per_level, keys
