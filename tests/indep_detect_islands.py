"""A plain-Python restatement of the island list (include/ofps_hip.h A5i) -- written from the definition, not from the kernel: no labels
are propagated, nothing is sorted by a network.  The densified field comes from the C oracle (oracle.densify, what the detector reads), the
lit map from numpy f32, the components from a flood fill in raster order with an explicit stack.  Test infrastructure only."""
from collections import namedtuple

import numpy as np

import oracle

F = np.float32
NOT_LISTED = 0xFFFF
MAX_ISLANDS = 6400

Islands = namedtuple("Islands", "dim n_islands n_components table root field")
# table: int32 [n_islands, 8], every qualifying component in rank order (seed, area, x0, y0, x1, y1, sum_x, sum_y)
# root:  int32 [dim, dim], the seed of the cell's component, -1 where the cell is not lit
# field: f32 [dim, dim, 2], the densified field


def lit_map(field, target_motion):
    x, y = field[..., 0].astype(F), field[..., 1].astype(F)
    xx, yy = (x * x).astype(F), (y * y).astype(F)                       # both products rounded before the sum: no contraction
    with np.errstate(invalid="ignore"):
        return np.sqrt((xx + yy).astype(F)).astype(F) >= F(target_motion)


def components(lit):
    """-> (root [d, d] int32, [(seed, cells [(x, y), ...]), ...] in seed order): 8-connected flood fill in raster order"""
    d = lit.shape[0]
    root = np.full((d, d), -1, np.int32)
    lit = lit.tolist()
    seen = [[False] * d for _ in range(d)]
    comps = []
    for y in range(d):
        for x in range(d):
            if not lit[y][x] or seen[y][x]:
                continue
            seed = y * d + x
            seen[y][x] = True
            stack, cells = [(x, y)], []
            while stack:
                cx, cy = stack.pop()
                cells.append((cx, cy))
                for ny in range(max(cy - 1, 0), min(cy + 2, d)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, d)):
                        if lit[ny][nx] and not seen[ny][nx]:
                            seen[ny][nx] = True
                            stack.append((nx, ny))
            for cx, cy in cells:
                root[cy, cx] = seed
            comps.append((seed, cells))
    return root, comps


def islands(entries, min_size, subdivide, target_motion):
    """every qualifying component, ranked: area descending, then seed ascending"""
    d = oracle.block_dim(min_size, subdivide)
    field = np.ascontiguousarray(oracle.densify(np.ascontiguousarray(entries, F).reshape(-1, 4), d, d), F).reshape(d, d, 2)
    root, comps = components(lit_map(field, target_motion))
    cells = d * d
    rows = []
    for seed, cs in comps:
        area = len(cs)
        if not (F(area) / F(cells) >= F(min_size)):
            continue
        xs, ys = [c[0] for c in cs], [c[1] for c in cs]
        rows.append((seed, area, min(xs), min(ys), max(xs), max(ys), sum(xs), sum(ys)))
    rows.sort(key=lambda r: (-r[1], r[0]))
    table = np.array(rows, np.int32).reshape(-1, 8)
    for a in (root, field, table):
        a.setflags(write=False)
    return Islands(d, len(rows), len(comps), table, root, field)


def listed(isl, K):
    """what max_islands = K hands out -> (counts [4], table [n_listed, 8], labels u16 [d, d], field f32 [d, d, 2])"""
    assert 1 <= K <= MAX_ISLANDS
    d = isl.dim
    n_listed = min(isl.n_islands, K)
    rank = np.full(d * d + 1, NOT_LISTED, np.int64)                      # by seed; the last entry answers for "not lit"
    rank[isl.table[:n_listed, 0]] = np.arange(n_listed)
    labels = rank[isl.root].astype(np.uint16)                            # root -1 -> the last entry
    own_seed = isl.root == np.arange(d * d, dtype=np.int32).reshape(d, d)
    copied = (labels != NOT_LISTED) & ~own_seed
    field = np.where(copied[..., None], isl.field, F(0)).astype(F)
    counts = np.array([isl.n_islands, isl.n_components, d, n_listed], np.int32)
    return counts, isl.table[:n_listed], labels, field
