"""Case lists for the block-motion detector (ofps_amd/csrc/detect.hip, fed by densify.hip) over its whole grid and parameter domain.
CPU only: numpy and the two oracles -- never the library under test.  tests/test_detect_cases_cpu.py proves that every case has the
property it is named for (so that no GPU test passes vacuously) and pins the literals below; tests/test_detect_domain_gpu.py runs them.

The detector (block-motion-detector/src/lib.rs:49-118): dim = ceil(subdivide / sqrt(min_size)) cells per side; a cell is on when
|mean motion| >= target_motion; the largest 8-connected island wins (the earliest in raster order among equals); the answer is Some when
area / dim^2 >= min_size, and the island's first cell in raster order (its seed) is never copied into the returned field.

Every expectation downstream is bit equality: areas and membership are integers, the field is a copy."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle
from oracle import np_oracle

F = np.float32
TARGET = 0.003                    # the plugin's default target_motion
MOVE = (0.01, 0.0)                # a lit cell's motion: well above TARGET
STRONG = (0.02, 0.01)             # ... where one cell of the case sits at the threshold itself

# ---- the grid: (min_size, subdivide) inside the property ranges (plugins.py: 0.01..1, 1..16) -> cells per side ---------------------------
# sides where the code changes behaviour: 16 | 17 (256 cells: one-workgroup densifier and one-pass sort | two-pass sort), 32 | 33 (1,024
# cells: one cell per detector thread | a second trip of every strided loop), 90 | 91 (dynamic LDS 48,600 B | 49,696 B: the 48 KiB
# attribute), 1 and 2 (w - 1 == 0; a grid smaller than the 3 x 3 neighbourhood).  129 and 159 exist only off the 0.001 raster.
GRID = ((1.0, 1), (0.25, 1), (0.112, 1), (0.063, 1), (0.05, 2), (0.05, 3), (0.04, 3), (0.0625, 4), (0.014, 2), (0.017, 4), (0.016, 4),
        (0.015, 4), (0.021, 9), (0.012, 7), (0.024, 10), (0.01, 9), (0.024, 14), (0.014, 15), (0.012, 14), (0.010156, 13), (0.010127, 16),
        (0.01, 16))
GRID_SIDES = (1, 2, 3, 4, 9, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 90, 91, 127, 128, 129, 159, 160)
PAIR = dict(zip(GRID_SIDES, GRID))
REQUIRED_SIDES = (1, 2, 3, 4, 9, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 90, 91, 127, 128, 160)
SIDE_161 = (0.009877, 16)         # just under the property range: the first side the library refuses


def params(pair, target_motion=TARGET):
    return dict(min_size=pair[0], subdivide=pair[1], target_motion=target_motion)


# ---- entries that light chosen cells exactly ----------------------------------------------------------------------------------------------
def positions(dim):
    """one coordinate per cell index: x / (dim - 1) clamped into (0, 1) -- the densifier's all-component clamp sends 0, 1 and everything
    outside to a corner (motion_field.rs:164-178).  On a one-cell grid every position lands in cell 0."""
    if dim == 1:
        return np.array([0.5], F)
    return np.clip(np.arange(dim, dtype=F) / F(dim - 1), F(1e-4), F(1 - 1e-4)).astype(F)


def entries(dim, on, motion=MOVE, background=True, counts=None, motions=None):
    """-> [n, 4] f32 records (x, y, mx, my).  on: the lit cells [(x, y), ...], in the order their records are emitted.  motion: every lit
    record's motion, unless motions gives one (mx, my) per lit cell or one [c, 2] array per lit cell (its c records, in order).  counts: records
    per lit cell (an int or one per cell; default 1).  background: one still record in every cell that is not lit, after the lit ones."""
    on = [tuple(c) for c in on]
    p = positions(dim)
    rows = []
    for k, (x, y) in enumerate(on):
        if motions is not None:
            m = np.asarray(motions[k], F).reshape(-1, 2)
        else:
            m = np.asarray(motion, F).reshape(1, 2)
        c = m.shape[0] if m.shape[0] > 1 else (1 if counts is None else int(counts if np.isscalar(counts) else counts[k]))
        m = np.broadcast_to(m, (c, 2))
        r = np.empty((c, 4), F)
        r[:, 0], r[:, 1], r[:, 2:] = p[x], p[y], m
        rows.append(r)
    if background:
        lit = np.zeros((dim, dim), bool)
        for x, y in on:
            lit[y, x] = True
        ys, xs = np.nonzero(~lit)
        r = np.zeros((len(xs), 4), F)
        r[:, 0], r[:, 1] = p[xs], p[ys]
        rows.append(r)
    return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), F), dtype=F)


# ---- shapes: on-cell sets for a side -----------------------------------------------------------------------------------------------------
def antidiagonal(d):
    return [(d - 1 - i, i) for i in range(d)]


def diagonal(d):
    return [(i, i) for i in range(d)]


def _rect(x0, y0, w, h):
    return [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]


def corner_blobs(d, anti=False):
    """two a x a blobs that share one corner point and nothing else: 4-connected they are two islands"""
    a = min(d // 2, 3)
    return (_rect(a, 0, a, a) + _rect(0, a, a, a)) if anti else (_rect(0, 0, a, a) + _rect(a, a, a, a))


def corner_blobs_anti(d):
    return corner_blobs(d, True)


def serpentine(d):
    """full even rows joined by one cell at alternating ends of the odd rows: one island whose path is as long as the grid allows"""
    out = []
    for y in range(d):
        out += _rect(0, y, d, 1) if y % 2 == 0 else [(d - 1 if (y // 2) % 2 == 0 else 0, y)]
    return out


def last_first(d):
    """a ring opened at the top-left: column 0 down, the last row, the last column up, row 0 back to x = 2.  Cell 0 joins cells 2 .. d - 2
    only through the far corner, so the winning label travels AGAINST raster order through the whole island."""
    assert d >= 4
    return ([(0, y) for y in range(d)] + [(x, d - 1) for x in range(1, d)] + [(d - 1, y) for y in range(d - 2, -1, -1)] +
            [(x, 0) for x in range(d - 2, 1, -1)])


@lru_cache(maxsize=None)
def _spiral_pair(d):
    """two square spirals wound into each other, one the point reflection of the other (so of equal area), one free cell between
    neighbouring arms (an arm of the same spiral every 4 cells): walked from (0, 0) clockwise, a step is taken while the next cell touches
    nothing but the walker's own last two cells"""
    def refl(c):
        return (d - 1 - c[0], d - 1 - c[1])
    a = [(0, 0)]
    taken = {a[0], refl(a[0])}
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    k = 0
    while True:
        for turn in (0, 1):
            dx, dy = dirs[(k + turn) % 4]
            n = (a[-1][0] + dx, a[-1][1] + dy)
            if not (0 <= n[0] < d and 0 <= n[1] < d):
                continue
            near = {(n[0] + ox, n[1] + oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1)}
            if (near & taken) - set(a[-2:]) or refl(n) in near:
                continue
            a.append(n); taken.add(n); taken.add(refl(n))
            k = (k + turn) % 4
            break
        else:
            break
    return tuple(a), tuple(refl(c) for c in a)


def spirals(d):
    a, b = _spiral_pair(d)
    return list(a) + list(b)


def spirals_extra(d):
    """the same pair with one more cell on the later spiral (the one that does not hold cell 0): the last free cell in raster order that
    touches it and not the other one"""
    a, b = _spiral_pair(d)
    sa, sb = set(a), set(b)

    def touches(c, s):
        return any((c[0] + ox, c[1] + oy) in s for ox in (-1, 0, 1) for oy in (-1, 0, 1))
    for i in range(d * d - 1, -1, -1):
        c = (i % d, i // d)
        if c not in sa and c not in sb and touches(c, sb) and not touches(c, sa):
            return list(a) + list(b) + [c]
    raise AssertionError("no free cell next to the later spiral")


def lattice(d):
    """isolated cells (2i, 2j): (ceil(d / 2))^2 islands of area 1; cell 0 wins, and as the seed it is not copied"""
    return [(x, y) for y in range(0, d, 2) for x in range(0, d, 2)]


def block_lattice(d):
    """the same lattice of isolated 16 x 16 blocks: every other 16-cell tile in both directions"""
    out = []
    for y0 in range(0, d - 15, 32):
        for x0 in range(0, d - 15, 32):
            out += _rect(x0, y0, 16, 16)
    return out


def all_on(d):
    return _rect(0, 0, d, d)


def nothing(d):
    return []


def one_cell(d):
    return [(d // 2, d // 2)]


K1024_HALF = {33: 2, 64: 4, 65: 5, 160: 8}


def k1024_blocks(d):
    """one clipped (2 hw + 1)^2 block around every cell whose index is a multiple of 1,024: islands that lie across a detector thread's
    second, third, ... cell.  The middle one has one more column, so the winner is neither the first nor the last."""
    hw, K = K1024_HALF[d], (d * d - 1) // 1024
    out = []
    for k in range(1, K + 1):
        cx, cy = (1024 * k) % d, (1024 * k) // d
        x1 = cx + hw + (1 if k == K // 2 + 1 else 0)
        out += [(x, y) for y in range(max(cy - hw, 0), min(cy + hw, d - 1) + 1) for x in range(max(cx - hw, 0), min(x1, d - 1) + 1)]
    return out


def far_edge_lines(d):
    """a vertical line in the last column (rows 0 .. d - 4) and a longer horizontal line in the last row (columns 0 .. d - 3): the neighbour
    clipping at the far edges; the winner lies in the last row"""
    return [(d - 1, y) for y in range(d - 3)] + [(x, d - 1) for x in range(d - 2)]


def first_cells(d, a):
    """the first `a` cells in raster order of the smallest square block that holds them"""
    s = int(np.ceil(np.sqrt(a))) if a else 0
    return _rect(0, 0, s, s)[:a]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
# name; cells per side; the detector's parameters; make() -> records; some: the Some / None outcome; area: the winning island's area (also
# when the outcome is None: 0 only when no cell is on); seed: the winner's first cell in raster order (None when no cell is on)
Case = namedtuple("Case", "name side params make some area seed")


def _side(pair):
    return oracle.block_dim(*pair)


def _shape_case(shape, pair, area, some, seed, tag=None):
    d = _side(pair)
    return Case(f"{tag or shape.__name__}-{d}", d, params(pair), lru_cache(maxsize=1)(lambda: entries(d, shape(d))), some, area, seed)


P = PAIR
# (shape, (min_size, subdivide), area as a literal, Some?, seed cell)
SHAPES = tuple(_shape_case(*s) for s in (
    # one cell thick: min_size 0.01 and subdivide <= 10 give a side of 10 * subdivide, whose diagonal reaches the minimum area subdivide^2
    (antidiagonal, P[2], 2, True, 1), (antidiagonal, (0.01, 1), 10, True, 9), (antidiagonal, P[14], 14, True, 13),
    (antidiagonal, P[33], 33, True, 32), (antidiagonal, (0.01, 10), 100, True, 99), (antidiagonal, P[160], 160, False, 159),
    (diagonal, (0.01, 1), 10, True, 0), (diagonal, P[17], 17, True, 0), (diagonal, (0.01, 10), 100, True, 0), (diagonal, P[160], 160, False, 0),
    (corner_blobs, P[4], 2 * 2 * 2, True, 0), (corner_blobs, P[14], 2 * 3 * 3, True, 0), (corner_blobs, P[65], 2 * 3 * 3, False, 0),
    (corner_blobs_anti, P[4], 2 * 2 * 2, True, 2), (corner_blobs_anti, P[14], 2 * 3 * 3, True, 3), (corner_blobs_anti, P[17], 2 * 3 * 3, True, 3),
    (corner_blobs_anti, P[65], 2 * 3 * 3, False, 3),
    # ceil(d / 2) full rows and floor(d / 2) joints
    (serpentine, P[3], 2 * 3 + 1, True, 0), (serpentine, P[16], 8 * 16 + 8, True, 0), (serpentine, P[17], 9 * 17 + 8, True, 0),
    (serpentine, P[33], 17 * 33 + 16, True, 0), (serpentine, P[90], 45 * 90 + 45, True, 0), (serpentine, P[91], 46 * 91 + 45, True, 0),
    (serpentine, P[160], 80 * 160 + 80, True, 0),
    # 4 d - 5 cells
    (last_first, P[4], 4 * 4 - 5, True, 0), (last_first, P[16], 4 * 16 - 5, True, 0), (last_first, P[33], 4 * 33 - 5, True, 0),
    (last_first, P[65], 4 * 65 - 5, True, 0), (last_first, P[128], 4 * 128 - 5, True, 0), (last_first, P[160], 4 * 160 - 5, True, 0),
    # two spirals of equal area: the earlier seed (cell 0) wins; with one more cell the later one (seed (0, 2)) does
    (spirals, P[17], 80, True, 0), (spirals, P[33], 288, True, 0), (spirals, P[64], 1055, True, 0), (spirals, P[160], 6479, True, 0),
    (spirals_extra, P[17], 81, True, 2 * 17), (spirals_extra, P[33], 289, True, 2 * 33), (spirals_extra, P[64], 1056, True, 2 * 64),
    (spirals_extra, P[160], 6480, True, 2 * 160),
    # area-1 islands survive only with subdivide = 1 (1 / 100 >= 0.01); the returned field is then all zero
    (lattice, (0.01, 1), 1, True, 0), (lattice, P[9], 1, False, 0), (lattice, P[128], 1, False, 0), (lattice, P[160], 1, False, 0),
    (block_lattice, P[160], 16 * 16, True, 0),
    (all_on, P[2], 2 * 2, True, 0), (all_on, P[3], 3 * 3, True, 0), (all_on, P[16], 16 * 16, True, 0), (all_on, P[17], 17 * 17, True, 0),
    (all_on, P[32], 32 * 32, True, 0), (all_on, P[33], 33 * 33, True, 0), (all_on, P[90], 90 * 90, True, 0), (all_on, P[91], 91 * 91, True, 0),
    (all_on, P[160], 160 * 160, True, 0),
    (nothing, P[3], 0, False, None), (nothing, P[17], 0, False, None), (nothing, P[160], 0, False, None),
    (one_cell, P[2], 1, True, 3), (one_cell, (0.01, 1), 1, True, 55), (one_cell, P[14], 1, False, 7 * 14 + 7), (one_cell, P[129], 1, False, 64 * 129 + 64),
    # side 1: w - 1 == 0, every record lands in cell 0
    (one_cell, P[1], 1, True, 0, "side"),
    # (2 hw + 1)^2 and one more column; at side 33 and 64 the blocks are clipped by the left and the last row
    (k1024_blocks, P[33], 4 * 4 + 4, True, 29 * 33), (k1024_blocks, P[64], 5 * 9 + 9, True, 28 * 64), (k1024_blocks, P[65], 11 * 11 + 11, True, 42 * 65 + 12),
    (k1024_blocks, P[160], 17 * 17 + 17, True, 75 * 160 + 24),
    # d - 2 cells in the last row
    (far_edge_lines, P[33], 33 - 2, True, 32 * 33), (far_edge_lines, P[64], 64 - 2, True, 63 * 64), (far_edge_lines, P[65], 65 - 2, False, 64 * 65),
    (far_edge_lines, P[159], 159 - 2, False, 158 * 159), (far_edge_lines, P[160], 160 - 2, False, 159 * 160),
))

# ---- area / cells == min_size exactly in f32: the shape of exactly that area is Some, one cell less is None ------------------------------
AREA_EQUALITY_PAIRS = ((1.0, 1, 1), (0.25, 2, 4), (0.25, 16, 256), (0.0625, 4, 16), (0.0625, 16, 256), (0.04, 2, 4), (0.01, 1, 1), (0.01, 16, 256))


def _equality_case(m, s, a, some):
    d = _side((m, s))
    n = a if some else a - 1
    return Case(f"equal-{m}-{s}-{'some' if some else 'none'}", d, params((m, s)), lru_cache(maxsize=1)(lambda: entries(d, first_cells(d, n))), some,
                n, 0 if n else None)


AREA_EQUALITY = tuple(_equality_case(m, s, a, some) for m, s, a in AREA_EQUALITY_PAIRS for some in (True, False))


# ---- |m| == target_motion: a bridge cell between a smaller earlier blob and a larger later one -------------------------------------------
BRIDGE_GEOMETRY = {3: (1, 1), 14: (3, 4), 17: (3, 3), 33: (4, 5), 160: (16, 16)}          # side -> (blob width, height of the earlier blob)


def bridge_shape(d):
    """-> (left, bridge, right): left wl x hh at the origin, right wl x (hh + 1) one free column further, the bridge cell (wl, 0) between.
    Bridge on: one island of 2 wl hh + wl + 1 cells from seed 0; bridge off: the right blob wins, wl (hh + 1) cells from seed wl + 1"""
    wl, hh = BRIDGE_GEOMETRY[d]
    return _rect(0, 0, wl, hh), (wl, 0), _rect(wl + 1, 0, wl, hh + 1)


def mag_separate(m):
    """|m| as the detector must compute it: both products rounded to f32 before the sum (no contraction)"""
    m = np.asarray(m, F)
    xx = (m[..., 0] * m[..., 0]).astype(F); yy = (m[..., 1] * m[..., 1]).astype(F)
    return np.sqrt((xx + yy).astype(F)).astype(F)


def mag_fused(m):
    """the two forms a contracting compiler can give x * x + y * y: fma(x, x, y * y) and fma(y, y, x * x)"""
    m = np.asarray(m, F)
    xx = (m[..., 0] * m[..., 0]).astype(F); yy = (m[..., 1] * m[..., 1]).astype(F)
    return (np.sqrt(np_oracle.fma32(m[..., 0], m[..., 0], yy)).astype(F), np.sqrt(np_oracle.fma32(m[..., 1], m[..., 1], xx)).astype(F))


def bridge_entries(d, bridge_motions, hole=None, left_motions=None):
    """the bridge shape with STRONG motion everywhere but the bridge cell, which gets bridge_motions [c, 2]; hole: (cell of the right blob,
    its motions); left_motions: motions of the left blob's cell (0, 1)"""
    left, br, right = bridge_shape(d)
    on = left + [br] + right
    motions = [np.asarray(STRONG, F)] * len(on)
    motions[len(left)] = np.asarray(bridge_motions, F).reshape(-1, 2)
    if hole is not None:
        motions[on.index(hole[0])] = np.asarray(hole[1], F).reshape(-1, 2)
    if left_motions is not None:
        motions[on.index((0, 1))] = np.asarray(left_motions, F).reshape(-1, 2)
    return entries(d, on, motions=motions)


def bridge_value(d, e):
    """the bridge cell's densified value, read from the C oracle"""
    wl = BRIDGE_GEOMETRY[d][0]
    return oracle.densify(e, d, d)[0, wl].copy()


def _bridge_areas(d):
    wl, hh = BRIDGE_GEOMETRY[d]
    return 2 * wl * hh + wl + 1, wl * (hh + 1), wl + 1


def _three_motions(d):
    return np.random.default_rng(290 + d).uniform(0.003, 0.006, (3, 2)).astype(F)            # three records: the mean is no round number


@lru_cache(maxsize=None)
def _contraction_motions():
    """seeded search: one-record cells whose mean's magnitude differs by an ulp between the separately rounded and BOTH fused evaluations
    -> ([k, 2] motions with fused > separate, [k, 2] with fused < separate)"""
    v = np.random.default_rng(29).uniform(0.002, 0.02, (4096, 2)).astype(F)
    mean = (v / (np_oracle.EPSILON + F(1.0))).astype(F)                                      # one record: sum = v, count = eps + 1
    sep, (fa, fb) = mag_separate(mean), mag_fused(mean)
    up = v[(fa > sep) & (fb > sep) & (fa == fb)]
    down = v[(fa < sep) & (fb < sep) & (fa == fb)]
    assert len(up) >= 2 and len(down) >= 2
    return up[:2], down[:2]


def _edge_case(name, d, make, target_of, on):
    """target_of(value of the bridge cell) -> target_motion; on: is the bridge cell on under it?"""
    e = make()
    t = float(target_of(bridge_value(d, e)))
    joined, split, seed_split = _bridge_areas(d)
    return Case(name, d, params(PAIR[d], t), lambda: e, True, joined if on else split, 0 if on else seed_split)


def _magnitude_edge():
    out = []
    for d in sorted(BRIDGE_GEOMETRY):
        mk = (lambda d=d: bridge_entries(d, _three_motions(d)))
        out.append(_edge_case(f"edge-{d}-at", d, mk, mag_separate, True))
        out.append(_edge_case(f"edge-{d}-above", d, mk, lambda m: np.nextafter(mag_separate(m), F(np.inf)), False))
    up, down = _contraction_motions()
    for k, (d, v) in enumerate(zip((14, 17), up)):       # a contracted build finds the cell ON: target = the fused (larger) value
        out.append(_edge_case(f"contract-up{k}-{d}", d, lambda d=d, v=v: bridge_entries(d, v), lambda m: mag_fused(m)[0], False))
    for k, (d, v) in enumerate(zip((17, 33), down)):     # a contracted build finds the cell OFF: target = the separate (larger) value
        out.append(_edge_case(f"contract-down{k}-{d}", d, lambda d=d, v=v: bridge_entries(d, v), mag_separate, True))
    return tuple(out)


MAGNITUDE_EDGE = _magnitude_edge()
CONTRACTION = tuple(c for c in MAGNITUDE_EDGE if c.name.startswith("contract"))

# ---- NaN, infinities, signed zeros, positions outside the frame --------------------------------------------------------------------------
INF, NAN = F(np.inf), F(np.nan)
DENORM = F(1.401298464324817e-45)                        # the smallest f32: (-DENORM + 0) / 2 is the tie that rounds to -0.0
SPECIAL_SIDES = (14, 17)                                 # the one-workgroup densifier | the general path


def _piles(d):
    """the left blob and a (wl + 1) x hh blob in the last corner, whose cell 0 / last cell are lit ONLY by records with NaN or
    out-of-range positions"""
    wl, hh = BRIDGE_GEOMETRY[d]
    left, corner = _rect(0, 0, wl, hh), _rect(d - wl - 1, d - hh, wl + 1, hh)
    e = entries(d, [c for c in left if c != (0, 0)] + [c for c in corner if c != (d - 1, d - 1)], motion=STRONG)
    to_first = [(NAN, 0.5), (0.5, NAN), (-1.0, 0.5), (0.5, -0.25), (0.0, 0.0), (-INF, 0.3), (-0.0, 0.5), (NAN, NAN), (2.0, -2.0)]
    to_last = [(2.0, 0.5), (0.5, 1.0), (INF, 0.1), (1.0, 1.0), (0.999, 7.0), (INF, INF), (0.5, INF)]
    extra = np.array([p + STRONG for p in to_first + to_last], F)
    keep = ~(((e[:, 0] == positions(d)[0]) & (e[:, 1] == positions(d)[0])) | ((e[:, 0] == positions(d)[-1]) & (e[:, 1] == positions(d)[-1])))
    return np.ascontiguousarray(np.concatenate([extra[::2], e[keep], extra[1::2]]), dtype=F)     # (the two cells' still records dropped)


def _negzero(d):
    """no still records: with target_motion <= 0 every cell is on, the empty ones included.  Cells (1, 1) and (d - 2, d - 2) have the mean
    (-0.0, +0.0); cell (2, 1) has (-0.0, -0.0)"""
    on = [c for c in all_on(d) if (c[0] + c[1]) % 3 == 0 or c in ((1, 1), (d - 2, d - 2), (2, 1))]
    motions = [np.asarray(MOVE, F)] * len(on)
    for c in ((1, 1), (d - 2, d - 2)):
        motions[on.index(c)] = np.array([(-DENORM, 0.0), (0.0, 0.0)], F)
    motions[on.index((2, 1))] = np.array([(-DENORM, -DENORM), (0.0, 0.0)], F)
    return entries(d, on, motions=motions, background=False)


def _special(d):
    joined, split, seed_split = _bridge_areas(d)
    wl, hh = BRIDGE_GEOMETRY[d]
    hole = (wl + 2, 1)                                   # inside the right blob, not its seed
    pair = PAIR[d]
    mk = lambda f: lru_cache(maxsize=1)(f)
    return (
        # a NaN mean is off (NaN >= t is false): the bridge (NaN, y), a hole (x, NaN), and in the left blob +inf and -inf in one cell (NaN sum)
        Case(f"nan-{d}", d, params(pair), mk(lambda: bridge_entries(d, (NAN, 0.02), (hole, (0.02, NAN)), [(INF, 0.0), (-INF, 0.0)])), True,
             split - 1, seed_split),
        # infinite means are on and copied: the bridge (+inf, 0), a cell of the right blob (0, -inf), a cell of the left (-inf, +inf)
        Case(f"inf-{d}", d, params(pair), mk(lambda: bridge_entries(d, (INF, 0.0), (hole, (0.0, -INF)), (-INF, INF))), True, joined, 0),
        Case(f"negzero-target0-{d}", d, params(pair, 0.0), mk(lambda: _negzero(d)), True, d * d, 0),
        Case(f"negzero-negative-target-{d}", d, params(pair, -1.0), mk(lambda: _negzero(d)), True, d * d, 0),
        Case(f"piles-{d}", d, params(pair), mk(lambda: _piles(d)), True, (wl + 1) * hh, (d - hh) * d + d - wl - 1),
    )


SPECIAL_VALUES = tuple(c for d in SPECIAL_SIDES for c in _special(d))


# ---- the densifier's switch: n <= 8,192 records AND <= 256 cells take the one-workgroup kernel -------------------------------------------
def _many(d, n, seed):
    """n records at seeded positions, dozens per cell, whose cell means hover around TARGET: the sequential f32 sums decide which cells are on"""
    rng = np.random.default_rng(seed)
    e = np.empty((n, 4), F)
    e[:, :2] = rng.uniform(0.001, 0.999, (n, 2)).astype(F)
    e[:, 2] = (TARGET + rng.normal(0, 0.002, n)).astype(F)
    e[:, 3] = rng.normal(0, 0.002, n).astype(F)
    return e


def _switch_case(d, n, some, area, seed):
    return Case(f"switch-{d}-{n}", d, params(PAIR[d]), lru_cache(maxsize=1)(lambda: _many(d, n, 1000 * d + n)), some, area, seed)


DENSIFY_SWITCH = (_switch_case(16, 8191, True, 124, 2), _switch_case(16, 8192, True, 122, 1), _switch_case(16, 8193, True, 150, 2),
                  _switch_case(17, 1, False, 1, 264), _switch_case(17, 8192, True, 102, 13))

ALL_CASES = SHAPES + AREA_EQUALITY + MAGNITUDE_EDGE + SPECIAL_VALUES + DENSIFY_SWITCH
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# ---- batches for ofps_hip_detect_dev: items of equal n_per_item (one record per cell: lit or still) --------------------------------------
Batch = namedtuple("Batch", "name side params make")     # make() -> [batch, n_per_item, 4]


def _batch(name, d, shapes):
    return Batch(name, d, params(PAIR[d]), lru_cache(maxsize=1)(lambda: np.stack([entries(d, s(d)) for s in shapes])))


BATCHES = (
    _batch("batch-14x3", 14, (corner_blobs_anti, nothing, serpentine)),                   # the one-workgroup densifier, one item per workgroup
    _batch("batch-17x7", 17, (serpentine, nothing, last_first, all_on, spirals, antidiagonal, corner_blobs)),
    _batch("batch-33x3", 33, (k1024_blocks, nothing, spirals_extra)),
    _batch("batch-160x2", 160, (serpentine, all_on)),
    # dozens of records per cell in seeded order: the items' sorts and sequential sums, not one record per cell (which any order leaves right)
    Batch("batch-14x3-many", 14, params(PAIR[14]), lru_cache(maxsize=1)(lambda: np.stack([_many(14, 3000, 140 + k) for k in range(3)]))),
    Batch("batch-17x3-many", 17, params(PAIR[17]), lru_cache(maxsize=1)(lambda: np.stack([_many(17, 3000, 170 + k) for k in range(3)]))),
    Batch("batch-33x2-many", 33, params(PAIR[33]), lru_cache(maxsize=1)(lambda: np.stack([_many(33, 9000, 330 + k) for k in range(2)]))),
    Batch("batch-17x3-empty", 17, params(PAIR[17]), lambda: np.zeros((3, 0, 4), F)),          # n_per_item = 0
)
BATCH_BY_NAME = {b.name: b for b in BATCHES}


# ---- expectations -------------------------------------------------------------------------------------------------------------------------
_expected = {}


def expected(e, prm):
    """oracle.detect_motion, once per (records, parameters) -> (has, area, field[dim, dim, 2]); the field is all zero when has is False"""
    key = (e.shape, hash(e.tobytes()), tuple(sorted(prm.items())))
    if key not in _expected:
        r = oracle.detect_motion(e, **prm)
        d = oracle.block_dim(prm["min_size"], prm["subdivide"])
        out = (False, 0, np.zeros((d, d, 2), F)) if r is None else (True, r[0], r[1])
        out[2].setflags(write=False)
        _expected[key] = out
    return _expected[key]
