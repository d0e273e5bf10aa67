"""Case lists for the island list of the block-motion detector (include/ofps_hip.h A5i; ofps_amd/csrc/detect.hip).  CPU only: the shape
builders and entries() of tests/detect_cases.py, numpy, the oracle and the plain-Python restatement tests/indep_detect_islands.py -- never
the library under test.  tests/test_detect_islands_cpu.py proves the restatement and the literals; tests/test_detect_islands_gpu.py runs
the cases.  Every expectation is bit equality."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import detect_cases as dc
import indep_detect_islands as indep
import oracle

F = np.float32
SIDES = (1, 2, 3, 4, 14, 17, 33, 64, 65, 160)
EQUAL_SIDES = (4, 9, 17, 33, 64, 65, 128, 160)


# ---- two (min_size, subdivide) families whose side is d itself ---------------------------------------------------------------------------
def pair_area2(d):
    """min_size half way between 1 / d^2 and 1 / (d - 1)^2: an island of area 2 qualifies, one of area 1 does not (d >= 4)"""
    assert d >= 4
    return (float(F((1.0 / d ** 2 + 1.0 / (d - 1) ** 2) / 2.0)), 1)


def pair_area1(d):
    """min_size = f32(1 / d^2): area 1 qualifies exactly at equality (not at side 14, where the side becomes 15)"""
    assert d in EQUAL_SIDES
    return (float(F(1.0 / d ** 2)), 1)


def pair_of(d, family):
    if d < 4:
        return dc.PAIR[d]                                                # sides 1, 2, 3: the detector's own grid pairs
    return pair_area2(d) if family == "a2" else pair_area1(d)


# ---- one more shape -----------------------------------------------------------------------------------------------------------------------
def dominoes(d):
    """horizontal dominoes every third column and second row, clipped at the last column: ceil(d / 3) x ceil(d / 2) isolated islands, of
    area 2 but a row's last one where d % 3 == 1 (area 1).  Side 160: 4,320 components, 4,240 of them whole dominoes"""
    return [(x + k, y) for y in range(0, d, 2) for x in range(0, d, 3) for k in (0, 1) if x + k < d]


def equality_beside(d, a):
    """the first `a` cells of their square block at the origin -- the island exactly at the bound -- and a - 1 cells filled column by column
    from the last column: one cell smaller, well apart"""
    big = dc.first_cells(d, a)
    small = [(d - 1 - k // d, k % d) for k in range(a - 1)]
    assert not small or min(x for x, _ in small) > max(x for x, _ in big) + 1
    return big + small


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
# name; side; the detector's parameters; make() -> records; n_islands / n_components as literals where the shape gives them (else None)
Case = namedtuple("Case", "name side params make n_islands n_components")


def _case(shape, d, family, n_islands=None, n_components=None, name=None):
    pair = pair_of(d, family)
    return Case(f"{name or shape.__name__}-{d}-{family}", d, dc.params(pair), lru_cache(maxsize=1)(lambda: dc.entries(d, shape(d))), n_islands, n_components)


def _half(d):
    return (d + 1) // 2


def _n_dominoes(d, whole=False):
    return ((d + 1) // 3 if whole else (d + 2) // 3) * _half(d)


CASES = tuple(
    [_case(dc.nothing, d, "a2", 0, 0) for d in (1, 3, 14, 160)] +
    [_case(dc.one_cell, 1, "a2", 1, 1), _case(dc.one_cell, 2, "a2", 1, 1), _case(dc.one_cell, 14, "a2", 0, 1), _case(dc.one_cell, 17, "a1", 1, 1),
     _case(dc.one_cell, 160, "a1", 1, 1), _case(dc.one_cell, 160, "a2", 0, 1)] +
    [_case(dc.all_on, d, "a2", 1, 1) for d in SIDES] +
    # isolated cells: tied islands of area 1, ordered purely by seed -- or none at all
    [_case(dc.lattice, d, "a1", _half(d) ** 2, _half(d) ** 2) for d in (4, 17, 33, 65, 160)] +
    [_case(dc.lattice, d, "a2", 0, _half(d) ** 2) for d in (4, 14, 17, 33, 64, 65, 160)] +
    [_case(dominoes, d, "a2", _n_dominoes(d, whole=True), _n_dominoes(d)) for d in (4, 14, 17, 33, 64, 65, 160)] +
    [_case(dominoes, d, "a1", _n_dominoes(d), _n_dominoes(d)) for d in (17, 160)] +
    [_case(dc.serpentine, d, "a2", 1, 1) for d in (14, 17, 33, 65, 160)] +
    [_case(dc.last_first, d, "a2", 1, 1) for d in (4, 14, 33, 65, 160)] +
    [_case(dc.spirals, d, "a2", 2, 2) for d in (17, 33, 64, 160)] +
    [_case(dc.spirals_extra, d, "a2", 2, 2) for d in (17, 33, 64, 160)] +
    [_case(dc.corner_blobs, d, "a2", 1, 1) for d in (4, 14, 17, 65)] +
    [_case(dc.corner_blobs_anti, d, "a2", 1, 1) for d in (4, 14, 17, 65)] +
    [_case(dc.antidiagonal, d, "a2", 1, 1) for d in (2, 14, 33, 160)] +
    [_case(dc.far_edge_lines, d, "a2", 2, 2) for d in (33, 64, 65, 160)] +
    [_case(dc.k1024_blocks, d, "a2") for d in (33, 64, 65, 160)] +
    [_case(dc.block_lattice, 64, "a2", 4, 4), _case(dc.block_lattice, 160, "a2", 25, 25)]
)


def _equality(m, s, a):
    d = oracle.block_dim(m, s)
    return Case(f"equal-beside-{m}-{s}", d, dc.params((m, s)), lru_cache(maxsize=1)(lambda: dc.entries(d, equality_beside(d, a))), 1, 2 if a > 1 else 1)


AREA_EQUALITY = tuple(_equality(m, s, a) for m, s, a in dc.AREA_EQUALITY_PAIRS)
# cells at the threshold itself: the detector's own edge cases, read as island lists
MAGNITUDE_EDGE = tuple(Case("islands-" + c.name, c.side, c.params, c.make, None, None) for c in dc.MAGNITUDE_EDGE)

ALL_CASES = CASES + AREA_EQUALITY + MAGNITUDE_EDGE
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

_reference = {}


def reference(e, prm):
    """the restatement's full ranking, once per (records, parameters); read-only"""
    key = (e.shape, hash(e.tobytes()), tuple(sorted(prm.items())))
    if key not in _reference:
        _reference[key] = indep.islands(e, **prm)
    return _reference[key]


def k_values(n_islands):
    """truncation, labels 0xFFFF beyond K, n_islands reported in full: 1, 2, n - 1, n, n + 1 and the maximum"""
    return sorted({k for k in (1, 2, n_islands - 1, n_islands, n_islands + 1, indep.MAX_ISLANDS) if 1 <= k <= indep.MAX_ISLANDS})


# ---- frames for the fused forms: a planted moving rectangle on still texture ----------------------------------------------------------------
FW, FH, BLOCK, RANGE = 128, 96, 8, 8
FUSED = dict(block=BLOCK, search_range=RANGE, min_size=0.02, subdivide=2, target_motion=0.003)      # side 15; a block's motion is n / 128: well clear


@lru_cache(maxsize=None)
def frames(n=5, seed=33):
    """n luma frames: seeded texture that stays, a flat band in the bottom-left corner (nothing for the contrast gate to keep), two
    textured rectangles that move 2 and 3 pixels per frame"""
    rng = np.random.default_rng(seed)
    back = rng.integers(0, 256, (FH, FW), dtype=np.uint8)
    back[72:96, 0:64] = 128
    obj_a = rng.integers(0, 256, (24, 32), dtype=np.uint8)
    obj_b = rng.integers(0, 256, (24, 24), dtype=np.uint8)
    out = np.empty((n, FH, FW), np.uint8)
    for k in range(n):
        f = back.copy()
        f[16:40, 8 + 2 * k:40 + 2 * k] = obj_a
        f[56:80, 96 - 3 * k:120 - 3 * k] = obj_b
        out[k] = f
    out.setflags(write=False)
    return out
