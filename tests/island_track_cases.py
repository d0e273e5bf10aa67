"""Case lists for the island tracks (include/ofps_hip.h A5t; ofps_amd/csrc/detect_tracks.hip).  CPU only: the shape builders and entries()
of tests/detect_cases.py, numpy and the restatements -- never the library under test.  tests/test_island_tracks_cpu.py proves the
restatement on the hand-derived sequences below; tests/test_island_tracks_gpu.py runs them.  Every expectation is equality."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import detect_cases as dc
import detect_islands_cases as ic
import indep_island_tracks as indep

F = np.float32


def rect(x0, y0, w, h):
    return [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]


# ---- hand-derived sequences on an 8 x 8 grid --------------------------------------------------------------------------------------------------
# min_size = 1 / 64 exactly, subdivide 1: side 8, and an island of one cell qualifies at equality
PRM8 = dc.params((1.0 / 64.0, 1))
K8 = 8
# name; frames: the lit cells of each; T, reach, G; want: per frame the rows (id, slot, age, hits) in rank order
Hand = namedtuple("Hand", "name frames T reach G want")

_bar = rect(1, 2, 5, 2)
_pieces = rect(1, 2, 3, 2) + rect(5, 2, 1, 2)
_e_both = rect(0, 0, 3, 3) + rect(5, 0, 1, 2)
_two = rect(0, 0, 2, 2) + [(5, 5)]

HAND = (
    # A: one cell that moves a cell per frame.  Reach 0 never overlaps: a new id per frame; the old slot is freed BEHIND the matching, so
    # the slots alternate.  Reach 1 sees the neighbour cell
    Hand("A-reach0", [[(k + 1, 3)] for k in range(4)], 4, 0, 0, [[(1, 0, 1, 1)], [(2, 1, 1, 1)], [(3, 0, 1, 1)], [(4, 1, 1, 1)]]),
    Hand("A-reach1", [[(k + 1, 3)] for k in range(4)], 4, 1, 0, [[(1, 0, k + 1, k + 1)] for k in range(4)]),
    # B: 2 x 2 moving a cell per frame overlaps its footprint in two cells
    Hand("B", [rect(k, 3, 2, 2) for k in range(4)], 4, 0, 0, [[(1, 0, k + 1, k + 1)] for k in range(4)]),
    # C: an island, two empty frames, the island again: t = 4, born 1, so age 4; hits counts the frames it was seen in
    Hand("C-gap2", [rect(2, 2, 2, 2), [], [], rect(2, 2, 2, 2)], 4, 0, 2, [[(1, 0, 1, 1)], [], [], [(1, 0, 4, 2)]]),
    Hand("C-gap1", [rect(2, 2, 2, 2), [], [], rect(2, 2, 2, 2)], 4, 0, 1, [[(1, 0, 1, 1)], [], [], [(2, 0, 1, 1)]]),
    # D: a 5 x 2 bar, its 3 x 2 and 1 x 2 pieces (the larger piece is rank 0 and claims first), the bar again (6 pairs against 2)
    Hand("D", [_bar, _pieces, _bar], 4, 0, 0, [[(1, 0, 1, 1)], [(1, 0, 2, 2), (2, 1, 1, 1)], [(1, 0, 3, 3)]]),
    # E: 3 x 3 and 1 x 2, their 6 x 3 union (9 pairs against 2; slot 1 is freed), both again: the small one's cells are slot 0's by now,
    # slot 0 is claimed by rank 0, so it starts id 3 in the lowest free slot
    Hand("E", [_e_both, rect(0, 0, 6, 3), _e_both], 4, 0, 0, [[(1, 0, 1, 1), (2, 1, 1, 1)], [(1, 0, 2, 2)], [(1, 0, 3, 3), (3, 1, 1, 1)]]),
    # F: one slot, two islands: rows = min(n_listed, T) = 1
    Hand("F", [_two, _two], 1, 0, 0, [[(1, 0, 1, 1)], [(1, 0, 2, 2)]]),
    # G: (1, 1) is rank 0 (the smaller seed) and id 1, (3, 1) id 2; the one island between them sees one pair of each: the smaller id wins
    Hand("G", [[(1, 1), (3, 1)], [(2, 1)]], 4, 1, 0, [[(1, 0, 1, 1), (2, 1, 1, 1)], [(1, 0, 2, 2)]]),
    # H: the one slot is reused, the id is not
    Hand("H", [[(1, 1)], [], [(5, 5)], [(5, 5)]], 1, 0, 0, [[(1, 0, 1, 1)], [], [(2, 0, 1, 1)], [(2, 0, 2, 2)]]),
)
HAND_BY_NAME = {h.name: h for h in HAND}


def hand_frames(h):
    return [dc.entries(8, cells) for cells in h.frames]


# ---- seeded random sequences ------------------------------------------------------------------------------------------------------------------
def pair_of(d):
    """a (min_size, subdivide) with side d: an island of one cell qualifies where such a pair exists, else one of two"""
    return ic.pair_of(d, "a1" if d in ic.EQUAL_SIDES else "a2")


@lru_cache(maxsize=None)
def random_sequence(d, n_frames=12, seed=0, n_obj=4):
    """n_frames record arrays of d x d records each: a few rectangles on a random walk that vanish now and then, every lit cell with a motion of
    its own above the threshold (and below 64), every other cell one still record -> a tuple of read-only arrays"""
    rng = np.random.default_rng(1000 * d + seed)
    objs = [[int(rng.integers(0, d)), int(rng.integers(0, d)), int(rng.integers(1, max(2, d // 3 + 1))), int(rng.integers(1, max(2, d // 3 + 1)))]
            for _ in range(n_obj)]
    out = []
    for _ in range(n_frames):
        lit = set()
        for o in objs:
            o[0] = int(np.clip(o[0] + rng.integers(-2, 3), 0, d - 1))
            o[1] = int(np.clip(o[1] + rng.integers(-2, 3), 0, d - 1))
            if rng.random() < 0.25:                                       # not seen in this frame
                continue
            lit |= {(x, y) for x, y in rect(o[0], o[1], o[2], o[3]) if x < d and y < d}
        on = sorted(lit, key=lambda c: (c[1], c[0]))
        sign = rng.choice(np.array([-1.0, 1.0], F), (len(on), 2))
        motions = (sign * rng.uniform(0.01, 0.05, (len(on), 2))).astype(F)
        e = dc.entries(d, on, motions=list(motions) if on else None)
        e.setflags(write=False)
        out.append(e)
    return tuple(out)


RANDOM_SIDES_CPU = (1, 2, 3, 14, 17)
RANDOM_SIDES_GPU = (1, 2, 3, 4, 14, 17, 64, 65, 160)
REACH_GAP = tuple((r, g) for r in (0, 1, 4) for g in (0, 1, 3))
RANDOM_K, RANDOM_T = 8, 3             # four objects on three slots: untracked rows occur


def params_of(d):
    return dc.params(pair_of(d) if d >= 4 else dc.PAIR[d])


_reference = {}


def reference(frames, prm, K, T, reach, G, with_cells=True):
    """the restatement's answer for one whole sequence from a fresh tracker, once per argument set; read-only"""
    key = (tuple(hash(e.tobytes()) for e in frames), tuple(sorted(prm.items())), K, T, reach, G, with_cells)
    if key not in _reference:
        _reference[key] = indep.run(frames, prm, K, T, reach, G, None, with_cells)
    return _reference[key]


# ---- frames for the fused forms: two textured rectangles that move towards each other, cross and part --------------------------------------------
FW, FH, BLOCK, RANGE = ic.FW, ic.FH, ic.BLOCK, ic.RANGE
FUSED = dict(ic.FUSED)
N_FUSED = 10


@lru_cache(maxsize=None)
def frames(n=N_FUSED, seed=45):
    """n luma frames on still texture: rectangle a (24 rows x 24) moves 8 pixels right per frame, rectangle b (24 rows x 16, drawn above a,
    sharing four of its rows) 8 pixels left: apart in frames 0 .. 4, over each other in 5 and 6, apart again from 7 on -- the blocks they
    have just left move as well, so their islands part a frame or two later"""
    rng = np.random.default_rng(seed)
    back = rng.integers(0, 256, (FH, FW), dtype=np.uint8)
    obj_a = rng.integers(0, 256, (24, 24), dtype=np.uint8)
    obj_b = rng.integers(0, 256, (24, 16), dtype=np.uint8)
    out = np.empty((n, FH, FW), np.uint8)
    for k in range(n):
        f = back.copy()
        f[16:40, 16 + 8 * k:40 + 8 * k] = obj_a
        f[36:60, 104 - 8 * k:120 - 8 * k] = obj_b
        out[k] = f
    out.setflags(write=False)
    return out
