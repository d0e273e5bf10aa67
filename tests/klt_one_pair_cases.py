"""Seeded inputs for the identity hip_klt's one driver rests on: a batch of two frames IS the one-pair call (tests/test_klt_one_pair_is_a_batch_*).
The repainted pair of tests/klt_cases.py -- a small warp, a rectangle of it replaced by unrelated content, so that every setting below keeps
some tracks and drops others -- under six settings at two cells, and what the CPU restatements keep there.  Pure functions of their arguments;
nothing here calls the library."""
import functools

import klt_cases as kc
import klt_intra_cases as ic

W, H = 128, 96
LEVELS, RADIUS, ITERS = ic.SET                               # 2, 4, 10
CELLS = (8, 16)
MIN_SCORE = 900000                                           # above the best score of 104 of the 192 cells of 8 x 8, and of 5 of the 48 of 16 x 16
FB, Q, CUT = 256, ic.Q, 50                                   # N3f's limit (1/256 pixel), N3i's ratio (sixteenths) and cut (percent)
# name -> (mean_removal, fb_limit, intra ratio, cut)
SETTINGS = {"plain": (0, 0, 0, 0), "n3m": (1, 0, 0, 0), "n3f": (0, FB, 0, 0), "n3m_n3f": (1, FB, 0, 0), "intra_cut": (0, 0, Q, CUT),
            "n3f_intra": (0, FB, Q, 0)}
ROWS = [(name, cell) for name in SETTINGS for cell in CELLS]
PADDED_ROW, NO_SLOTS_ROW = ("n3f_intra", 8), ("n3m_n3f", 16)   # once with rows padded by 13 bytes, once with d_out_slots null
PAD = 13

# the 2048 x 1032 row: 33,024 slots at cell 8, above the 32,768 records the one-workgroup compaction takes
LARGE = dict(W=2048, H=1032, cell=8, levels=1, radius=1, iters=1, seed=3, slots=33024, kept_above=32768 // 2)

# what tests/indep_klt_intra.py keeps per row, (plain call, call started from the plain call's own slots): (kept, status 5, status 6)
PINNED = {("plain", 8): ((88, 0, 0), (88, 0, 0)), ("plain", 16): ((43, 0, 0), (43, 0, 0)),
          ("n3m", 8): ((88, 0, 0), (88, 0, 0)), ("n3m", 16): ((43, 0, 0), (43, 0, 0)),
          ("n3f", 8): ((74, 14, 0), (75, 13, 0)), ("n3f", 16): ((34, 9, 0), (35, 8, 0)),
          ("n3m_n3f", 8): ((77, 11, 0), (78, 10, 0)), ("n3m_n3f", 16): ((36, 7, 0), (35, 8, 0)),
          ("intra_cut", 8): ((67, 0, 21), (67, 0, 21)), ("intra_cut", 16): ((32, 0, 11), (32, 0, 11)),
          ("n3f_intra", 8): ((67, 14, 7), (67, 14, 7)), ("n3f_intra", 16): ((32, 9, 2), (32, 9, 2))}


def bounds_hold(name, cell, tally_, slots):
    """what keeps a row from passing on empty or trivially full output: some tracks kept and some not, and the row's own status present"""
    kept, no_return, intra = tally_
    _, fb, q, _ = SETTINGS[name]
    return 0 < kept < slots and (fb == 0 or no_return >= 1) and (q == 0 or intra >= 1)


def pair():
    return kc.repaint_pair(W, H)


@functools.lru_cache(maxsize=None)
def expect(name, cell, predicted):
    """the restatement's answer of one row; predicted: the tracks start from the guesses made from the unpredicted answer's slots"""
    import indep_klt_intra as ii
    zm, fb, q, cut = SETTINGS[name]
    prev, cur = pair()
    prev_slots = expect(name, cell, False)["slots"] if predicted else None
    return ii.flow_from(prev, cur, LEVELS, RADIUS, ITERS, prev_slots, q, cut, cell=cell, min_score=MIN_SCORE, mean_removal=bool(zm), fb_limit=fb)


def tally(slots):
    """raw slots [n, 6] -> (kept, status 5, status 6)"""
    st = slots[:, 5]
    return int((st == 0).sum()), int((st == 5).sum()), int((st == 6).sum())
