"""CPU tests of hip_sad's search levels (include/ofps_hip.h N1h): the restatement tests/indep_sad_hier.py against literals written out by
hand, against the oracle's plain search at levels 1, and on the planted shifts of tests/sad_hier_cases.py -- the statement that the
feature does what it is for -- and the header / library pair: the entry points are declared and exported.  No GPU call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from ofps_amd import _lib

import indep_sad_hier as ih
import sad_hier_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ofps_hip_set_sad_levels", "ofps_hip_get_sad_levels", "ofps_hip_sad_reach", "ofps_hip_sad_down2", "ofps_hip_sad_down2_dev",
               "ofps_hip_sad_refine", "ofps_hip_sad_refine_dev")


# ---------------------------------------------------------------- down2
@pytest.mark.parametrize("quad,want", [((1, 2, 2, 2), 2), ((0, 0, 0, 1), 0), ((0, 0, 1, 1), 1), ((255, 255, 255, 254), 255)])
def test_down2_rounds_half_up_on_the_sum_of_four(quad, want):
    assert ih.down2(np.array([quad[:2], quad[2:]], np.uint8)).tolist() == [[want]]


def test_down2_leaves_the_last_odd_column_and_row_unused():
    f = np.array([[10, 20, 30, 40, 250],
                  [10, 20, 30, 40, 250],
                  [99, 99, 99, 99, 99]], np.uint8)
    assert ih.down2(f).tolist() == [[15, 35]]            # 5 x 3 -> 2 x 1
    assert [p.shape for p in ih.pyramid(np.zeros((136, 200), np.uint8), 3)] == [(136, 200), (68, 100), (34, 50)]


def test_reach_follows_the_recurrence_and_the_ten_bit_bound():
    assert [ih.reach(8, L) for L in (1, 2, 3)] == [8, 19, 41]
    assert ih.reaches(8, 3) == [41, 19, 8]
    assert ih.reach(62, 2) == 127 and ih.reach(63, 2) is None
    assert ih.reach(29, 3) == 125 and ih.reach(30, 3) is None and ih.reach(32, 3) is None       # 32 -> 137
    assert ih.reach(64, 1) == 64 and ih.reach(65, 1) is None and ih.reach(8, 0) is None and ih.reach(8, 4) is None
    assert all(8 * ih.reach(r, L) + 6 <= 1023 for L in (2, 3) for r in range(65) if ih.reach(r, L) is not None)
    assert not ih.is_valid(24, 24, 16, 8, 2) and ih.is_valid(32, 32, 16, 8, 2)


# ---------------------------------------------------------------- refinement: tie-breaks and clamp, by hand
def test_a_flat_pair_returns_the_candidate_nearest_to_zero():
    """every candidate ties at SAD 0, so (d^2, dy, dx) decides: the valid candidate of the 7 x 7 window around the clamped predictor that is
    nearest to zero, the smaller dy, then the smaller dx among equals"""
    flat = np.full((48, 64), 90, np.uint8)                # 4 x 3 blocks of 16
    par = np.zeros((2 * 1, 3), np.int64).reshape(2, 3)    # parent lattice 2 x 1
    par[0] = (1, -1, 0)                                   # p = (2, -2): zero is inside the window
    par[1] = (5, 4, 0)                                    # p = (10, 8): the window is [7, 13] x [5, 11]
    best, n_valid = ih.refine(flat, flat, 16, par, 2, 1, 19)
    b = best.reshape(3, 4, 3)
    # block (0, 0): p clamps to (2, 0) (no room above): window x [-1, 5] -> valid x [0, 5], y [-3, 3] -> valid [0, 3]: zero wins
    assert b[0, 0].tolist() == [0, 0, 0] and n_valid[0] == 6 * 4
    # block (1, 1) (x0 16, y0 16): parent 0, p = (2, -2) unclamped: zero is a candidate
    assert b[1, 1].tolist() == [0, 0, 0] and n_valid[5] == 49
    # block (2, 1) (x0 32, y0 16): parent 1, p = (10, 8): nearest to zero is the window's corner (7, 5)
    assert b[1, 2].tolist() == [7, 5, 0]
    # block (3, 2) (x0 48, y0 32): p = (10, 8) clamps to (0, 0): x [-3, 0], y [-3, 0] valid
    assert b[2, 3].tolist() == [0, 0, 0] and n_valid[11] == 16
    # equal d^2: dy decides before dx -- a window that holds (-3, 4) and (4, -3) but nothing nearer
    par2 = np.array([[0, 0, 0]], np.int64)
    f2 = np.full((16, 16), 7, np.uint8)
    assert ih.refine(f2, f2, 16, par2, 1, 1, 3)[0].tolist() == [[0, 0, 0]]               # a one-block frame: only e = 0 is valid
    keys = sorted([(0, 25, 4 + 19, -3 + 19), (0, 25, -3 + 19, 4 + 19), (0, 25, -4 + 19, -3 + 19)])
    assert keys[0] == (0, 25, 15, 16)                                                   # dy = -4 first, whatever dx


def test_a_predictor_that_points_out_of_the_frame_is_clamped_at_every_edge():
    W, H, B = 64, 48, 16
    prev, cur = hc.refine_pair(W, H)
    x0s = np.arange(4) * B; y0s = np.arange(3) * B
    for kind in hc.PARENT_KINDS[2:]:
        par = hc.parents(kind, 2, 1)
        qx, qy = int(par[0, 0, 0]), int(par[0, 0, 1])
        best, n_valid = ih.refine(prev, cur, B, par.reshape(-1, 3), 2, 1, 127)
        for k, (dx, dy, _) in enumerate(best.tolist()):
            x0, y0 = int(x0s[k % 4]), int(y0s[k // 4])
            assert 0 <= x0 + dx <= W - B and 0 <= y0 + dy <= H - B
            px = min(max(2 * qx, -x0), W - B - x0); py = min(max(2 * qy, -y0), H - B - y0)
            assert abs(dx - px) <= 3 and abs(dy - py) <= 3
            # the clamp leaves the predictor ON the frame edge it pointed across: only the inward part of the window is valid there
            nx = sum(1 for e in range(-3, 4) if 0 <= x0 + px + e <= W - B)
            ny = sum(1 for e in range(-3, 4) if 0 <= y0 + py + e <= H - B)
            assert (nx == 4 or not qx) and (ny == 4 or not qy)
            assert n_valid[k] == nx * ny, (kind, k)


def test_the_parent_of_a_column_beyond_the_parent_lattice_is_the_last_one():
    # 200 x 136 at block 8: 25 columns, the parent lattice (100 x 68) has 12: column 24's parent would be 12 -> clamped to 11
    par = np.zeros((8 * 12, 3), np.int64)
    par[11::12, 0] = 2                                   # only the last parent column predicts (4, 0)
    assert ih.predictor(par, 12, 8, 24, 0, 192, 0, 8, 200, 136) == (0, 0)                # ... clamped: the block already touches the right edge
    assert ih.predictor(par, 12, 8, 23, 0, 184, 0, 8, 200, 136) == (4, 0)
    assert ih.predictor(par, 12, 8, 21, 0, 168, 0, 8, 200, 136) == (0, 0)                # parent 10


def test_levels_one_is_the_oracles_plain_search():
    prev, cur = hc.refine_pair(96, 64)
    ent, best, per_level = ih.search(prev, cur, 16, 8, 1)
    ent_o, best_o = oracle.sad_flow(prev, cur, 16, 8)
    np.testing.assert_array_equal(best, best_o)
    np.testing.assert_array_equal(ent.view(np.uint32), ent_o.view(np.uint32))           # entries(): N1's record arithmetic, bit for bit
    assert len(per_level) == 1


# ---------------------------------------------------------------- the planted shift
@pytest.mark.parametrize("i", range(len(hc.PLANTED)))
def test_planted_shift_beyond_the_range_is_found_by_every_reachable_block(i):
    W, H, B, R, L, d, n_reach, n_blk = hc.PLANTED[i]
    prev, cur, ent, best, per_level = hc.planted_expect(i)
    assert max(abs(d[0]), abs(d[1])) > R and max(abs(d[0]), abs(d[1])) <= ih.reach(R, L)
    reach = hc.reachable(W, H, B, L, d)
    print(f"case {i}: {int(reach.sum())} of {len(reach)} blocks fall under the rule")
    assert (int(reach.sum()), len(reach)) == (n_reach, n_blk)
    hit = (best[:, 0] == d[0]) & (best[:, 1] == d[1])
    assert not (reach & ~hit).any(), np.flatnonzero(reach & ~hit)
    plain = oracle.sad_flow(prev, cur, B, R)[1]
    assert not ((plain[:, 0] == d[0]) & (plain[:, 1] == d[1])).any()                    # the plain search finds d for no block
    assert np.abs(best[:, :2]).max() <= ih.reach(R, L)
    np.testing.assert_array_equal(ent.view(np.uint32), ih.entries(best, B, W, H).view(np.uint32))
    if (W, H, B) == (200, 136, 8):
        assert W // B == 25 and (W >> 1) // B == 12                                     # lattice column 24: no parent of its own
        assert not reach.reshape(H // B, W // B)[:, 24].any()


# ---------------------------------------------------------------- header and library
def test_the_header_declares_the_new_entry_points_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofps_hip.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/ofps_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by libofps_hip.so"
        assert name in _lib.PROTOTYPES
    assert "OFPS_HIP_API_VERSION 2" in text
    # the pure helper needs no device
    reach = _lib.load().ofps_hip_sad_reach
    for R in range(0, 66):
        for L in range(0, 5):
            want = ih.reach(R, L)
            got = reach(R, L)
            assert (got == want) if want is not None else (got < 0), (R, L, got)
