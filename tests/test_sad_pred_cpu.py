"""CPU tests of the neighbour and zero predictors of hip_sad's search levels (include/ofps_hip.h N1p): the restatement
tests/indep_sad_pred.py on the two-motion scenes of tests/sad_pred_cases.py -- the statement that the feature does what it is for --
against the one-predictor restatement at mode 0, and the header / library pair.  No GPU call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ofps_amd import _lib

import indep_sad_hier as ih
import indep_sad_pred as ip
import sad_hier_cases as hc
import sad_pred_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ofps_hip_set_sad_predictors", "ofps_hip_get_sad_predictors", "ofps_hip_sad_refine_pred", "ofps_hip_sad_refine_pred_dev")
SCENES = range(len(pc.TWO_MOTIONS))


def test_the_predictor_list_by_hand():
    # parent lattice 3 x 2, block 16 in a 96 x 64 frame (6 x 4 blocks); winners chosen so that every doubled vector stays inside
    par = np.zeros((6, 3), np.int64)
    par[:, 0] = (1, 2, 3, 4, 5, 6)
    par[:, 1] = (-1, -2, -3, 1, 2, 3)
    # block (2, 2): parent (1, 1) = index 4; neighbours left 3, right 5, above 1; none below
    got = ip.predictors(par, 3, 2, 2, 2, 32, 32, 16, 96, 64, ip.PRED_NEIGHBOURS)
    assert got == [(10, 4), (8, 2), (12, 6), (4, -4), (0, 0)]
    assert ip.predictors(par, 3, 2, 2, 2, 32, 32, 16, 96, 64, ip.PRED_PARENT) == [(10, 4)]
    # block (0, 0): parent (0, 0); no left, no above; every predictor clamped on its own (x >= 0 and y >= 0 here)
    got = ip.predictors(par, 3, 2, 0, 0, 0, 0, 16, 96, 64, ip.PRED_NEIGHBOURS)
    assert got == [(2, 0), (4, 0), (8, 2), (0, 0)]
    # a 1 x 1 parent lattice: the parent and zero
    assert ip.predictors(par[:1], 1, 1, 1, 0, 16, 0, 16, 32, 16, ip.PRED_NEIGHBOURS) == [(0, 0), (0, 0)]


@pytest.mark.parametrize("i", SCENES)
def test_mode_zero_is_the_one_predictor_restatement(i):
    W, H, B, R, L, bnd, dl, dr = pc.TWO_MOTIONS[i][:8]
    prev, cur, ent, best, _ = pc.two_motion_expect(i, ip.PRED_PARENT)
    ent_h, best_h, _ = ih.search(prev, cur, B, R, L)
    np.testing.assert_array_equal(best, best_h)
    np.testing.assert_array_equal(ent.view(np.uint32), ent_h.view(np.uint32))


@pytest.mark.parametrize("i", SCENES)
def test_two_motions_every_block_under_the_rule_returns_its_sides_vector(i):
    W, H, B, R, L, bnd, dl, dr, n_under, n_blk, n_miss0 = pc.TWO_MOTIONS[i]
    assert bnd % (2 * B) == B                                                            # the middle of a parent block's column
    assert all(max(abs(d[0]), abs(d[1])) <= ih.reach(R, L) for d in (dl, dr))
    under, want = pc.rule(W, H, B, L, bnd, dl, dr)
    assert (int(under.sum()), len(under)) == (n_under, n_blk)
    best0 = pc.two_motion_expect(i, ip.PRED_PARENT)[3]
    best1 = pc.two_motion_expect(i, ip.PRED_NEIGHBOURS)[3]
    miss0, miss1 = pc.misses(best0, under, want), pc.misses(best1, under, want)
    ins = pc.inside(W, H, B, want, bnd)
    print(f"scene {i}: {n_under} of {n_blk} under the rule, mode 0 misses {int(miss0.sum())}, mode 1 {int(miss1.sum())}; of the {int(ins.sum())} "
          f"blocks whose displaced block lies inside the frame mode 0 misses {int(pc.misses(best0, ins, want).sum())}, mode 1 "
          f"{int(pc.misses(best1, ins, want).sum())}")
    assert not miss1.any(), np.flatnonzero(miss1)
    assert int(miss0.sum()) == n_miss0 and n_miss0 >= 1
    assert np.abs(best1[:, :2]).max() <= ih.reach(R, L)


@pytest.mark.parametrize("i", [i for i in SCENES if pc.TWO_MOTIONS[i][4] == 2])
def test_at_levels_two_the_winner_key_never_gets_worse(i):
    """the parents are the top search's in both modes and mode 1's candidates are a superset (not so at levels 3: level 1's winners differ)"""
    k0 = pc.two_motion_expect(i, ip.PRED_PARENT)[4]
    k1 = pc.two_motion_expect(i, ip.PRED_NEIGHBOURS)[4]
    assert len(k0) == len(k1) and all(a <= b for a, b in zip(k1, k0))
    assert any(a < b for a, b in zip(k1, k0))


def test_refine_counts_distinct_predictors_on_the_synthetic_parents():
    W, H, B = 64, 48, 16
    prev, cur = hc.refine_pair(W, H)
    pnbx, pnby = hc.parent_lattice(W, H, B)
    assert (pnbx, pnby) == (2, 1)
    n = {kind: ip.refine(prev, cur, B, hc.parents(kind, pnbx, pnby).reshape(-1, 3), pnbx, pnby, 127, ip.PRED_NEIGHBOURS)[2] for kind in ("zero", "alternating")}
    assert (n["zero"] == 1).all()                                                       # parent, neighbour and zero coincide
    assert n["alternating"].max() == 3                                                  # parent, one neighbour, zero: a 2 x 1 lattice
    assert (ip.refine(prev, cur, B, hc.parents("alternating", pnbx, pnby).reshape(-1, 3), pnbx, pnby, 127, ip.PRED_PARENT)[2] == 1).all()


def test_the_header_declares_the_new_entry_points_and_the_library_exports_them():
    raw = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/ofps_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by libofps_hip.so"
        assert name in _lib.PROTOTYPES
    assert re.search(r"#define\s+OFPS_HIP_SAD_PRED_PARENT\s+0\b", text) and re.search(r"#define\s+OFPS_HIP_SAD_PRED_NEIGHBOURS\s+1\b", text)
    assert "OFPS_HIP_API_VERSION 2" in text and "N1p" in raw
