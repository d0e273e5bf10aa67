"""CPU: the restatement tests/indep_sad_intra.py gives what the cases of tests/sad_intra_cases.py derive by hand, and the planted scene
separates the ratios: the numbers tests/test_sad_intra_gpu.py relies on when it holds the library to the restatement."""
import numpy as np
import pytest

import indep_sad_intra as ii
import sad_intra_cases as ic
import sad_median_cases as mc


@pytest.mark.parametrize("name", list(ic.ACTIVITY))
def test_activity_of_the_derived_cases(name):
    frame, block, want = ic.ACTIVITY[name]()
    got = ii.activity(frame, block)
    assert got.dtype == np.uint32 and got.tolist() == want


def test_largest_activity_is_block_64_half_and_half():
    frame, block, want = ic.ACTIVITY["largest"]()
    assert max(want) == 522240 == 2048 * 128 + 2048 * 127 < 255 * 4096


def test_shapes_have_ragged_margins_and_cover_every_path():
    blocks = {b for _, _, b, _ in ic.SHAPES}
    assert {8, 16} <= blocks and blocks - {8, 16}                    # the lattice path and the general one
    assert any(W % b and H % b for W, H, b, _ in ic.SHAPES)
    assert any(s % 4 for _, _, b, s in ic.SHAPES if b in (8, 16)) and any(s % 16 == 0 for _, _, b, s in ic.SHAPES if b in (8, 16))
    for W, H, b, s in ic.SHAPES:
        a = ic.shape_activity(W, H, b, s)
        assert len(a) == (W // b) * (H // b) and (b == 1 or a.max() > 0)
        assert (ic.shape_frame(W, H, s)[:, W:] == 255).all()


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("ratio", ic.RATIOS)
def test_verdicts_of_the_derived_field(ratio, gated):
    best, act, kin = ic.field(gated)
    keep, counts, is_cut = ii.verdict(best, act, kin, ratio)
    np.testing.assert_array_equal(keep, ic.field_keep(ratio, gated))
    assert counts == ic.FIELD_COUNTS[(ratio, gated)] and not is_cut
    if gated:
        assert not (keep & ~np.array(ic.FIELD_GATE, np.uint8) & 1).any()                # unkept blocks never come back


@pytest.mark.parametrize("gated", [False, True])
def test_cut_rule_on_the_derived_field(gated):
    best, act, kin = ic.field(gated)
    cut_at, none_at = ic.FIELD_CUT[gated]
    keep, counts, is_cut = ii.verdict(best, act, kin, 8, cut_at)
    assert is_cut and not keep.any() and counts == ic.FIELD_COUNTS[(8, gated)]
    keep, _, is_cut = ii.verdict(best, act, kin, 8, none_at)
    assert not is_cut
    np.testing.assert_array_equal(keep, ic.field_keep(8, gated))
    assert not ii.verdict(best, act, kin, 8, 0)[2]
    keep, counts, is_cut = ii.verdict(best, act, np.zeros(12, np.uint8), 8, 1)          # no candidate: a cut
    assert is_cut and counts == (0, 0) and not keep.any()
    assert not ii.verdict(best, act, np.zeros(12, np.uint8), 8, 0)[2]


def test_scene_separates_the_ratios():
    _, F = mc.scene_vectors()
    planted = (F[:, 0] == mc.SCENE_D[0]) & (F[:, 1] == mc.SCENE_D[1])
    assert int(planted.sum()) == 72
    noise = [by * mc.SCENE_NBX + bx for bx, by in mc.SCENE_NOISE]
    keep = {q: ic.scene_keep(q).astype(bool) for q in ic.SCENE_RATIOS}
    assert {q: int(k.sum()) for q, k in keep.items()} == ic.SCENE_KEPT
    np.testing.assert_array_equal(keep[4], planted)                                     # exactly the blocks whose winner is (5, -3)
    extra = np.flatnonzero(keep[8] & ~planted)
    assert extra.tolist() == [0 * mc.SCENE_NBX + 4]                                     # ... plus block (4, 0)
    assert int(keep[16][noise].sum()) == 3                                              # the encoder's literal rule lets three noise blocks through
    # the safe blocks are kept at the three ratios and at everything between 2 and 16.  (q = 1 asks for SAD < A / 16, which the interpolated
    # planted texture does not give every block: the verdict is monotonic in q, so 2 is the strictest ratio that holds all 29.)
    for q in range(2, 17):
        assert ic.scene_keep(q)[mc.scene_safe_blocks()].all(), q
    assert not ic.scene_keep(1)[mc.scene_safe_blocks()].all()
    assert int(mc.scene_safe_blocks().sum()) == 29


def test_scene_cut_threshold():
    _, (n_cand, n_intra), _ = ii.verdict(mc.scene_vectors()[1], ic.scene_activity(), None, ic.SCENE_Q)
    assert (n_cand, n_intra) == (mc.SCENE_NBLK, ic.SCENE_INTRA_AT_Q) == (96, 23)
    assert 100 * 23 < ic.SCENE_NO_CUT * 96 and 100 * 23 >= ic.SCENE_CUT * 96
    assert ic.scene_keep(ic.SCENE_Q, cut=ic.SCENE_NO_CUT).sum() == ic.SCENE_KEPT[ic.SCENE_Q]
    assert ic.scene_keep(ic.SCENE_Q, cut=ic.SCENE_CUT).sum() == 0


def test_noise_against_noise_is_all_intra():
    _, _, _, F = mc.sparse_pair()
    act = ic.sparse_activity()
    assert (F[:, 2] > act).all()                                                        # every SAD exceeds its activity
    for q in range(1, 17):
        assert not ii.keep_flags(F, act, None, q).any()


def test_synthetic_lattice_has_equalities_and_a_partial_workgroup():
    best, act, kin = ic.synthetic(120, 67)
    assert len(best) % 256 != 0
    eq = 16 * best[:, 2].astype(np.int64) == 8 * act.astype(np.int64)
    assert eq.sum() > 100 and 0 < ii.keep_flags(best, act, kin, 8).sum() < kin.sum()


def test_stream_with_a_cut():
    for k in range(1, 6):
        ent, best, (n_cand, n_intra) = ic.stream_expect(k)
        assert len(ent) == len(best) == ic.STREAM_KEPT[k] and n_cand == mc.SCENE_NBLK, k
        if k in (2, 3):                                                                 # cuts by the rule: records are lost to it
            assert 100 * n_intra >= ic.STREAM_P * n_cand and n_intra < n_cand
            assert len(ic.stream_expect(k, cut=0)[0]) == n_cand - n_intra > 0
    assert len(ic.stream_expect(2, cut=0)[0]) == ic.STREAM_KEPT_WITHOUT_CUT[2]
    assert len(ic.stream_expect(1, cut=ic.SCENE_CUT)[0]) == 0 and len(ic.stream_expect(1, cut=ic.SCENE_NO_CUT)[0]) == 73
